"""Float64 NumPy restatement of the NMF updates with the L1/L2 penalty on the codes (test infrastructure only).

The objective is  loss(y, x D) + l1 sum(x) + l2/2 |x|^2  with D's rows at unit norm:
  MU    x <- x * max(g+, 0) / max(g- + l1 + l2 x, 1e-15)   (g+, g- the likelihood's x-gradient parts, oracle/nmf.py;
        x on the right is the x before the update); the D update, l2_strict and the stop rule as without it
  HALS  the x sweep on C = y D^T - l1 and G = D D^T + l2 I (the exact coordinate minimiser of the penalised
        objective); the D sweep, the normalisation and the x rescale as without it
At l1 = l2 = 0 both are oracle/nmf.py's updates (test_nmf_penalty_host.py pins that)."""
import numpy as np

from oracle import common
from oracle import nmf as onmf


def _f64(*arrays):
    return tuple(None if a is None else np.asarray(a, np.float64) for a in arrays)


def mu_update_x(y, x, d, mask=None, likelihood='l2', l1=0.0, l2=0.0):
    y, x, d, mask = _f64(y, x, d, mask)
    pos, neg = onmf._parts_x(y, x, d, mask, likelihood)
    return x * np.maximum(pos, 0.0) / np.maximum(neg + l1 + l2 * x, common.JITTER)


def mu_step(y, x, d, mask=None, likelihood='l2', l1=0.0, l2=0.0):
    """One penalised MU iteration -> (x_new, D_new normalised, max|D - D_new|)."""
    y, x, d, mask = _f64(y, x, d, mask)
    x = mu_update_x(y, x, d, mask, likelihood, l1, l2)
    d_new = common.l2_strict(onmf.update_d(y, x, d, mask, likelihood))
    return x, d_new, float(np.max(np.abs(d - d_new)))


def mu_iterates(y, d0, x0=None, mask=None, likelihood='l2', l1=0.0, l2=0.0, n=1):
    """The (x, D) after each of n iterations from (x0 or ones, l2_strict(d0)), as nmf.solve(tol=0) runs them."""
    y, d0, x0, mask = _f64(y, d0, x0, mask)
    x = np.ones((y.shape[0], d0.shape[0])) if x0 is None else x0
    d = common.l2_strict(d0)
    out = []
    for _ in range(n):
        x, d, _ = mu_step(y, x, d, mask, likelihood, l1, l2)
        out.append((x, d))
    return out


def sweep(V, C, G):
    """For k = 0 .. K-1 in order, with the current V: where G[k,k] > 0,
    V[:,k] = max(0, V[:,k] - (V G[:,k] - C[:,k]) / G[k,k])."""
    V = np.array(V, np.float64)
    for k in range(G.shape[0]):
        if G[k, k] > 0:
            V[:, k] = np.maximum(0.0, V[:, k] - (V.dot(G[:, k]) - C[:, k]) / G[k, k])
    return V


def hals_x_sweep(y, x, d, l1=0.0, l2=0.0):
    """The penalised x sweep: the sweep on y D^T - l1 and D D^T + l2 I."""
    y, x, d = _f64(y, x, d)
    return sweep(x, y.dot(d.T) - l1, d.dot(d.T) + l2 * np.eye(d.shape[0]))


def hals_step(y, x, d, l1=0.0, l2=0.0):
    """One penalised HALS iteration -> (x_new, D_new, max|D - D_new|)."""
    y, x, d = _f64(y, x, d)
    F = y.shape[1]
    xs = hals_x_sweep(y, x, d, l1, l2)
    stats = np.concatenate([xs.T.dot(y), xs.T.dot(xs)], axis=1)
    Dt = sweep(d.T, stats[:, :F].T, stats[:, F:])
    nrm = np.sqrt(np.sum(Dt * Dt, axis=0))
    pos = nrm > 0
    d_new = Dt.T.copy()
    d_new[pos] /= nrm[pos][:, None]
    xs[:, pos] *= nrm[pos]
    return xs, d_new, float(np.max(np.abs(d - d_new)))


def hals_iterates(y, d0, x0=None, l1=0.0, l2=0.0, n=1):
    y, d0, x0 = _f64(y, d0, x0)
    x = np.ones((y.shape[0], d0.shape[0])) if x0 is None else x0
    d = common.l2_strict(d0)
    out = []
    for _ in range(n):
        x, d, _ = hals_step(y, x, d, l1, l2)
        out.append((x, d))
    return out


def objective(y, x, d, mask=None, likelihood='l2', l1=0.0, l2=0.0):
    """loss + l1 sum(x) + l2/2 |x|^2 ('l2': 1/2 |M o (y - x D)|^2; 'kl': sum M o (y log(y / v) - y + v),
    v = x D + 1e-15)."""
    y, x, d, mask = _f64(y, x, d, mask)
    m = 1.0 if mask is None else mask
    v = x.dot(d)
    if likelihood == 'l2':
        loss = 0.5 * np.sum((m * (y - v)) ** 2)
    else:
        v = v + common.JITTER
        ylog = np.where(y > 0, y * np.log(np.where(y > 0, y, 1.0) / v), 0.0)
        loss = np.sum(m * (ylog - y + v))
    return float(loss + l1 * np.sum(x) + 0.5 * l2 * np.sum(x * x))
