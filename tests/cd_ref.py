"""NumPy restatement of solve_fastpath + coordinate descent, cheap enough for wide dictionaries (test infrastructure only).

oracle/lasso.py's `_cd` recomputes x.A for every coordinate (N K^2 F per sweep).  `solve` below is the same
iteration in Gram form, derived from oracle/lasso.py:237-276 and :123-146:
  row-normalise A, fold a 1-D mask into y and A, scale alpha, tol and x        (oracle/lasso.py:247-261)
  g = y An^H - x (An An^H)
  for k = 0 .. K-1 in order:  z = g_k + x_k G_kk ;  x_k <- S(z, alpha_k) ;  g -= dx G[k, :]
  the stop test max_k(|dx_k| - tol_k) < 0 is collected over all coordinates on sweeps 0, 10, 20, ...
at N K^2 per sweep.  Rows are independent, so every coordinate step is taken for all rows at once.  A zero
step leaves g untouched.  `solve_masked` is the 2-D-mask iteration (oracle/lasso.py:129-139) with the residual
r = (y - x.A) o M kept up to date instead of recomputed, QUIRK included: the x_k A_k term is unmasked, so
z = r . conj(A_k) + x_k (A_k . conj(A_k)).

`dtype=` (float32 / complex64) runs everything from the normalisation on in that precision; without it the
run is float64 / complex128.  test_cd_ref_host.py pins both functions to oracle.lasso.solve."""
import numpy as np

from oracle import lasso as olasso
from oracle.common import real_dtype


class Result(object):
    """it, x: what lasso.solve returns.  moved[i]: share of the (row, coordinate) pairs whose step in sweep i
    was non-zero.  stop[j]: max_k(|dx_k| - tol_k) of the j-th check sweep (sweep 10 j), in the scaled
    variables the test is made in.  s: the row norms of A (x_scaled = x * s).  after[i]: the codes after
    sweep i, for the sweeps listed in `keep`."""

    def __init__(self):
        self.it, self.x, self.s = None, None, None
        self.moved, self.stop, self.after = [], [], {}


def err(x, x_ref):
    """max|x - x_ref| / max(1, max|x_ref|): the measure every oracle comparison of the LASSO tests uses."""
    x_ref = np.asarray(x_ref)
    return float(np.max(np.abs(np.asarray(x) - x_ref))) / max(1.0, float(np.max(np.abs(x_ref))))


def _working(dtype, like):
    if dtype is not None:
        return np.dtype(dtype)
    return np.dtype(np.complex128 if np.dtype(like).kind == 'c' else np.float64)


def _prepare(y, A, alpha, x, tol, mask, dtype):
    """oracle/lasso.py:247-265 in the working precision -> y, An, alpha, tol_k, x_scaled, s, mask2d."""
    wdt = _working(dtype, y.dtype)
    rdt = real_dtype(wdt)
    y, A = np.asarray(y).astype(wdt), np.asarray(A).astype(wdt)
    K = A.shape[0]
    x = np.zeros(y.shape[:-1] + (K,), wdt) if x is None else np.asarray(x).astype(wdt)
    if mask is not None:
        mask = np.asarray(mask).astype(rdt)
        if mask.ndim == 1:
            y, A = y * mask, A * mask
    s = np.sqrt(np.sum(np.real(np.conj(A) * A), axis=-1)).astype(rdt)
    A = A / s[:, None]
    alpha = rdt.type(alpha) / s
    tol = rdt.type(tol) * s
    x = x * s
    if mask is None:
        alpha = alpha * rdt.type(A.shape[-1])
    else:
        alpha = alpha * np.sum(mask, axis=-1, keepdims=mask.ndim == 2)   # [K] or [N, K]
        if mask.ndim == 1:
            mask = None
    return y, A, alpha, tol, x, s, mask


def _run(x, alpha, tol, maxiter, shrink, gkk, target, apply_step, keep):
    """The sweep loop shared by the two forms: target(k) is what the step adds to x_k G_kk, apply_step(k, rows, dx)
    carries the non-zero steps (of the rows named) into it."""
    res = Result()
    K = x.shape[-1]
    res.it = maxiter - 1
    for i in range(maxiter):
        worst, moved = -np.inf, 0
        for k in range(K):
            z = target(k) + x[:, k] * gkk[k]
            xn = shrink(z, alpha[..., k])
            dx = xn - x[:, k]
            if i % 10 == 0:
                worst = max(worst, float(np.max(np.abs(dx) - tol[k])))
            x[:, k] = xn
            rows = np.flatnonzero(dx)
            if rows.size:
                moved += rows.size
                apply_step(k, rows, dx[rows])
        res.moved.append(moved / float(x.size))
        if i in keep:
            res.after[i] = x.copy()
        if i % 10 == 0:
            res.stop.append(worst)
            if worst < 0.0:
                res.it = i
                break
    return res


def _finish(res, x, s, shape):
    res.s = s
    res.x = (x / s).reshape(shape)
    res.after = dict((i, (v / s).reshape(shape)) for i, v in res.after.items())
    return res


def solve(y, A, alpha, x=None, tol=1.0e-3, method='cd', maxiter=1000, mask=None, dtype=None, keep=()):
    """lasso.solve(method='cd' | 'cd_pos') without a mask or with a 1-D mask, in Gram form."""
    assert method in ('cd', 'cd_pos') and (mask is None or np.ndim(mask) == 1)
    positive = method == 'cd_pos'
    y, A, alpha, tol, x, s, _ = _prepare(y, A, alpha, x, tol, mask, dtype)
    shape = x.shape
    y, x = y.reshape(-1, y.shape[-1]), x.reshape(-1, x.shape[-1]).copy()
    shrink = olasso._pick_shrink(A, positive)
    At = olasso._adjoint(A, positive)
    G = A.dot(At)
    g = y.dot(At) - x.dot(G)

    def apply_step(k, rows, dx):
        g[rows] = g[rows] - dx[:, None] * G[k]
    res = _run(x, alpha, tol, maxiter, shrink, np.diagonal(G), lambda k: g[:, k], apply_step, keep)
    return _finish(res, x, s, shape)


def solve_masked(y, A, alpha, mask, x=None, tol=1.0e-3, method='cd', maxiter=1000, dtype=None, keep=()):
    """lasso.solve(method='cd' | 'cd_pos', mask=<y's shape>), in residual form."""
    assert method in ('cd', 'cd_pos') and np.ndim(mask) == np.ndim(y)
    positive = method == 'cd_pos'
    y, A, alpha, tol, x, s, mask = _prepare(y, A, alpha, x, tol, mask, dtype)
    shape = x.shape
    F = y.shape[-1]
    y, mask, x = y.reshape(-1, F), mask.reshape(-1, F), x.reshape(-1, x.shape[-1]).copy()
    alpha = alpha.reshape(-1, alpha.shape[-1])
    shrink = olasso._pick_shrink(A, positive)
    At = olasso._adjoint(A, positive)
    r = (y - x.dot(A)) * mask
    gkk = np.sum(A * At.T, axis=-1)          # A_k . conj(A_k), as the reference evaluates it

    def apply_step(k, rows, dx):
        r[rows] = r[rows] - dx[:, None] * (A[k] * mask[rows])
    res = _run(x, alpha, tol, maxiter, shrink, gkk, lambda k: r.dot(At[:, k]), apply_step, keep)
    return _finish(res, x, s, shape)
