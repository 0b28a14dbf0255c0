"""Float64 NumPy restatement of em-hals, HALS NMF for data with missing or weighted entries (test infrastructure
only).

The objective is  1/2 sum w o (y - x D)^2 + l1 sum(x) + l2/2 |x|^2  with weights w in [0, 1] and D's rows at unit
norm.  One iteration from (x, D):
  y' = w o y + (1 - w) o (x D)                       the unobserved part filled in from the current model
  (x, D) <- one HALS iteration on y'                 penalty_ref.hals_step: x sweep, D sweep, normalise, rescale
1/2 |y' - x D|^2 = 1/2 sum w (y - xD)^2 + 1/2 sum (1 - w)(x0 D0 - xD)^2 + const >= the masked loss, with equality
at (x0, D0); HALS does not increase the left side, so no iteration increases the masked objective.  At w = 1 the
imputation returns y itself, and the iteration is penalty_ref.hals_step bit for bit."""
import numpy as np

from oracle import common

from penalty_ref import _f64, hals_step


def impute_np(y, w, x, d):
    """w y + (1 - w)(x D), formed as the kernel forms it (the product with (1 - w) first, then w y added)."""
    y, w, x, d = _f64(y, w, x, d)
    return w * y + (1.0 - w) * x.dot(d)


def emhals_step_np(y, w, x, d, l1=0.0, l2=0.0):
    """One em-hals iteration -> (x_new, D_new, max|D - D_new|).  w None: one HALS iteration."""
    y, w, x, d = _f64(y, w, x, d)
    return hals_step(y if w is None else impute_np(y, w, x, d), x, d, l1, l2)


def emhals_solve_np(y, d0, w=None, x0=None, tol=1e-3, maxiter=1000, l1=0.0, l2=0.0, trace=None, objs=None):
    """nmf.solve(method='em-hals') restated: x = ones by default, D l2_strict normalised, then the MU loop's stop
    rule (it = 1 .. maxiter-1; (it, D_new, x) at the first max|D - D_new| < tol, else (maxiter, D, x)).
    trace collects |(y - x D_new) o w|_F, objs the penalised masked objective, after every iteration."""
    y, d0, w, x0 = _f64(y, d0, w, x0)
    x = np.ones((y.shape[0], d0.shape[0])) if x0 is None else x0
    d = common.l2_strict(d0)
    for it in range(1, maxiter):
        x, d_new, diff = emhals_step_np(y, w, x, d, l1, l2)
        if trace is not None:
            trace.append(float(np.linalg.norm((y - x.dot(d_new)) * (1.0 if w is None else w))))
        if objs is not None:
            objs.append(masked_objective(y, w, x, d_new, l1, l2))
        if diff < tol:
            return it, d_new, x
        d = d_new
    return maxiter, d, x


def masked_mu_np(y, d0, w, x0=None, maxiter=2):
    """The masked multiplicative update (method='mu', l2, mask w), maxiter-1 iterations -> (D, x):
    x <- x o ((w o y) D^T)+ / max(((xD) o w) D^T, 1e-15), the same for D with the new x, then unit-norm rows."""
    y, d0, w, x0 = _f64(y, d0, w, x0)
    x = np.ones((y.shape[0], d0.shape[0])) if x0 is None else x0
    d = common.l2_strict(d0)
    ym = y * w
    for _ in range(1, maxiter):
        x = x * np.maximum(ym.dot(d.T), 0.0) / np.maximum((x.dot(d) * w).dot(d.T), common.JITTER)
        u = d * np.maximum(x.T.dot(ym), 0.0) / np.maximum(x.T.dot(x.dot(d) * w), common.JITTER)
        d = common.l2_strict(u)
    return d, x


def masked_objective(y, w, x, d, l1=0.0, l2=0.0):
    """1/2 sum w o (y - x D)^2 + l1 sum(x) + l2/2 |x|^2  (w None: w = 1)."""
    y, w, x, d = _f64(y, w, x, d)
    r = y - x.dot(d)
    loss = 0.5 * np.sum((1.0 if w is None else w) * r * r)
    return float(loss + l1 * np.sum(x) + 0.5 * l2 * np.sum(x * x))


def masked_rel_resid(y, w, x, d):
    """|(y - x D) o w|_F / |y o w|_F."""
    y, w, x, d = _f64(y, w, x, d)
    return float(np.linalg.norm((y - x.dot(d)) * w) / np.linalg.norm(y * w))


def hidden_rel_err(y, w, x, d):
    """|(y - x D) o (w == 0)|_F / |y o (w == 0)|_F: how well the entries the solver never saw are recovered."""
    y, w, x, d = _f64(y, w, x, d)
    h = (w == 0).astype(np.float64)
    return float(np.linalg.norm((y - x.dot(d)) * h) / np.linalg.norm(y * h))


def planted(N=300, F=129, K=12, seed=0):
    """The planted non-negative problem of the HALS tests (exactly rank K): (y, D start)."""
    rng = np.random.RandomState(seed)
    x0 = rng.uniform(size=(N, K)) * (rng.uniform(size=(N, K)) < 0.5)
    d0 = rng.uniform(size=(K, F)) * (rng.uniform(size=(K, F)) < 0.5)
    return x0.dot(d0), rng.uniform(size=(K, F)) + 0.1


def binary_mask(shape, missing, seed, dtype=np.float64):
    return (np.random.RandomState(seed).uniform(size=shape) >= missing).astype(dtype)


def weights(shape, lo, seed, dtype=np.float64):
    return np.random.RandomState(seed).uniform(lo, 1.0, size=shape).astype(dtype)
