"""CPU oracle: 1-D convolutional template learning (test infrastructure only).

Restates, in NumPy, the reference's
  decomp/template_matching.py:104-113   _coef_size
  decomp/template_matching.py:116-130   _temp2mat  (the dense operator A [T, C, N])
  decomp/template_matching.py:133-172   _coef2mat  (the dense X [B, T, S, N])
  decomp/template_matching.py:175-179   predict
  decomp/template_matching.py:182-229   solve_batch
  decomp/template_matching.py:232-268   Minibatcher (stack, sequential write-back)
  decomp/template_matching.py:271-337   solve_minibatch
  decomp/utils/data.py:12-16            minibatch_index
The im2col matrices are written in closed form: with pad = N - 1 (SAME) or N - S (VALID),
C = floor((S + 2 pad - N) / s) + 1 and Q = s (C - 1) - pad,
  A[(t, c), n] = D[t, n - s c + Q]   and   X[b, (t, k), n] = x[b, t, c] where n = s c - Q + k,
both zero where the tap falls outside [0, N).  The LASSO step is oracle.lasso.solve_fastpath on A.
Everything runs in the dtype it is given, so the same code serves as the float64 reference and,
on single-precision inputs, as a measure of the single-precision rounding floor.
"""
import numpy as np

from .common import JITTER, gershgorin, l2, l2_strict
from . import lasso


# ----------------------------------------------------------------- geometry ----
def coef_size(S, N, stride=1, padding='VALID'):
    """template_matching.py:104-113"""
    pad = N - S if padding == 'VALID' else N - 1
    return int(np.floor((S + 2 * pad - N) / stride + 1))


def geometry(S, N, stride, padding):
    """(C, Q): the coefficients per template and the offset of A[(t, c), n] = D[t, n - s c + Q]."""
    pad = N - S if padding == 'VALID' else N - 1
    C = coef_size(S, N, stride, padding)
    return C, stride * (C - 1) - pad


def _taps(S, N, stride, padding):
    """(c, k, n) of every tap inside the signal: n = s c - Q + k in [0, N)."""
    C, Q = geometry(S, N, stride, padding)
    n = stride * np.arange(C)[:, None] - Q + np.arange(S)[None, :]
    c, k = np.nonzero((n >= 0) & (n < N))
    return c, k, n[c, k]


def temp2mat(D, N, stride, padding):
    """template_matching.py:116-130 : A [T, C, N]."""
    T, S = D.shape
    C, _ = geometry(S, N, stride, padding)
    A = np.zeros((T, C, N), D.dtype)
    c, k, n = _taps(S, N, stride, padding)
    A[:, c, n] = D[:, k]
    return A


def coef2mat(x, N, S, stride, padding):
    """template_matching.py:133-172 : X [B, T, S, N] for x [B, T, C] ([T, S, N] for x [T, C])."""
    x3 = x[None] if x.ndim == 2 else x
    B, T, C = x3.shape
    if C != coef_size(S, N, stride, padding):
        raise ValueError('x has %d coefficients, the geometry needs %d' % (C, coef_size(S, N, stride, padding)))
    X = np.zeros((B, T, S, N), x.dtype)
    c, k, n = _taps(S, N, stride, padding)
    X[:, :, k, n] = x3[:, :, c]
    return X[0] if x.ndim == 2 else X


def predict(x, D, N, stride=1, padding='SAME'):
    """template_matching.py:175-179 : tensordot(x, A, 2)."""
    return np.tensordot(x, temp2mat(D, N, stride, padding), 2)


# -------------------------------------------------------------- LASSO step ----
def lasso_step(y, D, x, alpha, stride, padding, method, maxiter, tol, trace=None):
    """template_matching.py:201-206 : lasso.solve_fastpath on A.reshape(T C, N); y [B, N], x [B, T, C].
    Returns (it, x_new [B, T, C])."""
    B, N = y.shape
    A = temp2mat(D, N, stride, padding).reshape(-1, N)
    it, xf = lasso.solve_fastpath(y, A, alpha, x.reshape(B, -1), tol, maxiter, method, trace=trace)
    return it, xf.reshape(x.shape)


# ----------------------------------------------------------------- D step ----
def statistics(y, x, S, stride, padding):
    """template_matching.py:208-215 : XXt [T S, T S] and yX [T S] of y [B, N], x [B, T, C]."""
    B, N = y.shape
    X = coef2mat(x, N, S, stride, padding).reshape(B, -1, N)
    Xt = np.moveaxis(X, -2, -1)
    if X.dtype.kind == 'c':
        Xt = np.conj(Xt)
    XXt = np.tensordot(X, Xt, ((0, -1), (0, -2)))
    yX = np.tensordot(y, X, ((0, -1), (0, -1)))
    return XXt, yX


def accumulate(XXt_sum, yX_sum, XXt, yX, it):
    """template_matching.py:322-323 : the running sums XXt_sum + XXt / it, yX_sum + yX / it."""
    return XXt_sum + XXt / it, yX_sum + yX / it


def d_update(D, XXt, yX):
    """template_matching.py:217-223 : D_new = l2(D + (yX - XXt D) / (Gershgorin(XXt) + 1e-15)) and
    max|D - D_new|."""
    L = gershgorin(XXt) + JITTER
    D_flat = D.flatten()
    D_new = l2(np.reshape(D_flat + (yX - np.dot(XXt, D_flat)) / L, D.shape))
    return D_new, float(np.max(np.abs(D - D_new)))


# ------------------------------------------------------------------ loops ----
def minibatch_index(shape, minibatch, rng):
    """data.py:12-16"""
    if minibatch is None and len(shape) == 1:
        return tuple([slice(None, None, None) for _ in shape])
    return tuple([rng.randint(0, s, minibatch) for s in shape])


def gather_windows(a, rows, starts, w):
    """template_matching.py:243-252 : stack a[row, ..., start:start + w] over the draws."""
    return np.stack([a[r, ..., s:s + w] for r, s in zip(rows, starts)], axis=0)


def scatter_windows(a, rows, starts, w, values):
    """template_matching.py:254-260 : write the windows back one after the other (the last one wins);
    ``a`` is modified in place."""
    for r, s, v in zip(rows, starts, values):
        a[r, ..., s:s + w] = v
    return a


def solve_batch(y, D, alpha, x, stride, padding, tol, maxiter, lasso_method, lasso_iter, lasso_tol,
                trace=None):
    """template_matching.py:182-229; y [B, N], x [B, T, C].  ``trace`` (a list) receives max|D - D_new|
    of every outer iteration, the stopping one included."""
    D = l2_strict(D)
    S = D.shape[1]
    for it in range(1, maxiter):
        _, x = lasso_step(y, D, x, alpha, stride, padding, lasso_method, lasso_iter, lasso_tol)
        XXt, yX = statistics(y, x, S, stride, padding)
        D_new, diff = d_update(D, XXt, yX)
        if trace is not None:
            trace.append(diff)
        if diff < tol:
            return it, D_new, x
        D = D_new
    return maxiter, D, x


def solve_minibatch(y, D, alpha, x, stride, padding, tol, minibatch, size_of_minibatch, maxiter,
                    lasso_method, lasso_iter, lasso_tol, rng, trace=None):
    """template_matching.py:271-337; y [B, N], x [B, T, C] (a copy is updated and returned); ``trace`` as
    in solve_batch."""
    D = l2_strict(D)
    S = D.shape[1]
    w = int(size_of_minibatch)
    cw = coef_size(S, w, stride, padding)
    x = x.copy()
    yX_sum = np.zeros(D.size, dtype=y.dtype)
    XXt_sum = np.zeros((D.size, D.size), dtype=y.dtype)
    for it in range(1, maxiter):
        rows, starts = minibatch_index((y.shape[0], y.shape[-1] - w), minibatch, rng)
        yw = gather_windows(y, rows, starts, w)
        xw = gather_windows(x, rows, starts, cw)
        _, xw = lasso_step(yw, D, xw, alpha, stride, padding, lasso_method, lasso_iter, lasso_tol)
        scatter_windows(x, rows, starts, cw, xw)
        XXt, yX = statistics(yw, xw, S, stride, padding)
        XXt_sum, yX_sum = accumulate(XXt_sum, yX_sum, XXt, yX, it)
        D_new, diff = d_update(D, XXt_sum, yX_sum)
        if trace is not None:
            trace.append(diff)
        if diff < tol:
            return it, D_new, x
        D = D_new
    return maxiter, D, x


def solve(y, D, alpha, stride=1, padding='SAME', x=None, tol=1.0e-4, minibatch=None,
          size_of_minibatch=None, maxiter=1000, lasso_method='acc_ista', lasso_iter=10,
          lasso_tol=1.0e-5, random_seed=None, trace=None):
    """template_matching.py:12-101 without the validation: x defaults to zeros; y [N] or [B, N]."""
    rng = np.random.RandomState(random_seed)
    S, N = D.shape[-1], y.shape[-1]
    if x is None:
        x = np.zeros(y.shape[:-1] + (D.shape[0], coef_size(S, N, stride, padding)), dtype=y.dtype)
    one_d = y.ndim == 1
    y2, x2 = (y[None], x[None]) if one_d else (y, x)
    if minibatch is None:
        it, D, x2 = solve_batch(y2, D, alpha, x2, stride, padding, tol, maxiter,
                                lasso_method, lasso_iter, lasso_tol, trace)
    else:
        it, D, x2 = solve_minibatch(y2, D, alpha, x2, stride, padding, tol, minibatch, size_of_minibatch,
                                    maxiter, lasso_method, lasso_iter, lasso_tol, rng, trace)
    return it, D, (x2[0] if one_d else x2)
