"""NumPy restatement of template learning with a greedy coder (decomp_amd.template_matching.solve with
lasso_method 'omp', 'mp' or 'mp_pos') and the planted problems its tests share.  Test infrastructure only.

The reference project has no greedy template learner; the loops below are the composition of pieces that are each
checked on their own: the coders tm_omp_ref.omp_gram / tm_pursuit_ref.mp_gram, and oracle.template_matching's
statistics, accumulate and d_update.  Everything runs in the dtype it is given, so the same code is the double
reference and, on single-precision inputs, the measure of what single precision does to a trajectory.
"""
import functools

import numpy as np

import tm_omp_ref
import tm_pursuit_ref as mp
from omp_ref import single_exact
from oracle import template_matching as otm
from oracle.common import l2_strict

# make_problem(seed, B, T, S, N, stride, padding, nev, cplx), noise 0.05
PLANTED = [
    (100, 32, 2, 9, 130, 1, 'SAME', 4, False),
    (102, 32, 2, 9, 130, 2, 'SAME', 4, False),
    (101, 16, 3, 8, 64, 1, 'VALID', 3, True),
]


def code(coder, y, D, N, stride, padding, s, tol=None):
    """x [B, T, C] of the coder ('omp', 'mp', 'mp_pos') with at most s events per signal, in y's dtype."""
    if coder == 'omp':
        return tm_omp_ref.omp_gram(y, D, N, stride, padding, n=s, tol=tol)[0]
    return mp.mp_gram(y, D, N, stride, padding, n=s, tol=tol, positive=(coder == 'mp_pos'))[0]


def solve_batch(y, D, stride, padding, coder, s, coder_tol, tol, maxiter, trace=None):
    """template_matching.solve_batch with the coder in place of the LASSO step; y [B, N].  ``trace`` (a list) receives
    max|D - D_new| of every outer iteration.  Returns (it, D, x)."""
    D = l2_strict(D)
    S, N = D.shape[1], y.shape[1]
    x = None
    for it in range(1, maxiter):
        x = code(coder, y, D, N, stride, padding, s, coder_tol)
        XXt, yX = otm.statistics(y, x, S, stride, padding)
        D_new, diff = otm.d_update(D, XXt, yX)
        if trace is not None:
            trace.append(diff)
        if diff < tol:
            return it, D_new, x
        D = D_new
    return maxiter, D, x


def solve_minibatch(y, D, stride, padding, coder, s, coder_tol, tol, minibatch, size_of_minibatch, maxiter, rng,
                    trace=None):
    """template_matching.solve_minibatch likewise: every window is coded from zero, written back in draw order, and the
    statistics enter the running sums XXt_sum += XXt / it, yX_sum += yX / it.  Returns (it, D, the full x)."""
    D = l2_strict(D)
    T, S = D.shape
    w = int(size_of_minibatch)
    cw = otm.coef_size(S, w, stride, padding)
    x = np.zeros((y.shape[0], T, otm.coef_size(S, y.shape[1], stride, padding)), dtype=y.dtype)
    yX_sum = np.zeros(D.size, dtype=y.dtype)
    XXt_sum = np.zeros((D.size, D.size), dtype=y.dtype)
    for it in range(1, maxiter):
        rows, starts = otm.minibatch_index((y.shape[0], y.shape[1] - w), minibatch, rng)
        yw = otm.gather_windows(y, rows, starts, w)
        xw = code(coder, yw, D, w, stride, padding, s, coder_tol)
        otm.scatter_windows(x, rows, starts, cw, xw)
        XXt, yX = otm.statistics(yw, xw, S, stride, padding)
        XXt_sum, yX_sum = otm.accumulate(XXt_sum, yX_sum, XXt, yX, it)
        D_new, diff = otm.d_update(D, XXt_sum, yX_sum)
        if trace is not None:
            trace.append(diff)
        if diff < tol:
            return it, D_new, x
        D = D_new
    return maxiter, D, x


def coded_residual(y, D, stride, padding, s, coder='omp'):
    """How well templates D explain y: the median over the signals of |y - x * D| / |y| with x the coder's code of y
    on D, at most s events per signal -- coded and measured in double, whatever dtype D has."""
    wide = np.complex128 if (np.iscomplexobj(y) or np.iscomplexobj(D)) else np.float64
    y, D = np.asarray(y).astype(wide), np.asarray(D).astype(wide)
    N = y.shape[1]
    x = code(coder, y, D, N, stride, padding, s)
    return float(np.median(mp.residual_norm(x, y, D, N, stride, padding)))


@functools.lru_cache(maxsize=None)
def planted(i):
    """(y, D0, (stride, padding), nev) of PLANTED[i] in double with single-exact entries: D0 is the normalised truth
    plus 0.5 randn / sqrt(S).  The arrays are shared: do not write to them."""
    seed, B, T, S, N, stride, padding, nev, cplx = PLANTED[i]
    y, D, _ = mp.make_problem(seed, B, T, S, N, stride, padding, nev, cplx)
    rng = np.random.RandomState(seed + 1000)
    e = rng.randn(T, S)
    if cplx:
        e = e + 1j * rng.randn(T, S)
    D0 = l2_strict(D) + 0.5 * e / np.sqrt(S)
    y, D0 = single_exact(y, D0)
    y.setflags(write=False)
    D0.setflags(write=False)
    return y, D0, (stride, padding), nev


def precision_dtype(cplx, precision):
    return np.dtype({('single', False): np.float32, ('single', True): np.complex64,
                     ('double', False): np.float64, ('double', True): np.complex128}[(precision, cplx)])


@functools.lru_cache(maxsize=None)
def planted_run(i, precision, iterations=10):
    """(residual at the start, residual after ``iterations`` outer iterations of solve_batch with 'omp' in that
    precision), both coded_residual."""
    y, D0, (stride, padding), nev = planted(i)
    dt = precision_dtype(PLANTED[i][-1], precision)
    start = coded_residual(y, l2_strict(D0), stride, padding, nev)
    it, D, _ = solve_batch(y.astype(dt), D0.astype(dt), stride, padding, 'omp', nev, None, 0.0, iterations + 1)
    assert it == iterations + 1
    return start, coded_residual(y, D, stride, padding, nev)
