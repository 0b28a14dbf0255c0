"""NumPy restatement of template learning with multichannel templates (decomp_amd.template_matching.solve with
D [T, Ch, S], y [B, Ch, N] and lasso_method 'omp', 'mp' or 'mp_pos') and the planted problems its tests share.  Test
infrastructure only.

The model is that of tm_multichannel_ref: y[b, ch, n] ~ sum_(t, c) x[b, t, c] D[t, ch, n - s c + Q], one coefficient per
event for all channels.  x is shared by the channels, so XXt [T S, T S] is the one-channel statistic of x alone and yX
[T, Ch, S] is, channel by channel, the one-channel yX: ``statistics`` is oracle.template_matching.statistics applied
per channel.  ``d_update`` takes the gradient step channel by channel with the Gershgorin bound of XXt (that of the
block-diagonal operator with Ch copies of XXt) and normalises a template over its Ch S entries.  The coders are
tm_multichannel_ref.omp_gram / mp_gram.  Everything runs in the dtype it is given.
"""
import functools

import numpy as np

import tm_multichannel_ref as mc
from omp_ref import single_exact
from oracle import template_matching as otm
from oracle.common import JITTER, gershgorin, l2, l2_strict
from tm_learn_ref import precision_dtype

# make_problem(seed, B, T, Ch, S, N, stride, padding, nev, cplx), noise 0.05
PLANTED = [
    (200, 32, 2, 3, 9, 130, 1, 'SAME', 4, False),
    (202, 32, 2, 2, 9, 130, 2, 'SAME', 4, False),
    (201, 16, 3, 4, 8, 64, 1, 'VALID', 3, True),
]


def normalize_templates(D, strict=True):
    """l2_strict (or l2) of D [T, Ch, S] over the Ch S entries of a template."""
    f = l2_strict if strict else l2
    return f(D.reshape(D.shape[0], -1)).reshape(D.shape)


def statistics(y, x, S, stride, padding):
    """(XXt [T S, T S], yX [T Ch S]) of y [B, Ch, N], x [B, T, C]."""
    T = x.shape[1]
    per_ch = [otm.statistics(y[:, ch], x, S, stride, padding) for ch in range(y.shape[1])]
    yX = np.stack([p[1].reshape(T, S) for p in per_ch], axis=1)
    return per_ch[0][0], yX.reshape(-1)


def d_update(D, XXt, yX):
    """U[t, ch, k] = D[t, ch, k] + (yX[t, ch, k] - sum XXt[(t, k), (t', k')] D[t', ch, k']) / (Gershgorin(XXt) + 1e-15),
    D_new = l2(U) over the Ch S entries of a template: (D_new, max|D - D_new|)."""
    T, Ch, S = D.shape
    L = gershgorin(XXt) + JITTER
    cols = np.moveaxis(D, 1, -1).reshape(T * S, Ch)                          # [(t, k), ch]
    rhs = np.moveaxis(yX.reshape(D.shape), 1, -1).reshape(T * S, Ch)
    U = cols + (rhs - np.dot(XXt, cols)) / L
    D_new = normalize_templates(np.moveaxis(U.reshape(T, S, Ch), -1, 1), strict=False)
    return D_new, float(np.max(np.abs(D - D_new)))


def code(coder, y, D, N, stride, padding, s, tol=None):
    """x [B, T, C] of the coder ('omp', 'mp', 'mp_pos') with at most s events per signal, in y's dtype."""
    if coder == 'omp':
        return mc.omp_gram(y, D, N, stride, padding, n=s, tol=tol)[0]
    return mc.mp_gram(y, D, N, stride, padding, n=s, tol=tol, positive=(coder == 'mp_pos'))[0]


def solve_batch(y, D, stride, padding, coder, s, coder_tol, tol, maxiter, trace=None):
    """template_matching.solve_batch for y [B, Ch, N], D [T, Ch, S].  Returns (it, D, x)."""
    D = normalize_templates(D)
    S, N = D.shape[-1], y.shape[-1]
    x = None
    for it in range(1, maxiter):
        x = code(coder, y, D, N, stride, padding, s, coder_tol)
        XXt, yX = statistics(y, x, S, stride, padding)
        D_new, diff = d_update(D, XXt, yX)
        if trace is not None:
            trace.append(diff)
        if diff < tol:
            return it, D_new, x
        D = D_new
    return maxiter, D, x


def solve_minibatch(y, D, stride, padding, coder, s, coder_tol, tol, minibatch, size_of_minibatch, maxiter, rng,
                    trace=None):
    """template_matching.solve_minibatch likewise: windows yw [m, Ch, w] coded from zero, written back in draw order,
    XXt_sum += XXt / it, yX_sum += yX / it.  Returns (it, D, the full x)."""
    D = normalize_templates(D)
    T, S = D.shape[0], D.shape[-1]
    B, N = y.shape[0], y.shape[-1]
    w = int(size_of_minibatch)
    cw = otm.coef_size(S, w, stride, padding)
    x = np.zeros((B, T, otm.coef_size(S, N, stride, padding)), dtype=y.dtype)
    yX_sum = np.zeros(D.size, dtype=y.dtype)
    XXt_sum = np.zeros((T * S, T * S), dtype=y.dtype)
    for it in range(1, maxiter):
        rows, starts = otm.minibatch_index((B, N - w), minibatch, rng)
        yw = otm.gather_windows(y, rows, starts, w)
        xw = code(coder, yw, D, w, stride, padding, s, coder_tol)
        otm.scatter_windows(x, rows, starts, cw, xw)
        XXt, yX = statistics(yw, xw, S, stride, padding)
        XXt_sum, yX_sum = otm.accumulate(XXt_sum, yX_sum, XXt, yX, it)
        D_new, diff = d_update(D, XXt_sum, yX_sum)
        if trace is not None:
            trace.append(diff)
        if diff < tol:
            return it, D_new, x
        D = D_new
    return maxiter, D, x


def coded_residual(y, D, stride, padding, s, coder='omp'):
    """The median over the signals of |y - x * D| / |y| (all channels) with x the coder's code of y on D, at most s
    events per signal -- coded and measured in double, whatever dtype D has."""
    wide = np.complex128 if (np.iscomplexobj(y) or np.iscomplexobj(D)) else np.float64
    y, D = np.asarray(y).astype(wide), np.asarray(D).astype(wide)
    N = y.shape[-1]
    x = code(coder, y, D, N, stride, padding, s)
    return float(np.median(mc.residual_norm(x, y, D, N, stride, padding)))


@functools.lru_cache(maxsize=None)
def planted(i):
    """(y [B, Ch, N], D0 [T, Ch, S], (stride, padding), nev) of PLANTED[i] in double with single-exact entries: D0 is
    the normalised truth plus 0.5 randn / sqrt(Ch S).  The arrays are shared: do not write to them."""
    seed, B, T, Ch, S, N, stride, padding, nev, cplx = PLANTED[i]
    y, D, _ = mc.make_problem(seed, B, T, Ch, S, N, stride, padding, nev, cplx)
    rng = np.random.RandomState(seed + 1000)
    e = rng.randn(T, Ch, S)
    if cplx:
        e = e + 1j * rng.randn(T, Ch, S)
    D0 = normalize_templates(D) + 0.5 * e / np.sqrt(Ch * S)
    y, D0 = single_exact(y, D0)
    y.setflags(write=False)
    D0.setflags(write=False)
    return y, D0, (stride, padding), nev


@functools.lru_cache(maxsize=None)
def planted_run(i, precision, iterations=10):
    """(residual at the start, residual after ``iterations`` outer iterations of solve_batch with 'omp' in that
    precision), both coded_residual."""
    y, D0, (stride, padding), nev = planted(i)
    dt = precision_dtype(PLANTED[i][-1], precision)
    start = coded_residual(y, normalize_templates(D0), stride, padding, nev)
    it, D, _ = solve_batch(y.astype(dt), D0.astype(dt), stride, padding, 'omp', nev, None, 0.0, iterations + 1)
    assert it == iterations + 1
    return start, coded_residual(y, D, stride, padding, nev)
