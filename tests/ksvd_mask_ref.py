"""NumPy reference for masked approximate K-SVD (decomp_amd.ksvd.solve(mask=...), decomp_amd/csrc/ksvd_mask.hpp) and
the problems its tests share.  Test infrastructure only.  Everything runs in the dtype it is given.

One iteration, for y [N, F], x [N, K], D [K, F] (atoms are rows), weights m [N, F] or [F], real and >= 0, entering
linearly; the objective is sum m |y - x D|^2:
  1. x = masked omp(y, D, s, coef_tol; m)                      (omp_mask_ref.reference)
  2. R = y - x D (hidden entries kept; they enter sums only multiplied by m)
  3. for k = 0 .. K-1, I = {i : x[i, k] != 0} ascending, fixed for the sweep; I empty: atom k is kept; else
     g = x[I, k], d = D[k], m_i = m[i]:
       c_f = sum_I m_if |g_i|^2;  n_f = sum_I m_if conj(g_i) R_if + c_f d_f;  u_f = n_f / c_f (d_f where !(c_f > 0))
       d' = u / |u| (d where !(|u| > 0));  q_i = sum_f m_if |d'_f|^2
       g'_i = (sum_f m_if R_if conj(d'_f) + g_i sum_f m_if d_f conj(d'_f)) / q_i (0 where !(q_i > 0))
       R[I] += g d - g' d';  x[I, k] = g';  D[k] = d'
  4. max|D_new - D_old| < tol: stop
"""
import functools

import numpy as np

import ksvd_ref
import omp_mask_ref
import omp_ref

CASES = ksvd_ref.CASES
ITERATIONS = ksvd_ref.ITERATIONS
KINDS = ('binary', 'weights')
KEEP = 0.7


def _real_dtype(a):
    return np.zeros(1, dtype=a.dtype).real.dtype


def sweep(y, x, D, m):
    """Step 3 on copies: (x, D, R)."""
    x, D = x.copy(), D.copy()
    m = np.broadcast_to(np.asarray(m).astype(_real_dtype(D)), y.shape)
    R = y - x @ D
    supports = [np.flatnonzero(x[:, k] != 0) for k in range(D.shape[0])]
    for k, I in enumerate(supports):
        if I.size == 0:
            continue
        g, d, RI, mI = x[I, k], D[k].copy(), R[I], m[I]
        mR = mI * RI
        c = (np.abs(g) ** 2) @ mI
        n = g.conj() @ mR + c * d
        seen = c > 0
        u = np.where(seen, n / np.where(seen, c, 1), d)
        nrm = np.sqrt(np.sum(np.abs(u) ** 2))
        dn = u / nrm if nrm > 0 else d
        q = mI @ (np.abs(dn) ** 2)
        num = mR @ dn.conj() + g * (mI @ (d * dn.conj()))
        fit = q > 0
        gn = np.where(fit, num / np.where(fit, q, 1), 0).astype(x.dtype)
        R[I] = RI + np.outer(g, d) - np.outer(gn, dn)
        x[I, k] = gn
        D[k] = dn
    return x, D, R


def objective(y, x, D, m):
    """sum m |y - x D|^2 / sum m |y|^2 in double."""
    y = np.asarray(y).astype(np.complex128 if np.iscomplexobj(y) else np.float64)
    m = np.broadcast_to(np.asarray(m, dtype=np.float64), y.shape)
    r = y - np.asarray(x).astype(y.dtype) @ np.asarray(D).astype(y.dtype)
    return float(np.sum(m * np.abs(r) ** 2) / np.sum(m * np.abs(y) ** 2))


def solve(y, D, m, s, tol=1e-3, maxiter=1000, coef_tol=None, log=None):
    """The loop: (it, D, x).  log (a list) receives per iteration (D, x, maxdiff, smallest OMP margin, OMP steps)."""
    D = ksvd_ref.normalise(D)
    x = np.zeros((y.shape[0], D.shape[0]), dtype=D.dtype)
    m2 = np.ascontiguousarray(np.broadcast_to(np.asarray(m).astype(_real_dtype(D)), y.shape))
    for it in range(1, maxiter):
        x, steps, margin, _ = omp_mask_ref.reference(y, D, m2, s, tol=coef_tol)
        x, D_new, _ = sweep(y, x, D, m2)
        maxdiff = float(np.max(np.abs(D_new - D)))
        D = D_new
        if log is not None:
            log.append((D.copy(), x.copy(), maxdiff, float(margin.min()), int(steps.max())))
        if maxdiff < tol:
            return it, D, x
    return maxiter, D, x


# ---- computed once per session, never modified ------------------------------------------------------------------
@functools.lru_cache(maxsize=None)
def case_masks(case):
    """(binary, weights) [N, F] in double, single-exact: one generator, keep first, then the weights; 30 % missing."""
    seed, N, F = CASES[case][:3]
    rng = np.random.RandomState(2000 + seed)
    keep = rng.rand(N, F) < KEEP
    binary = keep.astype(np.float64)
    weights = np.where(keep, 0.25 + 0.75 * rng.rand(N, F), 0).astype(np.float32).astype(np.float64)
    return omp_ref._freeze(binary, weights)


def case_mask(case, kind):
    return case_masks(case)[KINDS.index(kind)]


@functools.lru_cache(maxsize=None)
def sweep_inputs(case, kind, start='planted'):
    """(y, x, D, m) in double, all single-exact: D the perturbed (or a random) start, x the masked coder's codes
    for it, rounded to single."""
    seed, N, F, K, S, cplx = CASES[case]
    y, _, D0 = ksvd_ref.case_problem(case)
    m = case_mask(case, kind)
    D = D0 if start == 'planted' else ksvd_ref.random_start(100 + seed, K, F, cplx)
    x = omp_mask_ref.reference(y, D, m, S)[0]
    x = x.astype(omp_ref.precision_dtype(cplx, 'single')).astype(x.dtype)
    x.setflags(write=False)
    return y, x, D, m


@functools.lru_cache(maxsize=None)
def sweep_reference(case, kind, start, precision):
    """sweep() in the precision's dtype on sweep_inputs: (x, D)."""
    cplx = CASES[case][5]
    dt = omp_ref.precision_dtype(cplx, precision)
    y, x, D, m = sweep_inputs(case, kind, start)
    xs, Ds, _ = sweep(y.astype(dt), x.astype(dt), D.astype(dt), m)
    return omp_ref._freeze(xs, Ds)


def rel_resid(y, x, D, m):
    return float(np.sqrt(objective(y, x, D, m)))


def bounds_against(y, m, xr, Dr, xw, Dw, eps):
    """(D, x, residual) bounds: 4 x what a NumPy sweep in the working dtype (xw, Dw) shows against the double one
    (xr, Dr) -- the factor covers the other summation order of the chunked reduction -- floor 64 eps.  D relative to
    1, x relative to max|x_ref|, the residual as the difference of the weighted relative residuals."""
    floor = 64 * eps
    xmax = max(float(np.max(np.abs(xr))), 1e-300)
    bd = float(np.max(np.abs(Dw - Dr)))
    bx = float(np.max(np.abs(xw - xr))) / xmax
    br = abs(rel_resid(y, xw, Dw, m) - rel_resid(y, xr, Dr, m))
    return max(4 * bd, floor), max(4 * bx, floor), max(4 * br, floor)


def sweep_bounds(case, kind, start, precision):
    """bounds_against for a GPU sweep of sweep_inputs in this precision."""
    cplx = CASES[case][5]
    eps = float(np.finfo(omp_ref.precision_dtype(cplx, precision)).eps)
    y, _, _, m = sweep_inputs(case, kind, start)
    xr, Dr = sweep_reference(case, kind, start, 'double')
    xw, Dw = sweep_reference(case, kind, start, precision)
    return bounds_against(y, m, xr, Dr, xw, Dw, eps)


@functools.lru_cache(maxsize=None)
def loop_reference(case, kind, precision):
    """ITERATIONS iterations of solve() from the perturbed start in the precision's dtype: the per-iteration log
    [(D, x, maxdiff, smallest margin, OMP steps)]."""
    seed, N, F, K, S, cplx = CASES[case]
    dt = omp_ref.precision_dtype(cplx, precision)
    y, _, D0 = ksvd_ref.case_problem(case)
    m = case_mask(case, kind)
    log = []
    it, _, _ = solve(y.astype(dt), D0.astype(dt), m, S, tol=0.0, maxiter=ITERATIONS + 1, log=log)
    assert it == ITERATIONS + 1 and len(log) == ITERATIONS
    for entry in log:
        omp_ref._freeze(entry[0], entry[1])
    return tuple(log)

