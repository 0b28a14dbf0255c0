"""NumPy reference for approximate K-SVD (decomp_amd.ksvd, decomp_amd/csrc/ksvd.hpp) and the problems the K-SVD
tests share.  Test infrastructure only.  Everything runs in the dtype it is given.

One iteration, for y [N, F], x [N, K], D [K, F] (atoms are rows):
  1. x = omp(y, D, s, coef_tol)                              (omp_ref.omp_lstsq)
  2. R = y - x D
  3. for k = 0 .. K-1, I = {i : x[i, k] != 0} ascending, fixed for the sweep; I empty: atom k is kept; else
     g = x[I, k], d = D[k]:  u = g^H R[I] + |g|^2 d;  d' = u / |u| (d where !(|u| > 0));
     g' = R[I] d'^H + g (d . d'^H);  R[I] += g d - g' d';  x[I, k] = g';  D[k] = d'
  4. max|D_new - D_old| < tol: stop
"""
import functools

import numpy as np

import omp_ref

# (seed, N, F, K, S, cplx)
CASES = {1: (1, 509, 48, 40, 3, False), 2: (2, 509, 24, 70, 3, True), 3: (3, 300, 64, 130, 4, False)}
ITERATIONS = 4      # of the end-to-end comparison


def normalise(D):
    return D / np.sqrt(np.sum(np.abs(D) ** 2, axis=1, keepdims=True))


def sweep(y, x, D):
    """Step 3 on copies: (x, D, R)."""
    x, D = x.copy(), D.copy()
    R = y - x @ D
    supports = [np.flatnonzero(x[:, k] != 0) for k in range(D.shape[0])]
    for k, I in enumerate(supports):
        if I.size == 0:
            continue
        g, d, RI = x[I, k], D[k].copy(), R[I]
        u = g.conj() @ RI + np.sum(np.abs(g) ** 2) * d
        nrm = np.sqrt(np.sum(np.abs(u) ** 2))
        dn = u / nrm if nrm > 0 else d
        gn = RI @ dn.conj() + g * np.sum(d * dn.conj())
        R[I] = RI + np.outer(g, d) - np.outer(gn, dn)
        x[I, k] = gn
        D[k] = dn
    return x, D, R


def objective(y, x, D):
    """|y - x D|^2 / |y|^2 in double."""
    y = np.asarray(y).astype(np.complex128 if np.iscomplexobj(y) else np.float64)
    r = y - np.asarray(x).astype(y.dtype) @ np.asarray(D).astype(y.dtype)
    return float(np.sum(np.abs(r) ** 2) / np.sum(np.abs(y) ** 2))


def solve(y, D, s, tol=1e-3, maxiter=1000, coef_tol=None, log=None):
    """The loop: (it, D, x).  log (a list) receives per iteration (D, x, maxdiff, smallest OMP margin)."""
    D = normalise(D)
    x = np.zeros((y.shape[0], D.shape[0]), dtype=D.dtype)
    for it in range(1, maxiter):
        x, _, margin, _ = omp_ref.omp_lstsq(y, D, s, tol=coef_tol)
        x, D_new, _ = sweep(y, x, D)
        maxdiff = float(np.max(np.abs(D_new - D)))
        D = D_new
        if log is not None:
            log.append((D.copy(), x.copy(), maxdiff, float(margin.min())))
        if maxdiff < tol:
            return it, D, x
    return maxiter, D, x


def make_problem(seed, N, F, K, S, cplx):
    """(y, A, D0) in double with single-exact entries: planted unit-norm A; S non-zeros per row of magnitude 1-2;
    noise 0.02 |y| / sqrt(F); D0 = normalise(A + 0.1 P / sqrt(F)), P Gaussian."""
    rng = np.random.RandomState(seed)

    def randn(*shape):
        return rng.randn(*shape) + 1j * rng.randn(*shape) if cplx else rng.randn(*shape)
    A = normalise(randn(K, F))
    x0 = np.zeros((N, K))
    for i in range(N):
        idx = rng.choice(K, S, replace=False)
        x0[i, idx] = (1 + rng.rand(S)) * rng.choice([-1, 1], S)
    y = x0 @ A
    y = y + 0.02 * np.linalg.norm(y, axis=1, keepdims=True) / np.sqrt(F) * randn(N, F)
    D0 = normalise(A + 0.1 * randn(K, F) / np.sqrt(F))
    y, A = omp_ref.single_exact(y, A)
    _, D0 = omp_ref.single_exact(y, D0)
    return y, A, D0


def random_start(seed, K, F, cplx):
    """A random unit-norm dictionary with single-exact entries."""
    rng = np.random.RandomState(seed)
    D = rng.randn(K, F) + 1j * rng.randn(K, F) if cplx else rng.randn(K, F)
    D = normalise(D)
    return omp_ref.single_exact(D, D)[1]


# ---- computed once per session, never modified ------------------------------------------------------------------
@functools.lru_cache(maxsize=None)
def case_problem(case):
    return make_problem(*CASES[case])


@functools.lru_cache(maxsize=None)
def sweep_inputs(case, start='planted'):
    """(y, x, D) in double, all single-exact: D the perturbed (or a random) start, x = omp_lstsq(y, D, S) rounded
    to single."""
    seed, N, F, K, S, cplx = CASES[case]
    y, _, D0 = case_problem(case)
    D = D0 if start == 'planted' else random_start(100 + seed, K, F, cplx)
    x = omp_ref.omp_lstsq(y, D, S)[0]
    x = x.astype(omp_ref.precision_dtype(cplx, 'single')).astype(x.dtype)
    x.setflags(write=False)
    return y, x, D


@functools.lru_cache(maxsize=None)
def sweep_reference(case, start, precision):
    """sweep() in the precision's dtype on sweep_inputs: (x, D)."""
    cplx = CASES[case][5]
    dt = omp_ref.precision_dtype(cplx, precision)
    y, x, D = sweep_inputs(case, start)
    xs, Ds, _ = sweep(y.astype(dt), x.astype(dt), D.astype(dt))
    return omp_ref._freeze(xs, Ds)


def sweep_bounds(case, start, precision):
    """(D, x, residual) bounds for a GPU sweep in this precision: 4 x what the NumPy sweep in the working dtype shows
    against the double one (the factor covers the other summation order of the chunked reduction), floor 64 eps.
    D relative to 1, x relative to max|x_ref|, the residual as | |y - x D| / |y| - the same of the reference |."""
    cplx = CASES[case][5]
    eps = float(np.finfo(omp_ref.precision_dtype(cplx, precision)).eps)
    y = sweep_inputs(case, start)[0]
    xr, Dr = sweep_reference(case, start, 'double')
    xw, Dw = sweep_reference(case, start, precision)
    floor = 64 * eps
    bd = float(np.max(np.abs(Dw - Dr)))
    bx = float(np.max(np.abs(xw - xr))) / float(np.max(np.abs(xr)))
    br = abs(np.sqrt(objective(y, xw, Dw)) - np.sqrt(objective(y, xr, Dr)))
    return max(4 * bd, floor), max(4 * bx, floor), max(4 * br, floor)


@functools.lru_cache(maxsize=None)
def loop_reference(case, precision):
    """ITERATIONS iterations of solve() from the perturbed start in the precision's dtype: the per-iteration log
    [(D, x, maxdiff, smallest margin)]."""
    seed, N, F, K, S, cplx = CASES[case]
    dt = omp_ref.precision_dtype(cplx, precision)
    y, _, D0 = case_problem(case)
    log = []
    it, _, _ = solve(y.astype(dt), D0.astype(dt), S, tol=0.0, maxiter=ITERATIONS + 1, log=log)
    assert it == ITERATIONS + 1 and len(log) == ITERATIONS
    for D, x, _, _ in log:
        omp_ref._freeze(D, x)
    return tuple(log)


def recovery(A, D):
    """Per planted atom, the largest |<a, d>| over the learned atoms (double)."""
    A = np.asarray(A)
    D = normalise(np.asarray(D).astype(A.dtype))
    return np.max(np.abs(A @ D.conj().T), axis=1)
