"""NumPy restatement of solve_fastpath for parallel_cd and admm (test infrastructure only).

`solve` is oracle/lasso.py:150-233 and :237-276 once more (row-normalise A, fold a 1-D mask into y and A, scale alpha,
tol and x; the shotgun coordinate descent with the RandomState(0) stream of cumulative shuffles of one 0/1 vector;
ADMM with one inverse, or with one K x K inverse per row under a 2-D mask), for both methods, +- '_pos', mask none,
1-D or 2-D, an initial x and ADMM's rho.  It works in double / complex double whatever the dtype of its inputs and
records what the oracle does not hand out:
  ratio, p    K / Gershgorin(An An^H) and its integer part, the coordinates parallel_cd commits per iteration
  stats[j]    the stop statistic m of check iteration 10 j: max |dx_k| / tol_k for parallel_cd, the larger of
              max |x - x_new| / tol_k and max |z - x_new| / tol_k for ADMM.  The test is met when m < 1.
  full, before, after   parallel_cd at a met test: the full update (what the call returns), the committed iterate the
              iteration started from and the one it would have left behind
test_lasso_extra_ref_host.py pins `solve` to oracle.lasso (same `it`, x within 1e-12) and checks, for every case of
test_gpu_lasso_extra_shapes.py, the conditions that file relies on.

Two variants measure what single precision costs, without a kernel:
  round_iterates=True   double arithmetic, the iterates rounded to single after every iteration (the stop tests must
                        not depend on it)
  dtype='float32' | 'complex64'   ADMM as the library runs a single-precision problem: An, y An^H, the Gram matrix and
                        every iterate in single, the inverse worked in double from the single Gram matrix and stored in
                        single (2-D mask: the per-row systems are formed and kept in double, the product rounded)

`SHAPES`, `problem` and the tables below are the cases of the GPU file; every seed and tolerance in them was
chosen by the rule written next to it and is re-checked by the host test."""
import numpy as np

import cd_ref
from oracle import lasso as olasso
from oracle.common import gershgorin, real_dtype

# (N, F, K): the smallest shapes at which each path of the two solvers is live (test_gpu_lasso_extra_shapes.py)
SHAPES = {
    'tall': (160, 40, 20),
    'k33': (200, 70, 33),
    'k130': (150, 150, 130),
    'k260': (130, 600, 260),
    'over': (40, 48, 260),
}
DTYPES = ('float32', 'float64', 'complex64', 'complex128')
ALPHA = {'parallel_cd': 0.2, 'admm': 0.05}
MASKED_ADMM_ROWS = 16        # k260 (and k130 under rho): N K^2 work elements per call

# problem(name, cplx) seeds: the first seed >= 0 for which, without a mask and with the 1-D mask, in double and in
# single arithmetic, 1 < p < K and the fractional part of K / bound lies in [0.1, 0.9]
SEEDS = {
    ('tall', False): 0, ('tall', True): 0,
    ('k33', False): 0, ('k33', True): 0,
    ('k130', False): 0, ('k130', True): 1,
    ('k260', False): 0, ('k260', True): 0,
    ('over', False): 0, ('over', True): 2,
}

# stop tests: tol per (shape, complex, method, 2-D mask).  Rule: run the float64 / complex128 problem from x = None
# without a stop and take M_j = m_j * tol of check j (the largest step, in units of x).  parallel_cd (300 iterations):
# the last check j >= 1 with M_j >= 0.03, M_i >= 1.4 M_j for all i < j, and the full update of iteration 10 j more
# than 0.025 (> 100 x 2e-4) away from the committed iterates before and after it.  admm (it converges within a few
# checks): the last j in 1..3 with M_j >= 1e-3 (a thousand single-precision roundings) and the same distance to the
# earlier checks.
# tol = M_j / 0.8, rounded to two digits: the run stops at iteration 10 j with m = 0.8.
STOP_TOL = {
    ('k33', False, 'parallel_cd', False): 0.096,    # check 3
    ('k33', False, 'parallel_cd', True): 0.12,      # check 3
    ('k33', False, 'admm', False): 0.007,           # check 1
    ('k33', False, 'admm', True): 0.0039,           # check 2
    ('k33', True, 'parallel_cd', False): 0.13,      # check 2
    ('k33', True, 'parallel_cd', True): 0.073,      # check 3
    ('k33', True, 'admm', False): 0.0022,           # check 1
    ('k33', True, 'admm', True): 0.014,             # check 1
    ('k130', False, 'parallel_cd', False): 0.1,     # check 7
    ('k130', False, 'parallel_cd', True): 0.046,    # check 11
    ('k130', False, 'admm', False): 0.0096,         # check 1
    ('k130', False, 'admm', True): 0.0014,          # check 3
}


def rel_err(a, ref):
    """max|a - ref| / max(1, max|ref|): the measure of test_gpu_lasso_extra.py's `_err`."""
    return cd_ref.err(a, ref)


def problem(name, cplx, dtype=None):
    """y [N, F], A [K, F], a sparse non-zero x0 [N, K], mask [F] and mask [N, F] (0 / 1) of SHAPES[name]; codes
    of modulus in [0.3, 0.9] on 5 % of the entries, so that max|x| stays near 1 and `rel_err` is an absolute
    error.  dtype: cast y, A, x0 (masks to its real type); default float64 / complex128."""
    N, F, K = SHAPES[name]
    rng = np.random.RandomState(SEEDS[(name, bool(cplx))])

    def randn(*s):
        return (rng.randn(*s) + 1j * rng.randn(*s)) / np.sqrt(2.0) if cplx else rng.randn(*s)

    def codes(density):
        phase = randn(N, K)
        phase = phase / np.abs(phase)
        return phase * rng.uniform(0.3, 0.9, size=(N, K)) * (rng.uniform(size=(N, K)) < density)
    A = randn(K, F)
    xt = codes(0.05)
    y = xt.dot(A) + 0.1 * randn(N, F)
    x0 = xt + codes(0.05)
    mask1 = (rng.uniform(size=F) > 0.3).astype(np.float64)
    mask2 = (rng.uniform(size=(N, F)) > 0.3).astype(np.float64)
    if dtype is not None:
        dt = np.dtype(dtype)
        assert (dt.kind == 'c') == bool(cplx)
        rdt = real_dtype(dt)
        y, A, x0, mask1, mask2 = y.astype(dt), A.astype(dt), x0.astype(dt), mask1.astype(rdt), mask2.astype(rdt)
    return y, A, x0, mask1, mask2


def parallel_atoms(K, F, cplx, dtype=None, seed=3):
    """K nearly parallel atoms (one direction + 5 % noise): Gershgorin(An An^H) ~ K, so p <= 1."""
    rng = np.random.RandomState(seed)

    def randn(*s):
        return (rng.randn(*s) + 1j * rng.randn(*s)) / np.sqrt(2.0) if cplx else rng.randn(*s)
    A = randn(1, F) + 0.05 * randn(K, F)
    return A if dtype is None else A.astype(dtype)


class Result(object):
    """it, x: what lasso.solve returns; see the module docstring for the rest."""

    def __init__(self):
        self.it, self.x, self.ratio, self.p = None, None, None, None
        self.stats, self.full, self.before, self.after = [], None, None, None


def _working(dtype, like):
    if dtype is not None:
        return np.dtype(dtype)
    return np.dtype(np.complex128 if np.dtype(like).kind == 'c' else np.float64)


def _double(wdt):
    return np.dtype(np.complex128 if wdt.kind == 'c' else np.float64)


def _single(wdt):
    return np.dtype(np.complex64 if wdt.kind == 'c' else np.float32)


def _ratio(v, tol):
    """max |v_k| / tol_k (inf where tol is zero and v is not; nothing where both are)."""
    with np.errstate(divide='ignore', invalid='ignore'):
        q = np.abs(v) / tol
    q = q[~np.isnan(q)]
    return float(np.max(q)) if q.size else 0.0


def pcd_width(A, mask=None, dtype=None):
    """(K / bound, p) of parallel_cd (oracle/lasso.py:161-164) in the working precision `dtype`; a 1-D mask is
    folded into A first, a 2-D mask does not enter."""
    wdt = _working(dtype, A.dtype)
    rdt = real_dtype(wdt)
    A = np.asarray(A).astype(wdt)
    if mask is not None and np.ndim(mask) == 1:
        A = A * np.asarray(mask).astype(rdt)
    s = np.sqrt(np.sum(np.real(np.conj(A) * A), axis=-1)).astype(rdt)
    An = A / s[:, None]
    G = An.dot(np.conj(An.T))
    ratio = rdt.type(A.shape[0]) / gershgorin(G).astype(rdt).reshape(-1)[0]
    assert ratio.dtype == rdt
    return float(ratio), int(ratio)


def solve(y, A, alpha, x=None, tol=1.0e-3, method='parallel_cd', maxiter=1000, mask=None, rho=1.0, dtype=None,
          round_iterates=False):
    """lasso.solve(method='parallel_cd' | 'admm' [+ '_pos'], mask=None | [F] | y's shape, x=, rho=) -> Result."""
    positive = method.endswith('_pos')
    base = method[:-4] if positive else method
    assert base in ('parallel_cd', 'admm')
    wdt = _working(dtype, np.asarray(y).dtype)
    rdt = real_dtype(wdt)
    # ---- oracle/lasso.py:247-265 in the working precision ----
    y, A = np.asarray(y).astype(wdt), np.asarray(A).astype(wdt)
    K, F = A.shape
    shape = y.shape[:-1] + (K,)
    x = np.zeros(shape, wdt) if x is None else np.asarray(x).astype(wdt)
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
        alpha = alpha * rdt.type(F)
    elif mask.ndim == 1:
        alpha = alpha * np.sum(mask)
        mask = None
    else:
        mask = mask.reshape(-1, F)
        alpha = alpha * np.sum(mask, axis=-1, keepdims=True)            # [N, K]
    y, x = y.reshape(-1, F), x.reshape(-1, K)
    shrink = olasso._pick_shrink(A, positive)
    At = olasso._adjoint(A, positive)
    sdt = _single(wdt)

    def rounded(v):
        return v.astype(sdt).astype(wdt) if round_iterates else v

    res = Result()
    res.it = maxiter - 1
    yAt = (y if mask is None else y * mask).dot(At)
    G = A.dot(At)
    res.ratio = float(rdt.type(K) / gershgorin(G).reshape(-1)[0])
    res.p = int(res.ratio)
    if base == 'parallel_cd':
        if res.p <= 1:
            if mask is not None:                                        # oracle/lasso.py:166-170
                raise TypeError("_solve_cd_mask() missing 1 required positional argument: 'xp'")
            raise ValueError('p <= 1: the call is plain coordinate descent (cd_ref.solve)')
        out = _parallel_cd(res, yAt, A, At, G, alpha, x, tol, maxiter, shrink, mask, rounded)
    else:
        out = _admm(res, yAt, A, At, G, alpha, x, tol, maxiter, shrink, mask, rdt.type(rho), rounded)
    for name in ('full', 'before', 'after'):
        if getattr(res, name) is not None:
            setattr(res, name, (getattr(res, name) / s).reshape(shape))
    res.x = (out / s).reshape(shape)
    return res


def _parallel_cd(res, yAt, A, At, G, alpha, x0, tol, maxiter, shrink, mask, rounded):
    """oracle/lasso.py:172-189"""
    K = A.shape[0]
    rng = np.random.RandomState(0)
    select = np.zeros(K, dtype=tol.dtype)
    select[:res.p] = 1.0
    for i in range(maxiter):
        back = x0.dot(G) if mask is None else (x0.dot(A) * mask).dot(At)
        x_new = shrink(x0 + (yAt - back), alpha)
        dx = x_new - x0
        if i % 10 == 0:
            res.stats.append(_ratio(dx, tol))
            if np.max(np.abs(dx) - tol) < 0.0:
                rng.shuffle(select)
                res.it, res.full, res.before, res.after = i, x_new, x0, x0 + dx * select
                return x_new
        rng.shuffle(select)
        x0 = rounded(x0 + dx * select)
    return x0


def _admm(res, yAt, A, At, G, alpha, x, tol, maxiter, shrink, mask, rho, rounded):
    """oracle/lasso.py:193-233; the inverse is worked in double (complex double) in every working precision."""
    K = A.shape[0]
    wdt = A.dtype
    ddt = _double(wdt)
    eye = np.eye(K)
    if mask is None:
        Minv = np.linalg.inv(G.astype(ddt) + float(rho) * eye).astype(wdt)

        def apply_inv(v):
            return v.dot(Minv)
    else:
        Ad = A.astype(ddt)
        S = np.matmul(mask[:, None, :].astype(np.float64) * Ad, At.astype(ddt))        # [N, K, K]
        Sinv = np.linalg.inv(S + float(rho) * eye)

        def apply_inv(v):
            return np.matmul(v[:, None, :].astype(ddt), Sinv)[:, 0, :].astype(wdt)
    thr = alpha / rho
    u = x.copy()
    z = x.copy()
    for i in range(maxiter):
        x_new = apply_inv(yAt + rho * (z - u))
        z = shrink(x_new + u, thr)
        if i % 10 == 0:
            res.stats.append(max(_ratio(x - x_new, tol), _ratio(z - x_new, tol)))
            if np.max(np.abs(x - x_new) - tol) < 0.0 and np.max(np.abs(z - x_new) - tol) < 0.0:
                res.it = i
                return x_new
        x = rounded(x_new)
        u = rounded(u + x - z)
        z = rounded(z)
    return x


# ---- the cases of test_gpu_lasso_extra_shapes.py (the host test walks the same lists) ----------------------------
MASKS = ('nomask', 'mask1d', 'mask2d')
RHOS = (0.1, 1.0, 10.0)
RHO_CASES = (('over', 'nomask'), ('k130', 'nomask'), ('k130', 'mask2d'))
RHO_ITER = 15
LIMIT = {'float32': 2e-4, 'complex64': 2e-4, 'float64': 1e-9, 'complex128': 1e-9}   # test_gpu_lasso_extra.py's


def pick_mask(mname, mask1, mask2):
    return {'nomask': None, 'mask1d': mask1, 'mask2d': mask2}[mname]


def shape_runs(name, cplx, mname):
    """(method, maxiter, rows) of one case of test_shapes_against_the_reference: maxiter alternates 10 / 11 from
    method to method and from mask to mask, so each solver runs out on an even and on an odd count (11 passes the
    second check); masked ADMM at k260 takes the first MASKED_ADMM_ROWS rows."""
    methods = ['parallel_cd', 'admm'] + ([] if cplx else ['admm_pos', 'parallel_cd_pos'])
    runs = []
    for j, method in enumerate(methods):
        rows = MASKED_ADMM_ROWS if (name == 'k260' and mname == 'mask2d' and method.startswith('admm')) else None
        runs.append((method, 10 + (j + MASKS.index(mname)) % 2, rows))
    return runs


def stop_runs(i_star):
    """(tol is the case's, maxiter, expected it) for a reference that stops at i_star, + the stop at iteration 0."""
    return [(None, i_star, i_star - 1), (None, i_star + 1, i_star), (None, i_star + 5, i_star), (1.0e3, 50, 0)]


def inverse_batches(n, dtype, seed=11):
    """[3, n, n]: (a) random; (b) diagonally dominant with its rows reversed: the pivot of column k sits in row
    n - 1 - k, and in the columns k < n - 256 it is the only non-zero entry, so a pivot search that stops at row 256
    finds nothing to divide by; (c) A A^H + I with A [n, 2 n]."""
    rng = np.random.RandomState(seed + n)
    cplx = np.dtype(dtype).kind == 'c'

    def randn(*s):
        return (rng.randn(*s) + 1j * rng.randn(*s)) / np.sqrt(2.0) if cplx else rng.randn(*s)
    a = randn(n, n)
    b = randn(n, n) / n
    b[:, :n - 256] = 0.0
    b = (b + np.diag(1.0 + rng.uniform(size=n)))[::-1]
    A = randn(n, 2 * n) / np.sqrt(2.0 * n)
    c = A.dot(np.conj(A.T)) + np.eye(n)
    return np.stack([a, b, c]).astype(dtype)


def cut_rows(rows, y, x0, mask):
    """The first `rows` rows of a problem (rows = None: all of it); a 1-D mask stays whole."""
    if rows is None:
        return y, x0, mask
    return y[:rows], x0[:rows], mask[:rows] if (mask is not None and mask.ndim == 2) else mask
