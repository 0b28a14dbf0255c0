"""NumPy references for orthogonal matching pursuit (decomp_amd.omp, decomp_amd/csrc/omp.hpp) and the problems the
OMP tests share.  Test infrastructure only.

The algorithm, for one row y [F] and A [K, F], G = A A^H, n_k = sqrt(G_kk), support I = (), r = y, at most s times:
  1. tol given and |r|^2 <= tol: stop
  2. c_k = |r a_k^H| / n_k over k not in I with n_k > 0; k* = the lowest index attaining the maximum; maximum <= 0: stop
  3. L w = G[I, k*], d = G_k*k* - |w|^2; d <= eps_dep G_k*k*: stop, keeping the previous solution
  4. I <- I + (k*), x_I = argmin |y - x_I A_I|, r = y - x_I A_I
"""
import functools

import numpy as np

CAP = {'f': 64, 'c': 32}

# (seed, N, F, K, S, cplx)
CASES = {11: (11, 509, 48, 40, 5, False), 12: (12, 509, 24, 70, 8, False), 13: (13, 509, 64, 130, 16, False),
         14: (14, 509, 24, 70, 8, True), 15: (15, 131, 96, 300, 32, False), 16: (16, 131, 80, 200, 32, True)}
SINGLE_CASES = (11, 12, 13, 14)     # cases 15 and 16: a third of the rows has a margin below 1e-4, double only
DELTA = {'single': 1e-4, 'double': 1e-8}
RESID_DELTA = 1e-4
MAX_LEFT_OUT = 0.10


def eps_dep(dtype):
    """The kernel's dependence threshold for a dtype: 4096 eps of its real type."""
    return 4096.0 * float(np.finfo(np.dtype(dtype)).eps)


def make_problem(seed, N, F, K, S, cplx, noise=0.05):
    rng = np.random.RandomState(seed)
    A = rng.randn(K, F) * (0.5 + rng.rand(K, 1))
    if cplx:
        A = A + 1j * rng.randn(K, F)
    x0 = np.zeros((N, K))
    for i in range(N):
        idx = rng.choice(K, S, replace=False)
        x0[i, idx] = (1 + rng.rand(S)) * rng.choice([-1, 1], S)
    y = x0 @ A
    scale = noise * np.linalg.norm(y, axis=1, keepdims=True) / np.sqrt(F)
    e = rng.randn(N, F)
    if cplx:
        e = e + 1j * rng.randn(N, F)
    return y + scale * e, A


def _chol_pivot(L, g_col, gkk):
    """w of L w = g_col and the pivot d = gkk - |w|^2 (L: list of rows of the factor so far)."""
    n = len(L)
    w = np.zeros(n, dtype=g_col.dtype)
    for m in range(n):
        w[m] = (g_col[m] - np.sum(L[m][:m] * w[:m])) / L[m][m]
    return w, gkk - np.sum(np.abs(w) ** 2).real


def omp_lstsq(y, A, s, tol=None, eps=None):
    """The algorithm with np.linalg.lstsq on the support, in the input dtype.  y [..., F].
    Returns (x, steps [N], margin [N], resid_margin [N]): margin is the smallest (c_(1) - c_(2)) / |y| over the
    row's steps, resid_margin the smallest | |r|^2 - tol | / |y|^2 (inf without tol)."""
    F = A.shape[1]
    K = A.shape[0]
    y2 = y.reshape(-1, F)
    N = y2.shape[0]
    if eps is None:
        eps = eps_dep(y.dtype)
    AH = A.conj().T
    G = A @ AH
    g = G.diagonal().real
    nrm = np.sqrt(np.maximum(g, 0))
    x = np.zeros((N, K), dtype=y.dtype)
    steps = np.zeros(N, dtype=np.int64)
    margin = np.full(N, np.inf)
    rmargin = np.full(N, np.inf)
    for i in range(N):
        yi = y2[i]
        yn2 = float(np.vdot(yi, yi).real)
        I, L, coef, r = [], [], None, yi
        for _ in range(s):
            if tol is not None:
                r2 = float(np.vdot(r, r).real)
                if yn2 > 0:
                    rmargin[i] = min(rmargin[i], abs(r2 - tol) / yn2)
                if r2 <= tol:
                    break
            c = np.where(nrm > 0, np.abs(r @ AH) / np.where(nrm > 0, nrm, 1), -1.0)
            c[I] = -1.0
            k = int(np.argmax(c))                       # the first maximum: the lowest index
            if not c[k] > 0:
                break
            if K > 1 and yn2 > 0:
                second = np.partition(c, K - 2)[K - 2]
                margin[i] = min(margin[i], (c[k] - max(second, 0.0)) / np.sqrt(yn2))
            w, d = _chol_pivot(L, G[I, k], g[k])
            if not d > eps * g[k]:
                break
            L.append(np.concatenate([w.conj(), [np.sqrt(d)]]))
            I.append(k)
            coef = np.linalg.lstsq(A[I].T, yi, rcond=None)[0]
            r = yi - coef @ A[I]
        if I:
            x[i, I] = coef
        steps[i] = len(I)
    return x.reshape(y.shape[:-1] + (K,)), steps, margin, rmargin


def omp_gram(alpha0, G, ynorm2, s, tol=None, eps=None):
    """The same algorithm in Gram form (alpha = alpha0 - x_I G[I, :], |r|^2 = |y|^2 - Re(x_I . conj(alpha0_I)),
    x_I through the progressively extended Cholesky factor), in whatever dtype it is given.  alpha0 [N, K].
    Returns (x, steps)."""
    N, K = alpha0.shape
    dt = alpha0.dtype
    if eps is None:
        eps = eps_dep(dt)
    g = G.diagonal().real
    nrm = np.sqrt(np.maximum(g, 0))
    x = np.zeros((N, K), dtype=dt)
    steps = np.zeros(N, dtype=np.int64)
    for i in range(N):
        a0 = alpha0[i]
        I, L, z, xi = [], [], [], None
        alpha = a0
        r2 = None if tol is None else ynorm2[i]
        for _ in range(s):
            if tol is not None and r2 <= tol:
                break
            c = np.where(nrm > 0, np.abs(alpha) / np.where(nrm > 0, nrm, 1), -1)
            c[I] = -1
            k = int(np.argmax(c))
            if not c[k] > 0:
                break
            w, d = _chol_pivot(L, G[I, k], g[k])
            if not d > g.dtype.type(eps) * g[k]:
                break
            row = np.concatenate([w.conj(), [np.sqrt(d)]]).astype(dt)
            z.append((np.conj(a0[k]) - np.sum(row[:-1] * np.array(z, dtype=dt))) / row[-1])
            L.append(row)
            I.append(k)
            n = len(I)
            v = np.zeros(n, dtype=dt)           # L^H v = z
            t = np.array(z, dtype=dt)
            for m in range(n - 1, -1, -1):
                v[m] = t[m] / L[m][m]
                t[:m] -= np.conj(L[m][:m]) * v[m]
            xi = np.conj(v)
            alpha = a0 - xi @ G[I, :]
            if tol is not None:
                r2 = ynorm2[i] - np.sum(xi * np.conj(a0[I])).real
        if I:
            x[i, I] = xi
        steps[i] = len(I)
    return x, steps


def solve_fastpath_omp(y, A, alpha, x, tol, maxiter, method, mask=None, trace=None):
    """The signature of oracle.lasso.solve_fastpath with OMP inside: maxiter is the sparsity, tol the residual
    tolerance (None or negative: none); alpha, x and method are not read.  Patched into
    oracle.dictionary_learning.lasso it gives the reference dictionary loop for lasso_method='omp'."""
    assert mask is None
    t = None if tol is None or tol < 0 else tol
    xo, steps, _, _ = omp_lstsq(y, A, int(maxiter), tol=t)
    return int(steps.max()) if len(steps) else 0, xo


# ---- what the GPU tests compare against (computed once per session, never modified) ------------------------
def _freeze(*arrays):
    for a in arrays:
        a.setflags(write=False)
    return arrays


def single_exact(y, A):
    """(y, A) in double precision with entries that single precision represents exactly: one double reference then
    serves the tests of both precisions."""
    cplx = np.iscomplexobj(A)
    single, double = (np.complex64, np.complex128) if cplx else (np.float32, np.float64)
    return _freeze(y.astype(single).astype(double), A.astype(single).astype(double))


def precision_dtype(cplx, precision):
    if precision == 'single':
        return np.complex64 if cplx else np.float32
    return np.complex128 if cplx else np.float64


def row_metrics(x, y, A):
    """Per row, in double: |y - x A| / |y| and max_j in support |r a_j^H| / (|y| n_j)."""
    x = np.asarray(x).astype(y.dtype).reshape(y.shape[0], -1)
    r = y - x @ A
    yn = np.linalg.norm(y, axis=1)
    yn = np.where(yn > 0, yn, 1.0)
    nrm = np.linalg.norm(A, axis=1)
    corr = np.abs(r @ A.conj().T) / np.where(nrm > 0, nrm, 1.0)[None, :]
    corr = np.where(x != 0, corr, 0.0).max(axis=1)
    return np.linalg.norm(r, axis=1) / yn, corr / yn


class Analysis(object):
    """For a double problem (y [N, F], A) with single-exact entries, a sparsity and an optional tol:
      x, steps, margin, resid_margin   omp_lstsq in double
      keep(precision)                  rows whose support is compared: margin >= delta (1e-4 single, 1e-8 double)
                                       and, with tol, residual margin >= 1e-4
      cpu(precision)                   (x, steps) of omp_gram on the CPU in that dtype, products formed in it too
      bounds(precision)                (coefficient, orthogonality, residual) bounds for the GPU result: 4 x what
                                       cpu(precision) shows against the double reference (the factor covers the other
                                       summation order of the MFMA products and of the substitutions), floor 64 eps;
                                       coefficients over the compared rows relative to max|x_ref|, the other two over
                                       every row relative to |y|."""

    def __init__(self, y, A, s, tol=None):
        self.y, self.A, self.s, self.tol = y, A, s, tol
        self.cplx = np.iscomplexobj(A)
        self.x, self.steps, self.margin, self.resid_margin = _freeze(*omp_lstsq(y, A, s, tol=tol))
        self._cpu = {}

    def dtype(self, precision):
        return precision_dtype(self.cplx, precision)

    def keep(self, precision):
        keep = self.margin >= DELTA[precision]
        if self.tol is not None:
            keep = keep & (self.resid_margin >= RESID_DELTA)
        return keep

    def products(self, precision):
        dt = self.dtype(precision)
        y, A = self.y.astype(dt), self.A.astype(dt)
        alpha0 = y @ A.conj().T
        return alpha0, A @ A.conj().T, np.sum(np.abs(y) ** 2, axis=1).astype(alpha0.real.dtype)

    def cpu(self, precision):
        if precision not in self._cpu:
            alpha0, G, yn2 = self.products(precision)
            tol = None if self.tol is None else yn2.dtype.type(self.tol)
            self._cpu[precision] = _freeze(*omp_gram(alpha0, G, yn2, self.s, tol=tol))
        return self._cpu[precision]

    def bounds(self, precision, keep=None):
        eps = float(np.finfo(self.dtype(precision)).eps)
        xc = self.cpu(precision)[0]
        keep = self.keep(precision) if keep is None else keep
        coef = float(np.max(np.abs(xc.astype(self.x.dtype) - self.x)[keep], initial=0.0)) / float(np.max(np.abs(self.x)))
        res_c, orth_c = row_metrics(xc, self.y, self.A)
        res_r, _ = row_metrics(self.x, self.y, self.A)
        floor = 64 * eps
        return (max(4 * coef, floor), max(4 * float(orth_c.max()), floor),
                max(4 * float(np.max(res_c - res_r)), floor))


@functools.lru_cache(maxsize=None)
def case_problem(case):
    seed, N, F, K, S, cplx = CASES[case]
    return single_exact(*make_problem(seed, N, F, K, S, cplx))


def case_tol(case):
    y, _ = case_problem(case)
    return 0.02 * float(np.median(np.sum(np.abs(y) ** 2, axis=1)))


@functools.lru_cache(maxsize=None)
def case_analysis(case, with_tol):
    """s = S; with tol the sparsity of omp.solve(tol=...) alone, min(K, F, cap)."""
    seed, N, F, K, S, cplx = CASES[case]
    y, A = case_problem(case)
    if with_tol:
        return Analysis(y, A, min(K, F, CAP['c' if cplx else 'f']), tol=case_tol(case))
    return Analysis(y, A, S)
