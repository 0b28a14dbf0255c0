"""NumPy references for masked orthogonal matching pursuit (decomp_amd.omp.solve(mask=...),
decomp_amd/csrc/omp_mask.hpp) and the problems its tests share.  Test infrastructure only.

For one row y [F], A [K, F] and weights m [F] >= 0, with <u, v>_m = sum_f m_f u_f conj(v_f):
  double reference   omp_ref.omp_lstsq on (y sqrt(m), A sqrt(m)): the unweighted algorithm on the scaled row IS the
                     weighted one, and its coefficients are those for the unscaled A
  restate            the residual form of omp_mask.hpp in a working dtype: W = m |A|^2^T, alpha = (m o r) A^H,
                     c = |alpha| / sqrt(W), the pivot from g_j = <a_Ij, a_k*>_m, z_n = conj(alpha_k*) / sqrt(d),
                     x through the extended factor, r rebuilt from y -- products, weighted norms, factor and
                     residual all formed in that dtype
"""
import functools

import numpy as np

import omp_ref

ROWS = 257
KEEP = 0.7
# (case, single precision runs (mask kind, with_tol)); double precision runs everything.  Shares left out of the
# support comparison by the recipe below were computed on the CPU for all six cases (test_omp_mask_ref_host.py
# asserts them): cases 15 and 16 exceed the 10 % cap in single precision, case 13 in all but binary / fixed sparsity.
KINDS = ('binary', 'weights')
SINGLE_RUNS = {11: [(k, t) for k in KINDS for t in (False, True)],
               12: [(k, t) for k in KINDS for t in (False, True)],
               14: [(k, t) for k in KINDS for t in (False, True)],
               13: [('binary', False)]}
CASES = sorted(omp_ref.CASES)


def case_masks(case):
    """(binary, weights) of a case, by the issue's recipe: one generator, keep [257, F] first, then the weights; the
    rows the case has (cases 15 and 16 have 131) are the first of them."""
    seed, N, F = omp_ref.CASES[case][:3]
    rng = np.random.RandomState(1000 + seed)
    keep = rng.rand(ROWS, F) < KEEP
    binary = keep.astype(np.float64)
    weights = np.where(keep, 0.25 + 0.75 * rng.rand(ROWS, F), 0).astype(np.float32).astype(np.float64)
    rows = min(ROWS, N)
    return omp_ref._freeze(np.ascontiguousarray(binary[:rows]), np.ascontiguousarray(weights[:rows]))


def reference(y, A, m, s, tol=None):
    """Per row i omp_lstsq(y_i sqrt(m_i), A sqrt(m_i), s, tol) in the dtype given (double in the tests).
    Returns (x [N, K], steps, margin, resid_margin)."""
    N, K = y.shape[0], A.shape[0]
    x = np.zeros((N, K), dtype=np.result_type(y, A))
    steps = np.zeros(N, dtype=np.int64)
    margin = np.full(N, np.inf)
    rmargin = np.full(N, np.inf)
    for i in range(N):
        sq = np.sqrt(m[i])
        xi, st, mg, rm = omp_ref.omp_lstsq((y[i] * sq)[None, :], A * sq[None, :], s, tol=tol)
        x[i], steps[i], margin[i], rmargin[i] = xi[0], st[0], mg[0], rm[0]
    return x, steps, margin, rmargin


def restate(y, A, m, s, tol=None, dtype=None, eps=None):
    """The residual form of omp_mask.hpp, every quantity in `dtype`.  Returns (x, steps)."""
    dt = np.dtype(dtype if dtype is not None else np.result_type(y, A))
    rdt = np.zeros(1, dt).real.dtype
    y, A, m = y.astype(dt), A.astype(dt), m.astype(rdt)
    if eps is None:
        eps = omp_ref.eps_dep(dt)
    eps = rdt.type(eps)
    N, K = y.shape[0], A.shape[0]
    AH = A.conj().T.copy()
    A2 = (np.abs(A) ** 2).astype(rdt)
    x = np.zeros((N, K), dtype=dt)
    steps = np.zeros(N, dtype=np.int64)
    tol_t = None if tol is None else rdt.type(tol)
    for i in range(N):
        mi, yi = m[i], y[i]
        W = A2 @ mi                                   # n_k^2 of this row
        ok = W > 0
        nrm = np.sqrt(np.where(ok, W, 1))
        r = yi
        r2 = np.sum(mi * np.abs(yi) ** 2)
        I, L, z, xi = [], [], [], None
        for _ in range(s):
            if tol_t is not None and not r2 > tol_t:
                break
            alpha = (mi * r).astype(dt) @ AH
            c = np.where(ok, np.abs(alpha) / nrm, -1).astype(rdt)
            c[I] = -1
            k = int(np.argmax(c))
            if not c[k] > 0:
                break
            mk = (mi * np.conj(A[k])).astype(dt)
            g = A[I] @ mk if I else np.zeros(0, dtype=dt)
            gkk = (A[k] @ mk).real
            w, d = omp_ref._chol_pivot(L, g, gkk)
            if not d > eps * gkk:
                break
            row = np.concatenate([w.conj(), [np.sqrt(d)]]).astype(dt)
            z.append(dt.type(np.conj(alpha[k]) / row[-1]))
            L.append(row)
            I.append(k)
            n = len(I)
            v = np.zeros(n, dtype=dt)               # L^H v = z
            t = np.array(z, dtype=dt)
            for q in range(n - 1, -1, -1):
                v[q] = t[q] / L[q][q]
                t[:q] -= np.conj(L[q][:q]) * v[q]
            xi = np.conj(v)
            r = (yi - xi @ A[I]).astype(dt)
            r2 = np.sum(mi * np.abs(r) ** 2)
        if I:
            x[i, I] = xi
        steps[i] = len(I)
    return x, steps


def row_metrics(x, y, A, m):
    """Per row, in double and in the weighted inner product: |y - x A|_m / |y|_m and
    max_j in support |<r, a_j>_m| / (|y|_m n_j(row))."""
    x = np.asarray(x).astype(y.dtype).reshape(y.shape[0], -1)
    r = y - x @ A
    yn = np.sqrt(np.sum(m * np.abs(y) ** 2, axis=1))
    yn = np.where(yn > 0, yn, 1.0)
    W = m @ (np.abs(A) ** 2).T
    nrm = np.sqrt(np.where(W > 0, W, 1.0))
    corr = np.abs((m * r) @ A.conj().T) / nrm
    corr = np.where(x != 0, corr, 0.0).max(axis=1)
    return np.sqrt(np.sum(m * np.abs(r) ** 2, axis=1)) / yn, corr / yn


class Analysis(object):
    """For a double problem (y [N, F], A, m [N, F] or [F]) with single-exact entries, a sparsity and an optional tol:
      x, steps, margin, resid_margin   reference() in double
      keep(precision)                  rows whose support is compared (omp_ref.DELTA, omp_ref.RESID_DELTA)
      cpu(precision)                   (x, steps) of the working-dtype restatement: restate() (form 'residual'), or
                                       omp_ref.omp_gram on the products of the scaled problem (form 'gram': what a
                                       1-D mask runs)
      bounds(precision)                the rule of omp_ref.Analysis.bounds: 4 x what cpu(precision) shows against the
                                       double reference, floor 64 eps; coefficients over the compared rows relative to
                                       max|x_ref|, weighted orthogonality and residual excess over every row."""

    def __init__(self, y, A, m, s, tol=None, form='residual'):
        m = np.asarray(m, dtype=np.float64)
        self.shared = m.ndim == 1
        self.m1 = m
        self.m = np.ascontiguousarray(np.broadcast_to(m, y.shape))
        self.y, self.A, self.s, self.tol, self.form = y, A, s, tol, form
        self.cplx = np.iscomplexobj(A)
        self.x, self.steps, self.margin, self.resid_margin = omp_ref._freeze(*reference(y, A, self.m, s, tol=tol))
        self._cpu = {}

    def dtype(self, precision):
        return omp_ref.precision_dtype(self.cplx, precision)

    def rdtype(self, precision):
        return np.float32 if precision == 'single' else np.float64

    def keep(self, precision):
        keep = self.margin >= omp_ref.DELTA[precision]
        if self.tol is not None:
            keep = keep & (self.resid_margin >= omp_ref.RESID_DELTA)
        return keep

    def left_out(self, precision):
        return 1.0 - float(np.mean(self.keep(precision)))

    def cpu(self, precision):
        if precision not in self._cpu:
            dt = self.dtype(precision)
            if self.form == 'gram':
                sq = np.sqrt(self.m1).astype(self.rdtype(precision))
                ys, As = self.y.astype(dt) * sq, self.A.astype(dt) * sq
                yn2 = np.sum(np.abs(ys) ** 2, axis=1).astype(sq.dtype)
                tol = None if self.tol is None else sq.dtype.type(self.tol)
                out = omp_ref.omp_gram(ys @ As.conj().T, As @ As.conj().T, yn2, self.s, tol=tol)
            else:
                out = restate(self.y, self.A, self.m, self.s, tol=self.tol, dtype=dt)
            self._cpu[precision] = omp_ref._freeze(*out)
        return self._cpu[precision]

    def bounds(self, precision, keep=None):
        eps = float(np.finfo(self.dtype(precision)).eps)
        xc = self.cpu(precision)[0]
        keep = self.keep(precision) if keep is None else keep
        coef = float(np.max(np.abs(xc.astype(self.x.dtype) - self.x)[keep], initial=0.0)) / float(np.max(np.abs(self.x)))
        res_c, orth_c = row_metrics(xc, self.y, self.A, self.m)
        res_r, _ = row_metrics(self.x, self.y, self.A, self.m)
        floor = 64 * eps
        return (max(4 * coef, floor), max(4 * float(orth_c.max()), floor),
                max(4 * float(np.max(res_c - res_r)), floor))


def case_problem(case):
    """The first 257 rows of omp_ref.case_problem(case)."""
    y, A = omp_ref.case_problem(case)
    return y[:ROWS], A


def case_tol(case, kind):
    y, _ = case_problem(case)
    m = case_masks(case)[KINDS.index(kind)]
    return 0.02 * float(np.median(np.sum(m * np.abs(y) ** 2, axis=1)))


@functools.lru_cache(maxsize=None)
def case_analysis(case, kind, with_tol):
    """s = S; with tol the sparsity of omp.solve(tol=...) alone, min(K, F, cap)."""
    seed, N, F, K, S, cplx = omp_ref.CASES[case]
    y, A = case_problem(case)
    m = case_masks(case)[KINDS.index(kind)]
    if with_tol:
        return Analysis(y, A, m, min(K, F, omp_ref.CAP['c' if cplx else 'f']), tol=case_tol(case, kind))
    return Analysis(y, A, m, S)
