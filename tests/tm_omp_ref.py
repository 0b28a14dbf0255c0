"""NumPy references for orthogonal convolutional pursuit (decomp_amd.template_matching.orthogonal_pursuit,
decomp_amd/csrc/template_omp.hpp) and the problems its tests share.  Test infrastructure only.

The algorithm, for one signal y [N] and templates D [T, S], with A[(t, c), n] = D[t, n - s c + Q],
rho2[t, c] = |A_(t,c)|^2 and G[i, k] = A_i . A_k^H over the samples inside [0, N), support I = (), x = 0, E = |y|^2,
at most n times:
  1. tol given and E <= tol: stop
  2. alpha_k = r . A_k^H; score = |alpha_k|^2 / rho2_k over the atoms with rho2_k > 0 outside I; the lowest flat index
     t C + c attaining the maximum; maximum not > 0: stop
  3. L w = G[I, k*], d = rho2_k* - |w|^2; d <= eps_dep rho2_k*: stop, keeping the previous x
  4. I <- I + (k*); x_I = the least-squares fit of y on A_I; E = |y - x_I A_I|^2
omp_residual recomputes alpha from the residual at every step and fits with np.linalg.lstsq; omp_gram keeps alpha up
to date through the lag correlations and fits through the Cholesky factor, as the kernel does.
"""
import functools

import numpy as np

import omp_ref
import tm_pursuit_ref as mp
from oracle import template_matching as otm
from omp_ref import precision_dtype, eps_dep
from tm_pursuit_ref import _windows, _fold, predict, residual_norm, DELTA, RESID_DELTA, MAX_LEFT_OUT, CASES

CAP = omp_ref.CAP


def cap_of(cplx):
    return CAP['c' if cplx else 'f']


def _rho2(D, valid):
    return (np.abs(D) ** 2) @ valid.T.astype(np.float64)        # [T, C]


def correlate(r, D, N, stride, padding):
    """r A^H without the dense operator: r [B, N] -> [B, T, C], in double."""
    T, S = D.shape
    C, base, valid = _windows(S, N, stride, padding)
    idx = S + base[:, None] + np.arange(S)[None, :]
    rp = np.zeros((r.shape[0], N + 2 * S), dtype=np.result_type(r.dtype, D.dtype))
    rp[:, S:S + N] = r
    return np.einsum('bcs,ts->btc', rp[:, idx], np.conj(D))


def orthogonality(x, y, D, N, stride, padding):
    """max over the support (x != 0) of |r . A_j^H| / (rho_j |y|) per signal, r = y - x * D, in double."""
    x = np.asarray(x).astype(y.dtype)
    _, _, valid = _windows(D.shape[1], N, stride, padding)
    rho = np.sqrt(_rho2(D, valid))
    r = y - predict(x, D, N, stride, padding)
    a = np.abs(correlate(r, D, N, stride, padding)) / np.where(rho > 0, rho, 1.0)[None]
    yn = np.linalg.norm(y, axis=1)
    return np.where(x != 0, a, 0.0).reshape(x.shape[0], -1).max(axis=1) / np.where(yn > 0, yn, 1.0)


def _atom(D, N, base, valid, C, i):
    """Atom i = t C + c as an [N] vector."""
    t, c = divmod(i, C)
    a = np.zeros(N, dtype=D.dtype)
    v = valid[c]
    a[base[c] + np.flatnonzero(v)] = D[t, v]
    return a


def omp_residual(y, D, N, stride, padding, n=None, tol=None, eps=None):
    """The algorithm with alpha recomputed from the residual at every step and np.linalg.lstsq on the support's atoms,
    in double; neither the dense operator nor G is formed.  y [B, N].
    Returns (x [B, T, C], steps [B], margin [B], resid_margin [B]) with the margins of omp_ref.omp_lstsq on
    c = |alpha| / rho: the smallest (c_(1) - max(c_(2), 0)) / |y| over the signal's steps, and the smallest
    |E - tol| / |y|^2 (inf without tol)."""
    cplx = np.iscomplexobj(D) or np.iscomplexobj(y)
    dt = np.complex128 if cplx else np.float64
    y = np.asarray(y, dtype=dt)
    D = np.asarray(D, dtype=dt)
    T, S = D.shape
    B = y.shape[0]
    C, base, valid = _windows(S, N, stride, padding)
    K = T * C
    n = min(K, cap_of(cplx)) if n is None else n
    if eps is None:
        eps = eps_dep(dt)
    idx = S + base[:, None] + np.arange(S)[None, :]
    rho2 = _rho2(D, valid)
    rho = np.sqrt(rho2).ravel()
    Dc = np.conj(D)
    x = np.zeros((B, K), dtype=dt)
    steps = np.zeros(B, dtype=np.int64)
    margin = np.full(B, np.inf)
    rmargin = np.full(B, np.inf)
    for b in range(B):
        yn2 = float(np.sum(np.abs(y[b]) ** 2))
        I, L, atoms, coef, r = [], [], [], None, y[b]
        for _ in range(n):
            if tol is not None:
                E = float(np.sum(np.abs(r) ** 2))
                if yn2 > 0:
                    rmargin[b] = min(rmargin[b], abs(E - tol) / yn2)
                if E <= tol:
                    break
            rp = np.zeros(N + 2 * S, dtype=dt)
            rp[S:S + N] = r
            alpha = (rp[idx] @ Dc.T).T.ravel()
            c = np.where(rho > 0, np.abs(alpha) / np.where(rho > 0, rho, 1.0), -1.0)
            c[I] = -1.0
            k = int(np.argmax(c))                               # the first maximum: the lowest flat index
            if not c[k] > 0:
                break
            if K > 1 and yn2 > 0:
                second = np.partition(c, K - 2)[K - 2]
                margin[b] = min(margin[b], (c[k] - max(second, 0.0)) / np.sqrt(yn2))
            ak = _atom(D, N, base, valid, C, k)
            gcol = np.array([np.sum(a * np.conj(ak)) for a in atoms], dtype=dt)
            w, d = omp_ref._chol_pivot(L, gcol, rho2.ravel()[k])
            if not d > eps * rho2.ravel()[k]:
                break
            L.append(np.concatenate([w.conj(), [np.sqrt(d)]]))
            I.append(k)
            atoms.append(ak)
            AI = np.array(atoms)
            coef = np.linalg.lstsq(AI.T, y[b], rcond=None)[0]
            r = y[b] - coef @ AI
        if I:
            x[b, I] = coef
        steps[b] = len(I)
    return x.reshape(B, T, C), steps, margin, rmargin


def omp_gram(y, D, N, stride, padding, n=None, tol=None, eps=None, skip_unchanged=True):
    """The same algorithm in the Gram-update form of the kernel, in whatever dtype it is given: alpha0 = y A^H once;
    G[i, k] from the lag correlations Corr[t, t', m] = sum_k D[t, k] conj(D[t', k + m]) when atom i lies inside the
    signal, else the explicit sum over the overlap inside [0, N); x_I through the progressively extended Cholesky
    factor; alpha -= sum_j (x_j - x_j^previous) G[I_j, :] over the atoms within dh of I_j, j in order, the terms with
    x_j == x_j^previous left out (skip_unchanged; the newest atom's never); E = |y|^2 - Re(x_I . conj(alpha0_I)).
    Returns (x, steps)."""
    dt = y.dtype
    rt = np.zeros(1, dtype=dt).real.dtype
    cplx = dt.kind == 'c'
    T, S = D.shape
    B = y.shape[0]
    C, base, valid = _windows(S, N, stride, padding)
    K = T * C
    n = min(K, cap_of(cplx)) if n is None else n
    eps = rt.type(eps_dep(dt) if eps is None else eps)
    dh = (S - 1) // stride
    Dc = np.conj(D)
    idx = S + base[:, None] + np.arange(S)[None, :]
    rho2 = _fold(np.stack([np.where(valid[None, :, k], (np.abs(D[:, k]) ** 2).astype(rt)[:, None], rt.type(0))
                           for k in range(S)]))                  # [T, C]
    corr = np.zeros((T, T, 2 * S - 1), dtype=dt)                # every lag's sum over k in increasing k
    for k in range(S):
        corr[:, :, S - 1 - k:2 * S - 1 - k] = corr[:, :, S - 1 - k:2 * S - 1 - k] + D[:, k][:, None, None] * Dc[None]
    inside = valid.all(axis=1)

    def gram_row(t, cc, cps):
        """G[(t, cc), (:, cps)]: [T, len(cps)]."""
        ms = stride * (cc - cps)
        if inside[cc]:
            return corr[t][:, ms + S - 1]
        G = np.zeros((T, len(cps)), dtype=dt)
        for j, m in enumerate(ms):
            ks = [k for k in range(max(0, -m), min(S - 1, S - 1 - m) + 1) if valid[cc, k]]
            if ks:
                G[:, j] = _fold(np.stack([D[t, k] * Dc[:, k + m] for k in ks]))
        return G

    def gram(i, k):
        (t, cc), (tp, cp) = divmod(i, C), divmod(k, C)
        if abs(cc - cp) > dh:
            return dt.type(0)
        return gram_row(t, cc, np.array([cp]))[tp, 0]

    safe = np.where(rho2 > 0, rho2, rt.type(1))
    x = np.zeros((B, K), dtype=dt)
    steps = np.zeros(B, dtype=np.int64)
    tol_t = None if tol is None else rt.type(tol)
    for b in range(B):
        yp = np.zeros(N + 2 * S, dtype=dt)
        yp[S:S + N] = y[b]
        alpha0 = _fold(np.stack([np.outer(Dc[:, k], yp[idx[:, k]]) for k in range(S)]))    # [T, C]
        alpha = alpha0.copy()
        yn2 = rt.type(np.sum((np.abs(y[b]) ** 2).astype(rt)))
        E = yn2
        I, L, z = [], [], []
        xi = np.zeros(0, dtype=dt)
        for _ in range(n):
            if tol_t is not None and E <= tol_t:
                break
            score = np.where(rho2 > 0, (alpha.real * alpha.real + alpha.imag * alpha.imag) / safe, rt.type(-1)).ravel()
            score[I] = -1
            k = int(np.argmax(score))
            if not score[k] > 0:
                break
            gkk = rho2.ravel()[k]
            gcol = np.array([gram(i, k) for i in I], dtype=dt)
            w, d = omp_ref._chol_pivot(L, gcol, gkk)
            if not d > eps * gkk:
                break
            row = np.concatenate([w.conj(), [np.sqrt(d)]]).astype(dt)
            z.append((np.conj(alpha0.ravel()[k]) - np.sum(row[:-1] * np.array(z, dtype=dt))) / row[-1])
            L.append(row)
            I.append(k)
            m_ = len(I)
            v = np.zeros(m_, dtype=dt)           # L^H v = z
            t_ = np.array(z, dtype=dt)
            for m in range(m_ - 1, -1, -1):
                v[m] = t_[m] / L[m][m]
                t_[:m] -= np.conj(L[m][:m]) * v[m]
            xnew = np.conj(v)
            dx = xnew - np.concatenate([xi, [0]]).astype(dt)
            xi = xnew
            for j, i in enumerate(I):
                if skip_unchanged and j != m_ - 1 and dx[j] == 0:
                    continue
                t, cc = divmod(i, C)
                ca, cb = max(cc - dh, 0), min(cc + dh, C - 1)
                alpha[:, ca:cb + 1] = alpha[:, ca:cb + 1] - dx[j] * gram_row(t, cc, np.arange(ca, cb + 1))
            E = rt.type(yn2 - np.sum(xi * np.conj(alpha0.ravel()[I])).real)
            steps[b] += 1
        if I:
            x[b, I] = xi
    return x.reshape(B, T, C), steps


# ---- what the GPU tests compare against (computed once per session, never modified) --------------------------------
class Analysis(object):
    """For a double problem (y, D) with single-exact entries: the double reference (x, steps, margin, resid_margin) of
    omp_residual, keep(precision), cpu(precision) = omp_gram in that dtype, and bounds(precision) = (coefficient,
    orthogonality, residual) bounds for the GPU result: 4 x what cpu(precision) shows against the double reference (the
    factor covers the fused multiply-adds and the other summation order of the kernel), floor 64 eps; coefficients over
    the compared signals relative to max|x_ref|, orthogonality and residual over every signal relative to |y|."""

    def __init__(self, y, D, geom, n=None, tol=None):
        self.y, self.D, self.geom, self.n, self.tol = y, D, geom, n, tol
        self.cplx = np.iscomplexobj(D)
        N, stride, padding = geom
        self.x, self.steps, self.margin, self.resid_margin = omp_residual(y, D, N, stride, padding, n, tol)
        for a in (self.x, self.steps, self.margin, self.resid_margin):
            a.setflags(write=False)
        self.res = residual_norm(self.x, y, D, N, stride, padding)
        self._cpu = {}

    def dtype(self, precision):
        return precision_dtype(self.cplx, precision)

    def keep(self, precision):
        keep = self.margin >= DELTA[precision]
        if self.tol is not None:
            keep = keep & (self.resid_margin >= RESID_DELTA)
        return keep

    def left_out(self, precision):
        return 1.0 - float(np.mean(self.keep(precision)))

    def cpu(self, precision):
        if precision not in self._cpu:
            dt = self.dtype(precision)
            N, stride, padding = self.geom
            self._cpu[precision] = omp_gram(self.y.astype(dt), self.D.astype(dt), N, stride, padding, self.n, self.tol)
        return self._cpu[precision]

    def metrics(self, x):
        """(residual excess over the reference's, orthogonality) per signal of a result x, in double."""
        N, stride, padding = self.geom
        return (residual_norm(x, self.y, self.D, N, stride, padding) - self.res,
                orthogonality(x, self.y, self.D, N, stride, padding))

    def bounds(self, precision):
        eps = float(np.finfo(self.dtype(precision)).eps)
        xc = self.cpu(precision)[0]
        keep = self.keep(precision)
        coef = float(np.max(np.abs(xc.astype(self.x.dtype) - self.x)[keep], initial=0.0)) / float(np.max(np.abs(self.x)))
        res, orth = self.metrics(xc)
        floor = 64 * eps
        return max(4 * coef, floor), max(4 * float(orth.max()), floor), max(4 * float(res.max()), floor)


# (case, cplx) -> seed where that of tm_pursuit_ref.case_problem leaves out more than MAX_LEFT_OUT of the signals by
# this reference's own margins (none does: at most 3.1 % in single precision, with n and with tol)
SEEDS = {}


@functools.lru_cache(maxsize=None)
def case_problem(case, cplx):
    if (case, cplx) in SEEDS:
        return mp.make_problem(SEEDS[(case, cplx)], *CASES[case], cplx)[:2]
    return mp.case_problem(case, cplx)


def case_tol(case, cplx):
    y, _ = case_problem(case, cplx)
    return 0.02 * float(np.median(np.sum(np.abs(y) ** 2, axis=1)))


@functools.lru_cache(maxsize=None)
def case_analysis(case, cplx, with_tol):
    """n = nev; with tol the step limit is left at its default, min(T C, cap).  Asserts the share of signals the
    reference's own margins leave out."""
    B, T, S, N, stride, padding, nev = CASES[case]
    y, D = case_problem(case, cplx)
    if with_tol:
        an = Analysis(y, D, (N, stride, padding), tol=case_tol(case, cplx))
    else:
        an = Analysis(y, D, (N, stride, padding), n=nev)
    for precision in ('single', 'double'):
        assert an.left_out(precision) <= MAX_LEFT_OUT, (case, cplx, with_tol, precision, an.left_out(precision))
    return an


def edge_problem(cplx, B=2):
    """(y, D, (N, stride, padding), x0): noiseless events on the truncated atoms c = 1 and c = C - 2 and on the inside
    atom c = 4, which overlaps the first."""
    rng = np.random.RandomState(17)
    N, S = 30, 5
    D = rng.randn(1, S) + (1j * rng.randn(1, S) if cplx else 0)
    C = otm.geometry(S, N, 1, 'SAME')[0]
    inside = mp.inside_atoms(S, N, 1, 'SAME')
    assert 1 not in inside and C - 2 not in inside and 4 in inside
    x0 = np.zeros((B, 1, C))
    x0[:, 0, 1] = [2.0, -1.5][:B]
    x0[:, 0, 4] = [-1.0, 2.5][:B]
    x0[:, 0, C - 2] = [1.5, 1.0][:B]
    y = predict(x0.astype(D.dtype), D, N, 1, 'SAME')
    y, D = omp_ref.single_exact(y, D)
    return y, D, (N, 1, 'SAME'), x0


@functools.lru_cache(maxsize=None)
def problem_analysis(seed, B, T, S, N, stride, padding, nev, cplx, with_tol=False):
    """An Analysis of make_problem(seed, ...) with n = nev (or tol = 0.02 median |y|^2)."""
    y, D, _ = mp.make_problem(seed, B, T, S, N, stride, padding, nev, cplx)
    if with_tol:
        return Analysis(y, D, (N, stride, padding), tol=0.02 * float(np.median(np.sum(np.abs(y) ** 2, axis=1))))
    return Analysis(y, D, (N, stride, padding), n=nev)
