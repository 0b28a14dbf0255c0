"""NumPy references for convolutional matching pursuit (decomp_amd.template_matching.pursuit,
decomp_amd/csrc/template_pursuit.hpp) and the problems its tests share.  Test infrastructure only.

The algorithm, for one signal y [N] and templates D [T, S], with A[(t, c), n] = D[t, n - s c + Q],
rho2[t, c] = sum_n |A[(t, c), n]|^2 over the taps inside [0, N), r = y, E = |y|^2, x = 0, at most n times:
  1. tol given and E <= tol: stop
  2. alpha[t, c] = sum_n r[n] conj(A[(t, c), n]); score = |alpha|^2 / rho2 over the atoms with rho2 > 0 (positive:
     over the atoms with alpha > 0); the lowest flat index t C + c attaining the maximum; maximum not > 0: stop
  3. a = alpha* / rho2*, x[t*, c*] += a, E -= |alpha*|^2 / rho2*, r -= a A*
mp_residual recomputes alpha from r at every step; mp_gram keeps it up to date through the lag correlations, as the
kernel does.
"""
import functools

import numpy as np

from oracle import template_matching as otm
from omp_ref import single_exact, precision_dtype

DELTA = {'single': 1e-4, 'double': 1e-8}
RESID_DELTA = 1e-4
MAX_LEFT_OUT = 0.10


def _windows(S, N, stride, padding):
    """(C, base [C], valid [C, S]): atom c covers the samples base[c] + k, valid where they lie inside [0, N)."""
    C, Q = otm.geometry(S, N, stride, padding)
    base = stride * np.arange(C) - Q
    n = base[:, None] + np.arange(S)[None, :]
    return C, base, (n >= 0) & (n < N)


def inside_atoms(S, N, stride, padding):
    """The c whose taps lie entirely inside the signal."""
    _, _, valid = _windows(S, N, stride, padding)
    return np.flatnonzero(valid.all(axis=1))


def predict(x, D, N, stride, padding):
    """x * D without the dense operator: x [B, T, C] -> [B, N] (oracle.template_matching.predict, scattered tap by tap)."""
    T, S = D.shape
    C, base, valid = _windows(S, N, stride, padding)
    out = np.zeros((x.shape[0], N), dtype=np.result_type(x.dtype, D.dtype))
    for k in range(S):
        c = np.flatnonzero(valid[:, k])                          # base[c] + k: distinct samples
        out[:, base[c] + k] += np.tensordot(x[:, :, c], D[:, k], axes=(1, 0))
    return out


def mp_residual(y, D, N, stride, padding, n=None, tol=None, positive=False, energy=False):
    """The algorithm with alpha recomputed from the residual at every step, in double.  y [B, N].
    Returns (x [B, T, C], steps [B], margin [B], resid_margin [B]) (and E [B] after the loop with energy=True):
    margin is the smallest (c_(1) - max(c_(2), 0)) / |y| over the signal's steps, c = |alpha| / rho the best and the
    second-best score; resid_margin the smallest |E - tol| / |y|^2 (inf without tol)."""
    cplx = np.iscomplexobj(D) or np.iscomplexobj(y)
    dt = np.complex128 if cplx else np.float64
    y = np.asarray(y, dtype=dt)
    D = np.asarray(D, dtype=dt)
    T, S = D.shape
    B = y.shape[0]
    C, base, valid = _windows(S, N, stride, padding)
    K = T * C
    n = K if n is None else n
    idx = S + base[:, None] + np.arange(S)[None, :]            # into the residual padded by S zeros on both sides
    rho2 = (np.abs(D) ** 2) @ valid.T.astype(np.float64)        # [T, C]
    rho = np.sqrt(rho2)
    Dc = np.conj(D)
    x = np.zeros((B, T, C), dtype=dt)
    steps = np.zeros(B, dtype=np.int64)
    margin = np.full(B, np.inf)
    rmargin = np.full(B, np.inf)
    Eout = np.zeros(B)
    for b in range(B):
        rp = np.zeros(N + 2 * S, dtype=dt)
        rp[S:S + N] = y[b]
        yn2 = float(np.sum(np.abs(y[b]) ** 2))
        E = yn2
        for _ in range(n):
            if tol is not None:
                if yn2 > 0:
                    rmargin[b] = min(rmargin[b], abs(E - tol) / yn2)
                if E <= tol:
                    break
            alpha = (rp[idx] @ Dc.T).T                          # [T, C]
            ok = rho2 > 0
            if positive:
                ok = ok & (alpha.real > 0)
            score = np.where(ok, np.abs(alpha) ** 2 / np.where(rho2 > 0, rho2, 1.0), -1.0).ravel()
            i = int(np.argmax(score))                           # the first maximum: the lowest flat index
            if not score[i] > 0:
                break
            c = np.where(ok, np.abs(alpha) / np.where(rho2 > 0, rho, 1.0), -1.0).ravel()
            second = np.partition(c, K - 2)[K - 2] if K > 1 else 0.0
            if yn2 > 0:
                margin[b] = min(margin[b], (c[i] - max(second, 0.0)) / np.sqrt(yn2))
            t, cc = divmod(i, C)
            a = alpha[t, cc] / rho2[t, cc]
            x[b, t, cc] += a
            E -= score[i]
            v = valid[cc]
            rp[idx[cc, v]] -= a * D[t, v]
            steps[b] += 1
        Eout[b] = E
    out = (x, steps, margin, rmargin)
    return out + (Eout,) if energy else out


def _fold(terms):
    """Left-to-right sum of the rows of ``terms`` in their dtype."""
    acc = np.zeros(terms.shape[1:], dtype=terms.dtype)
    for row in terms:
        acc = acc + row
    return acc


def mp_gram(y, D, N, stride, padding, n=None, tol=None, positive=False):
    """The same algorithm in Gram-update form, in whatever dtype it is given: alpha0 = y A^H once, then
    alpha[t', c'] -= a G over the atoms within dh of the taken one, G from the lag correlations
    Corr[t, t', m] = sum_k D[t, k] conj(D[t', k + m]) when the taken atom lies inside the signal, else the explicit
    sum over the overlap inside [0, N).  Returns (x, steps)."""
    dt = y.dtype
    rt = np.zeros(1, dtype=dt).real.dtype
    T, S = D.shape
    B = y.shape[0]
    C, base, valid = _windows(S, N, stride, padding)
    K = T * C
    n = K if n is None else n
    dh = (S - 1) // stride
    Dc = np.conj(D)
    idx = S + base[:, None] + np.arange(S)[None, :]
    rho2 = _fold(np.stack([np.where(valid[None, :, k], (np.abs(D[:, k]) ** 2).astype(rt)[:, None], rt.type(0))
                           for k in range(S)]))                  # [T, C]
    corr = np.zeros((T, T, 2 * S - 1), dtype=dt)
    for m in range(-(S - 1), S):
        k0, k1 = max(0, -m), min(S - 1, S - 1 - m)
        corr[:, :, m + S - 1] = _fold(np.stack([np.outer(D[:, k], Dc[:, k + m]) for k in range(k0, k1 + 1)]))
    safe = np.where(rho2 > 0, rho2, rt.type(1))
    x = np.zeros((B, T, C), dtype=dt)
    steps = np.zeros(B, dtype=np.int64)
    tol_t = None if tol is None else rt.type(tol)
    for b in range(B):
        yp = np.zeros(N + 2 * S, dtype=dt)
        yp[S:S + N] = y[b]
        alpha = _fold(np.stack([np.outer(Dc[:, k], yp[idx[:, k]]) for k in range(S)]))    # [T, C]
        E = rt.type(np.sum((np.abs(y[b]) ** 2).astype(rt)))
        for _ in range(n):
            if tol_t is not None and E <= tol_t:
                break
            ok = rho2 > 0
            if positive:
                ok = ok & (alpha.real > 0)
            score = np.where(ok, (alpha.real * alpha.real + alpha.imag * alpha.imag) / safe, rt.type(-1)).ravel()
            i = int(np.argmax(score))
            if not score[i] > 0:
                break
            t, cc = divmod(i, C)
            a = dt.type(alpha[t, cc] / rho2[t, cc])
            x[b, t, cc] += a
            E = rt.type(E - score[i])
            ca, cb = max(cc - dh, 0), min(cc + dh, C - 1)
            cps = np.arange(ca, cb + 1)
            ms = stride * (cc - cps)
            if valid[cc].all():
                G = corr[t][:, ms + S - 1]                       # [T, nc]
            else:
                G = np.zeros((T, len(cps)), dtype=dt)
                for j, m in enumerate(ms):
                    ks = [k for k in range(max(0, -m), min(S - 1, S - 1 - m) + 1) if valid[cc, k]]
                    if ks:
                        G[:, j] = _fold(np.stack([D[t, k] * Dc[:, k + m] for k in ks]))
            alpha[:, ca:cb + 1] = alpha[:, ca:cb + 1] - a * G
            steps[b] += 1
    return x, steps


def mp_dense(y, A, n):
    """Plain matching pursuit on a dense operator A [K, N] in double: (x [B, K], steps)."""
    rho2 = np.sum(np.abs(A) ** 2, axis=1)
    x = np.zeros((y.shape[0], A.shape[0]), dtype=A.dtype)
    steps = np.zeros(y.shape[0], dtype=np.int64)
    for b in range(y.shape[0]):
        r = y[b].astype(A.dtype)
        for _ in range(n):
            alpha = A.conj() @ r
            score = np.where(rho2 > 0, np.abs(alpha) ** 2 / np.where(rho2 > 0, rho2, 1.0), -1.0)
            i = int(np.argmax(score))
            if not score[i] > 0:
                break
            a = alpha[i] / rho2[i]
            x[b, i] += a
            r = r - a * A[i]
            steps[b] += 1
    return x, steps


# ---- the shared problems ----------------------------------------------------------------------------------------
def make_problem(seed, B, T, S, N, stride, padding, nev, cplx, noise=0.05, signs=True):
    """Templates randn(T, S) (0.5 + rand(T, 1)) (+ 1j randn); per signal nev planted events on atoms whose taps lie
    entirely inside the signal (the outermost atoms of 'SAME' have one tap and are parallel across templates: an exact
    tie), amplitudes 1 + permutation(nev) / nev with random signs; noise 0.05 |y| / sqrt(N); single-exact entries.
    Returns (y [B, N], D, x0 [B, T, C])."""
    rng = np.random.RandomState(seed)
    D = rng.randn(T, S) * (0.5 + rng.rand(T, 1))
    if cplx:
        D = D + 1j * rng.randn(T, S)
    C, _ = otm.geometry(S, N, stride, padding)
    inside = inside_atoms(S, N, stride, padding)
    x0 = np.zeros((B, T, C))
    for b in range(B):
        pick = rng.choice(T * len(inside), nev, replace=False)
        amp = 1 + rng.permutation(nev) / nev
        if signs:
            amp = amp * rng.choice([-1, 1], nev)
        x0[b, pick // len(inside), inside[pick % len(inside)]] = amp
    y = predict(x0.astype(D.dtype), D, N, stride, padding)
    e = rng.randn(B, N)
    if cplx:
        e = e + 1j * rng.randn(B, N)
    y = y + noise * np.linalg.norm(y, axis=1, keepdims=True) / np.sqrt(N) * e
    y, D = single_exact(y, D)
    return y, D, x0


# (B, T, S, N, stride, padding, nev)
CASES = {
    0: (64, 2, 5, 40, 1, 'SAME', 4),         # events overlap: the Gram update and re-selection
    1: (64, 3, 8, 64, 1, 'VALID', 5),
    2: (64, 2, 9, 130, 2, 'SAME', 6),        # stride 2
    3: (32, 2, 4, 100, 6, 'SAME', 6),        # stride > S: dh = 0
    4: (64, 3, 16, 16, 1, 'VALID', 1),       # C = 1
    5: (32, 1, 1, 70, 1, 'SAME', 5),         # S = 1
    6: (32, 3, 17, 700, 1, 'SAME', 8),       # T C past 2048
    7: (32, 2, 33, 3001, 3, 'SAME', 10),
    8: (32, 4, 33, 5000, 1, 'SAME', 12),     # T C ~ 20 000
}
# (case, cplx) -> seed where the default (100 + case) leaves out more than MAX_LEFT_OUT of the signals by the
# reference's own margins (case 8, real, tol run: 15.6 % in single precision)
SEEDS = {(8, False): 200}


def residual_norm(x, y, D, N, stride, padding):
    """|y - predict(x)| / |y| per signal, in double."""
    r = y - predict(np.asarray(x).astype(y.dtype), D, N, stride, padding)
    yn = np.linalg.norm(y, axis=1)
    return np.linalg.norm(r, axis=1) / np.where(yn > 0, yn, 1.0)


class Analysis(object):
    """For a double problem (y, D) with single-exact entries: the double reference (x, steps, margin, resid_margin),
    keep(precision), cpu(precision) = mp_gram in that dtype, and bounds(precision) = (coefficient, residual) bounds
    for the GPU result: 4 x what cpu(precision) shows against the double reference (the factor covers the fused
    multiply-adds and the other summation order of the kernel), floor 64 eps; coefficients over the compared signals
    relative to max|x_ref|, residuals over every signal relative to |y|."""

    def __init__(self, y, D, geom, n=None, tol=None, positive=False):
        self.y, self.D, self.geom, self.n, self.tol, self.positive = y, D, geom, n, tol, positive
        self.cplx = np.iscomplexobj(D)
        N, stride, padding = geom
        self.x, self.steps, self.margin, self.resid_margin = mp_residual(y, D, N, stride, padding, n, tol, positive)
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

    def cpu(self, precision):
        if precision not in self._cpu:
            dt = self.dtype(precision)
            N, stride, padding = self.geom
            self._cpu[precision] = mp_gram(self.y.astype(dt), self.D.astype(dt), N, stride, padding, self.n, self.tol,
                                           self.positive)
        return self._cpu[precision]

    def bounds(self, precision):
        eps = float(np.finfo(self.dtype(precision)).eps)
        xc = self.cpu(precision)[0]
        keep = self.keep(precision)
        N, stride, padding = self.geom
        coef = float(np.max(np.abs(xc.astype(self.x.dtype) - self.x)[keep], initial=0.0)) / float(np.max(np.abs(self.x)))
        res = float(np.max(residual_norm(xc, self.y, self.D, N, stride, padding) - self.res))
        return max(4 * coef, 64 * eps), max(4 * res, 64 * eps)


@functools.lru_cache(maxsize=None)
def case_problem(case, cplx):
    B, T, S, N, stride, padding, nev = CASES[case]
    seed = SEEDS.get((case, cplx), 100 + case)
    return make_problem(seed, B, T, S, N, stride, padding, nev, cplx)[:2]


def case_tol(case, cplx):
    y, _ = case_problem(case, cplx)
    return 0.02 * float(np.median(np.sum(np.abs(y) ** 2, axis=1)))


@functools.lru_cache(maxsize=None)
def case_analysis(case, cplx, with_tol):
    """n = nev; with tol the step limit is left at its default, T C."""
    B, T, S, N, stride, padding, nev = CASES[case]
    y, D = case_problem(case, cplx)
    if with_tol:
        return Analysis(y, D, (N, stride, padding), tol=case_tol(case, cplx))
    return Analysis(y, D, (N, stride, padding), n=nev)
