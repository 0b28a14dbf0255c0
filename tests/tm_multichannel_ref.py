"""NumPy references for the greedy coders on multichannel templates (decomp_amd.template_matching.pursuit /
orthogonal_pursuit / predict with D [T, Ch, S], decomp_amd/csrc/template_multichannel.hpp) and the problems their tests
share.  Test infrastructure only.

The model: y[b, ch, n] ~ sum_(t, c) x[b, t, c] D[t, ch, n - s c + Q]; the atom of (t, c) is
A[(t, c), (ch, n)] = D[t, ch, n - s c + Q], rho2[t, c] = sum_ch sum_n |A|^2 over the taps inside [0, N), E = |y_b|^2 over
all channels.  The steps are those of tm_pursuit_ref (matching pursuit) and tm_omp_ref (orthogonal pursuit) with every
correlation summed over the channels; the functions here are written for D [T, Ch, S] directly and at Ch = 1 do the
arithmetic of those two files operation for operation.
"""
import functools

import numpy as np

import omp_ref
import tm_pursuit_ref as mp
import tm_omp_ref as op
from oracle import template_matching as otm
from omp_ref import precision_dtype, eps_dep, single_exact
from tm_pursuit_ref import _windows, _fold, DELTA, RESID_DELTA, MAX_LEFT_OUT, inside_atoms

__all__ = ['DELTA', 'RESID_DELTA', 'MAX_LEFT_OUT', 'inside_atoms', 'single_exact']


# ---- the channel-interleaved one-channel problem ('VALID' only) -----------------------------------------------------
def interleave(y, D):
    """y [B, Ch, N], D [T, Ch, S] -> y' [B, N Ch], D' [T, S Ch] with y'[n Ch + ch] = y[ch, n], D'[t, k Ch + ch] =
    D[t, ch, k]: with 'VALID' and stride Ch the one-channel problem on (y', D') is this one."""
    return (np.ascontiguousarray(np.swapaxes(y, -1, -2)).reshape(y.shape[:-2] + (-1,)),
            np.ascontiguousarray(np.swapaxes(D, -1, -2)).reshape(D.shape[0], -1))


def deinterleave(y, D, Ch):
    """The inverse of interleave."""
    return (np.ascontiguousarray(np.swapaxes(y.reshape(y.shape[:-1] + (-1, Ch)), -1, -2)),
            np.ascontiguousarray(np.swapaxes(D.reshape(D.shape[0], -1, Ch), -1, -2)))


# ---- operator -----------------------------------------------------------------------------------------------------
def predict(x, D, N, stride, padding):
    """x [B, T, C], D [T, Ch, S] -> [B, Ch, N]."""
    return np.stack([mp.predict(x, D[:, ch], N, stride, padding) for ch in range(D.shape[1])], axis=1)


def correlate(r, D, N, stride, padding):
    """r A^H: r [B, Ch, N] -> [B, T, C], in double."""
    return sum(op.correlate(r[:, ch], D[:, ch], N, stride, padding) for ch in range(D.shape[1]))


def rho2_of(D, valid):
    return sum((np.abs(D[:, ch]) ** 2) @ valid.T.astype(np.float64) for ch in range(D.shape[1]))    # [T, C]


def dense_operator(D, N, stride, padding):
    """A [T C, Ch N], built entry by entry."""
    T, Ch, S = D.shape
    C, base, valid = _windows(S, N, stride, padding)
    A = np.zeros((T * C, Ch * N), dtype=D.dtype)
    for t in range(T):
        for c in range(C):
            for ch in range(Ch):
                for k in range(S):
                    if valid[c, k]:
                        A[t * C + c, ch * N + base[c] + k] = D[t, ch, k]
    return A


def residual_norm(x, y, D, N, stride, padding):
    """|y - predict(x)| / |y| per signal over all channels, in double."""
    r = (y - predict(np.asarray(x).astype(y.dtype), D, N, stride, padding)).reshape(y.shape[0], -1)
    yn = np.linalg.norm(y.reshape(y.shape[0], -1), axis=1)
    return np.linalg.norm(r, axis=1) / np.where(yn > 0, yn, 1.0)


def orthogonality(x, y, D, N, stride, padding):
    """max over the support (x != 0) of |r . A_j^H| / (rho_j |y|) per signal, r = y - x * D, in double."""
    x = np.asarray(x).astype(y.dtype)
    _, _, valid = _windows(D.shape[-1], N, stride, padding)
    rho = np.sqrt(rho2_of(D, valid))
    r = y - predict(x, D, N, stride, padding)
    a = np.abs(correlate(r, D, N, stride, padding)) / np.where(rho > 0, rho, 1.0)[None]
    yn = np.linalg.norm(y.reshape(y.shape[0], -1), axis=1)
    return np.where(x != 0, a, 0.0).reshape(x.shape[0], -1).max(axis=1) / np.where(yn > 0, yn, 1.0)


def _double(y, D):
    cplx = np.iscomplexobj(D) or np.iscomplexobj(y)
    dt = np.complex128 if cplx else np.float64
    return np.asarray(y, dtype=dt), np.asarray(D, dtype=dt), dt, cplx


def _alpha(rp, idx, Dc):
    """sum_ch (rp[ch][idx] @ Dc[:, ch].T).T: [T, C]."""
    acc = np.zeros((Dc.shape[0], idx.shape[0]), dtype=Dc.dtype)
    for ch in range(Dc.shape[1]):
        acc = acc + (rp[ch][idx] @ Dc[:, ch].T).T
    return acc


# ---- residual forms, in double -----------------------------------------------------------------------------------
def mp_residual(y, D, N, stride, padding, n=None, tol=None, positive=False):
    """tm_pursuit_ref.mp_residual for y [B, Ch, N], D [T, Ch, S]: (x [B, T, C], steps, margin, resid_margin)."""
    y, D, dt, _ = _double(y, D)
    T, Ch, S = D.shape
    B = y.shape[0]
    C, base, valid = _windows(S, N, stride, padding)
    K = T * C
    n = K if n is None else n
    idx = S + base[:, None] + np.arange(S)[None, :]
    rho2 = rho2_of(D, valid)
    rho = np.sqrt(rho2)
    Dc = np.conj(D)
    x = np.zeros((B, T, C), dtype=dt)
    steps = np.zeros(B, dtype=np.int64)
    margin = np.full(B, np.inf)
    rmargin = np.full(B, np.inf)
    for b in range(B):
        rp = np.zeros((Ch, N + 2 * S), dtype=dt)
        rp[:, S:S + N] = y[b]
        yn2 = float(np.sum(np.abs(y[b]) ** 2))
        E = yn2
        for _ in range(n):
            if tol is not None:
                if yn2 > 0:
                    rmargin[b] = min(rmargin[b], abs(E - tol) / yn2)
                if E <= tol:
                    break
            alpha = _alpha(rp, idx, Dc)
            ok = rho2 > 0
            if positive:
                ok = ok & (alpha.real > 0)
            score = np.where(ok, np.abs(alpha) ** 2 / np.where(rho2 > 0, rho2, 1.0), -1.0).ravel()
            i = int(np.argmax(score))
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
            rp[:, idx[cc, v]] -= a * D[t][:, v]
            steps[b] += 1
    return x, steps, margin, rmargin


def _atom(D, N, base, valid, C, i):
    """Atom i = t C + c as a [Ch N] vector."""
    t, c = divmod(i, C)
    a = np.zeros((D.shape[1], N), dtype=D.dtype)
    v = valid[c]
    a[:, base[c] + np.flatnonzero(v)] = D[t][:, v]
    return a.ravel()


def omp_residual(y, D, N, stride, padding, n=None, tol=None, eps=None):
    """tm_omp_ref.omp_residual for y [B, Ch, N], D [T, Ch, S]: (x [B, T, C], steps, margin, resid_margin)."""
    y, D, dt, cplx = _double(y, D)
    T, Ch, S = D.shape
    B = y.shape[0]
    C, base, valid = _windows(S, N, stride, padding)
    K = T * C
    n = min(K, op.cap_of(cplx)) if n is None else n
    if eps is None:
        eps = eps_dep(dt)
    idx = S + base[:, None] + np.arange(S)[None, :]
    rho2 = rho2_of(D, valid)
    rho = np.sqrt(rho2).ravel()
    Dc = np.conj(D)
    x = np.zeros((B, K), dtype=dt)
    steps = np.zeros(B, dtype=np.int64)
    margin = np.full(B, np.inf)
    rmargin = np.full(B, np.inf)
    for b in range(B):
        yb = y[b].ravel()
        yn2 = float(np.sum(np.abs(yb) ** 2))
        I, L, atoms, coef, r = [], [], [], None, yb
        for _ in range(n):
            if tol is not None:
                E = float(np.sum(np.abs(r) ** 2))
                if yn2 > 0:
                    rmargin[b] = min(rmargin[b], abs(E - tol) / yn2)
                if E <= tol:
                    break
            rp = np.zeros((Ch, N + 2 * S), dtype=dt)
            rp[:, S:S + N] = r.reshape(Ch, N)
            alpha = _alpha(rp, idx, Dc).ravel()
            c = np.where(rho > 0, np.abs(alpha) / np.where(rho > 0, rho, 1.0), -1.0)
            c[I] = -1.0
            k = int(np.argmax(c))
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
            coef = np.linalg.lstsq(AI.T, yb, rcond=None)[0]
            r = yb - coef @ AI
        if I:
            x[b, I] = coef
        steps[b] = len(I)
    return x.reshape(B, T, C), steps, margin, rmargin


# ---- Gram forms, in the dtype given: every sum ch ascending, k ascending inside ---------------------------------------
class _Gram(object):
    """rho2, the lag correlations and the Gram rows of D [T, Ch, S] in D's dtype, summed as the kernels sum them."""

    def __init__(self, D, N, stride, padding):
        self.D, self.stride = D, stride
        dt = self.dt = D.dtype
        rt = self.rt = np.zeros(1, dtype=dt).real.dtype
        T, Ch, S = D.shape
        self.C, self.base, self.valid = _windows(S, N, stride, padding)
        valid = self.valid
        self.dh = (S - 1) // stride
        self.Dc = Dc = np.conj(D)
        self.idx = S + self.base[:, None] + np.arange(S)[None, :]
        self.rho2 = _fold(np.stack([np.where(valid[None, :, k], (np.abs(D[:, ch, k]) ** 2).astype(rt)[:, None], rt.type(0))
                                    for ch in range(Ch) for k in range(S)]))                 # [T, C]
        self.corr = np.zeros((T, T, 2 * S - 1), dtype=dt)
        for m in range(-(S - 1), S):
            k0, k1 = max(0, -m), min(S - 1, S - 1 - m)
            self.corr[:, :, m + S - 1] = _fold(np.stack([np.outer(D[:, ch, k], Dc[:, ch, k + m])
                                                         for ch in range(Ch) for k in range(k0, k1 + 1)]))
        self.inside = valid.all(axis=1)
        self.safe = np.where(self.rho2 > 0, self.rho2, rt.type(1))

    def alpha0(self, yb):
        """y_b A^H [T, C] for y_b [Ch, N]."""
        Ch, S = self.D.shape[1:]
        yp = np.zeros((Ch, yb.shape[1] + 2 * S), dtype=self.dt)
        yp[:, S:S + yb.shape[1]] = yb
        return _fold(np.stack([np.outer(self.Dc[:, ch, k], yp[ch, self.idx[:, k]]) for ch in range(Ch) for k in range(S)]))

    def row(self, t, cc, cps):
        """G[(t, cc), (:, cps)]: [T, len(cps)]."""
        D, Dc, S = self.D, self.Dc, self.D.shape[2]
        ms = self.stride * (cc - cps)
        if self.inside[cc]:
            return self.corr[t][:, ms + S - 1]
        G = np.zeros((D.shape[0], len(cps)), dtype=self.dt)
        for j, m in enumerate(ms):
            ks = [k for k in range(max(0, -m), min(S - 1, S - 1 - m) + 1) if self.valid[cc, k]]
            if ks:
                G[:, j] = _fold(np.stack([D[t, ch, k] * Dc[:, ch, k + m] for ch in range(D.shape[1]) for k in ks]))
        return G

    def entry(self, i, k):
        (t, cc), (tp, cp) = divmod(i, self.C), divmod(k, self.C)
        if abs(cc - cp) > self.dh:
            return self.dt.type(0)
        return self.row(t, cc, np.array([cp]))[tp, 0]

    def window(self, cc):
        return max(cc - self.dh, 0), min(cc + self.dh, self.C - 1)


def mp_gram(y, D, N, stride, padding, n=None, tol=None, positive=False):
    """tm_pursuit_ref.mp_gram for y [B, Ch, N], D [T, Ch, S] of one dtype: (x, steps)."""
    g = _Gram(D, N, stride, padding)
    dt, rt, C = g.dt, g.rt, g.C
    T, B = D.shape[0], y.shape[0]
    n = T * C if n is None else n
    x = np.zeros((B, T, C), dtype=dt)
    steps = np.zeros(B, dtype=np.int64)
    tol_t = None if tol is None else rt.type(tol)
    for b in range(B):
        alpha = g.alpha0(y[b])
        E = rt.type(np.sum((np.abs(y[b]) ** 2).astype(rt)))
        for _ in range(n):
            if tol_t is not None and E <= tol_t:
                break
            ok = g.rho2 > 0
            if positive:
                ok = ok & (alpha.real > 0)
            score = np.where(ok, (alpha.real * alpha.real + alpha.imag * alpha.imag) / g.safe, rt.type(-1)).ravel()
            i = int(np.argmax(score))
            if not score[i] > 0:
                break
            t, cc = divmod(i, C)
            a = dt.type(alpha[t, cc] / g.rho2[t, cc])
            x[b, t, cc] += a
            E = rt.type(E - score[i])
            ca, cb = g.window(cc)
            alpha[:, ca:cb + 1] = alpha[:, ca:cb + 1] - a * g.row(t, cc, np.arange(ca, cb + 1))
            steps[b] += 1
    return x, steps


def omp_gram(y, D, N, stride, padding, n=None, tol=None, eps=None):
    """tm_omp_ref.omp_gram for y [B, Ch, N], D [T, Ch, S] of one dtype: (x, steps)."""
    g = _Gram(D, N, stride, padding)
    dt, rt, C = g.dt, g.rt, g.C
    T, B = D.shape[0], y.shape[0]
    K = T * C
    n = min(K, op.cap_of(dt.kind == 'c')) if n is None else n
    eps = rt.type(eps_dep(dt) if eps is None else eps)
    x = np.zeros((B, K), dtype=dt)
    steps = np.zeros(B, dtype=np.int64)
    tol_t = None if tol is None else rt.type(tol)
    for b in range(B):
        alpha0 = g.alpha0(y[b])
        alpha = alpha0.copy()
        yn2 = rt.type(np.sum((np.abs(y[b]) ** 2).astype(rt)))
        E = yn2
        I, L, z = [], [], []
        xi = np.zeros(0, dtype=dt)
        for _ in range(n):
            if tol_t is not None and E <= tol_t:
                break
            score = np.where(g.rho2 > 0, (alpha.real * alpha.real + alpha.imag * alpha.imag) / g.safe, rt.type(-1)).ravel()
            score[I] = -1
            k = int(np.argmax(score))
            if not score[k] > 0:
                break
            gkk = g.rho2.ravel()[k]
            gcol = np.array([g.entry(i, k) for i in I], dtype=dt)
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
                if j != m_ - 1 and dx[j] == 0:
                    continue
                t, cc = divmod(i, C)
                ca, cb = g.window(cc)
                alpha[:, ca:cb + 1] = alpha[:, ca:cb + 1] - dx[j] * g.row(t, cc, np.arange(ca, cb + 1))
            E = rt.type(yn2 - np.sum(xi * np.conj(alpha0.ravel()[I])).real)
            steps[b] += 1
        if I:
            x[b, I] = xi
    return x.reshape(B, T, C), steps


# ---- what the GPU tests compare against (computed once per session, never modified) --------------------------------
class Analysis(object):
    """For a double problem (y [B, Ch, N], D [T, Ch, S]) with single-exact entries and coder 'mp' or 'omp': the double
    residual-form reference (x, steps, margin, resid_margin), keep(precision) by the rules of tm_pursuit_ref /
    tm_omp_ref (margin >= DELTA, in tol runs resid_margin >= RESID_DELTA), cpu(precision) = the Gram form in that
    dtype, and bounds(precision) = (coefficient, orthogonality, residual) bounds for the GPU result: 4 x what
    cpu(precision) shows against the double reference, floor 64 eps; coefficients over the compared signals relative
    to max|x_ref|, orthogonality (omp only, else None) and residual over every signal relative to |y|."""

    def __init__(self, coder, y, D, geom, n=None, tol=None, positive=False):
        assert coder in ('mp', 'omp') and not (positive and coder == 'omp')
        self.coder, self.y, self.D, self.geom, self.n, self.tol, self.positive = coder, y, D, geom, n, tol, positive
        self.cplx = np.iscomplexobj(D)
        N, stride, padding = geom
        if coder == 'mp':
            out = mp_residual(y, D, N, stride, padding, n, tol, positive)
        else:
            out = omp_residual(y, D, N, stride, padding, n, tol)
        self.x, self.steps, self.margin, self.resid_margin = out
        for a in out:
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
            if self.coder == 'mp':
                self._cpu[precision] = mp_gram(self.y.astype(dt), self.D.astype(dt), N, stride, padding, self.n,
                                               self.tol, self.positive)
            else:
                self._cpu[precision] = omp_gram(self.y.astype(dt), self.D.astype(dt), N, stride, padding, self.n,
                                                self.tol)
        return self._cpu[precision]

    def metrics(self, x):
        """(residual excess over the reference's, orthogonality) per signal of a result x, in double."""
        N, stride, padding = self.geom
        return (residual_norm(x, self.y, self.D, N, stride, padding) - self.res,
                orthogonality(x, self.y, self.D, N, stride, padding))

    def bounds(self, precision):
        floor = 64 * float(np.finfo(self.dtype(precision)).eps)
        xc = self.cpu(precision)[0]
        keep = self.keep(precision)
        coef = float(np.max(np.abs(xc.astype(self.x.dtype) - self.x)[keep], initial=0.0)) / float(np.max(np.abs(self.x)))
        res, orth = self.metrics(xc)
        return (max(4 * coef, floor), max(4 * float(orth.max()), floor) if self.coder == 'omp' else None,
                max(4 * float(res.max()), floor))


# ---- the shared problems ------------------------------------------------------------------------------------------
def make_problem(seed, B, T, Ch, S, N, stride, padding, nev, cplx, noise=0.05):
    """tm_pursuit_ref.make_problem with templates randn(T, Ch, S) (0.5 + rand(T, 1, 1)): events on atoms inside the
    signal, noise 0.05 |y| / sqrt(Ch N), single-exact entries.  Returns (y [B, Ch, N], D, x0 [B, T, C])."""
    rng = np.random.RandomState(seed)
    D = rng.randn(T, Ch, S) * (0.5 + rng.rand(T, 1, 1))
    if cplx:
        D = D + 1j * rng.randn(T, Ch, S)
    C, _ = otm.geometry(S, N, stride, padding)
    inside = inside_atoms(S, N, stride, padding)
    x0 = np.zeros((B, T, C))
    for b in range(B):
        pick = rng.choice(T * len(inside), nev, replace=False)
        amp = (1 + rng.permutation(nev) / nev) * rng.choice([-1, 1], nev)
        x0[b, pick // len(inside), inside[pick % len(inside)]] = amp
    y = predict(x0.astype(D.dtype), D, N, stride, padding)
    e = rng.randn(B, Ch, N)
    if cplx:
        e = e + 1j * rng.randn(B, Ch, N)
    y = y + noise * np.linalg.norm(y.reshape(B, -1), axis=1)[:, None, None] / np.sqrt(Ch * N) * e
    y, D = single_exact(y, D)
    return y, D, x0


# (B, T, Ch, S, N, stride, padding, nev)
CASES = {
    0: (32, 2, 3, 5, 40, 1, 'VALID', 4),
    1: (32, 3, 4, 8, 64, 2, 'VALID', 5),
    2: (16, 5, 2, 7, 300, 1, 'VALID', 6),      # C = 294: two c tiles
    3: (16, 9, 7, 4, 90, 3, 'VALID', 5),
    4: (16, 1, 16, 9, 530, 1, 'VALID', 8),
    5: (32, 3, 5, 16, 16, 1, 'VALID', 1),      # C = 1
    6: (32, 2, 3, 5, 40, 1, 'SAME', 4),
    7: (32, 3, 4, 8, 64, 2, 'SAME', 5),
    8: (16, 5, 2, 7, 300, 1, 'SAME', 6),       # C = 306: two c tiles
    9: (16, 9, 7, 4, 90, 6, 'SAME', 5),        # stride > S: dh = 0
}
VALID_CASES = [c for c in sorted(CASES) if CASES[c][6] == 'VALID']
# (case, cplx) -> the seed of make_problem for a 'SAME' case where the default (400 + case) leaves out more than
# MAX_LEFT_OUT of the signals by either coder's margins (none does: at most 3.1 %, case 6 with tol, in both precisions;
# the 'VALID' cases leave out none; test_tm_multichannel_ref_host.py asserts both)
SEEDS = {}


@functools.lru_cache(maxsize=None)
def case_problem(case, cplx):
    """(y [B, Ch, N], D [T, Ch, S]) in double.  'VALID': tm_pursuit_ref.make_problem(300 + case, ...) on the
    interleaved sizes (N Ch, S Ch, stride Ch), de-interleaved."""
    B, T, Ch, S, N, stride, padding, nev = CASES[case]
    if padding == 'VALID':
        y1, D1, _ = mp.make_problem(300 + case, B, T, S * Ch, N * Ch, stride * Ch, 'VALID', nev, cplx)
        y, D = deinterleave(y1, D1, Ch)
    else:
        y, D, _ = make_problem(SEEDS.get((case, cplx), 400 + case), B, T, Ch, S, N, stride, padding, nev, cplx)
    y.setflags(write=False)
    D.setflags(write=False)
    return y, D


def case_tol(case, cplx):
    y, _ = case_problem(case, cplx)
    return 0.02 * float(np.median(np.sum(np.abs(y.reshape(y.shape[0], -1)) ** 2, axis=1)))


@functools.lru_cache(maxsize=None)
def case_analysis(coder, case, cplx, with_tol):
    """n = nev; with tol the step limit is left at its default (T C, or min(T C, cap) for omp)."""
    B, T, Ch, S, N, stride, padding, nev = CASES[case]
    y, D = case_problem(case, cplx)
    if with_tol:
        return Analysis(coder, y, D, (N, stride, padding), tol=case_tol(case, cplx))
    return Analysis(coder, y, D, (N, stride, padding), n=nev)


def edge_problem(cplx, Ch=3, B=2):
    """tm_omp_ref.edge_problem with Ch channels: noiseless events on the truncated atoms c = 1 and c = C - 2 and on the
    inside atom c = 4, which overlaps the first.  (y, D, (N, stride, padding), x0)."""
    rng = np.random.RandomState(17)
    N, S = 30, 5
    D = rng.randn(1, Ch, S) + (1j * rng.randn(1, Ch, S) if cplx else 0)
    C = otm.geometry(S, N, 1, 'SAME')[0]
    inside = inside_atoms(S, N, 1, 'SAME')
    assert 1 not in inside and C - 2 not in inside and 4 in inside
    x0 = np.zeros((B, 1, C))
    x0[:, 0, 1] = [2.0, -1.5][:B]
    x0[:, 0, 4] = [-1.0, 2.5][:B]
    x0[:, 0, C - 2] = [1.5, 1.0][:B]
    y = predict(x0.astype(D.dtype), D, N, 1, 'SAME')
    y, D = single_exact(y, D)
    return y, D, (N, 1, 'SAME'), x0


def tier_problem(K, cplx):
    """One template of S = 3 taps on Ch = 2 channels with T C = K ('SAME', stride 1), B = 2 signals of 5 events:
    (y, D, (N, stride, padding)), for the tiers of the step kernels."""
    N = K - 2
    assert otm.geometry(3, N, 1, 'SAME')[0] == K
    y, D, _ = make_problem(K % 1000, 2, 1, 2, 3, N, 1, 'SAME', 5, cplx)
    return y, D, (N, 1, 'SAME')
