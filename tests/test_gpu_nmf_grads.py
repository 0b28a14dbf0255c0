"""GPU: the building blocks of the stochastic NMF methods and of the public gradient helpers, called directly and
compared elementwise with float64 NumPy, at shapes that leave the single tile of the fixtures' shapes.

  dcp_nmf_grads_*    n_x_updates in-place x updates, then the two parts of the D gradient
  dcp_nmf_apply_*    D_new = l2_strict(rule(D, P, Q)) and max|D - D_new|
  dcp_axpby_*        y = a x + b y
  dcp_mu_quotient_*  cur o max(pos, 0) / max(neg, 1e-15)
  Gaussian / Poisson / BetaDivergence .grad_x / .grad_d, Gaussian.logp

Error bounds.  Every product here sums d positive terms.  Rounded in a working precision with unit roundoff u,
such a sum is within lambda * sqrt(d) * u of its value, relative (the probabilistic bound of Higham & Mary,
"A new approach to probabilistic rounding error analysis", 2019), for a small lambda; this file takes lambda = 2.
The largest error measured on these products so far is 0.17 sqrt(d) u (65536-deep statistics product,
test_gpu_bf16x6_paths.py), and the split-bf16 core's error is of the fp32 core's size.  With P(d) = 2 sqrt(d) u:
  - one x update is a quotient of two parts, each at most a forward product (depth K, raised to a power of at most
    2 by the beta parts) followed by a reduction (depth F): at most 6 P(max(F, K)) + 4 u;
  - an error e in x enters the next update's output at most twice over (x and its negative part), so n updates
    stay within (2^n - 1) times one update's bound;
  - the D-side parts, formed from the kernel's own X_out, are one forward product and one reduction over the N rows
    (l2 without a mask: x^T x, then (x^T x) D): 3 P(max(N, F, K)) + 4 u.
The same formula with u = 2^-53 gives the float64 bounds (all below 1e-11 here)."""
import ctypes

import numpy as np
import pytest

from oracle import nmf as onmf
from oracle.common import l2_strict

pytestmark = pytest.mark.gpu

U = {np.float32: 2.0 ** -24, np.float64: 2.0 ** -53}
LAMBDA = 2.0


def _P(dt, d):
    return LAMBDA * np.sqrt(max(int(d), 1)) * U[dt]


def _x_bound(dt, F, K, n):
    return (2 ** n - 1) * (6 * _P(dt, max(F, K)) + 4 * U[dt])


def _d_bound(dt, N, F, K):
    return 3 * _P(dt, max(N, F, K)) + 4 * U[dt]


def _rel(got, ref):
    got = np.asarray(got, np.float64)
    ref = np.asarray(ref, np.float64)
    return float(np.max(np.abs(got - ref) / np.maximum(np.abs(ref), 1e-300)))


def _lib_h(t):
    from decomp_amd import _arrays
    return _arrays.lib_handle(t)


def _dev(a):
    import torch
    return torch.from_numpy(np.ascontiguousarray(a)).cuda()


class _Mode:
    """dcp_set_f32_product_mode for the duration of a block."""

    def __init__(self, mode):
        self.mode = mode

    def __enter__(self):
        import torch
        lib, h = _lib_h(torch.empty(1, device='cuda'))
        self.prev = lib.dcp_set_f32_product_mode(h, self.mode)
        assert self.prev in (0, 1)

    def __exit__(self, *exc):
        import torch
        lib, h = _lib_h(torch.empty(1, device='cuda'))
        lib.dcp_set_f32_product_mode(h, self.prev)


# likelihood name -> (kernel code, beta, oracle spec)
LIKS = {'l2': (0, None, 'l2'), 'kl': (1, None, 'kl'), 'is': (2, 0.0, 0.0), 'b0.5': (2, 0.5, 0.5)}


def _grads(Y, M, X, D, lik, nx):
    """(X_out, gpos, gneg) of one dcp_nmf_grads_* call (X itself is left alone)."""
    import torch
    from decomp_amd import _arrays, _hip
    from decomp_amd.nmf_methods.grads import set_beta
    code, beta, _ = LIKS[lik]
    y, d = _dev(Y), _dev(D)
    m = None if M is None else _dev(M)
    x = _dev(X.copy())
    K, F = D.shape
    gp, gn = torch.empty_like(d), torch.empty_like(d)
    lib, h = _lib_h(y)
    set_beta(h, code, beta)
    fn = getattr(lib, 'dcp_nmf_grads_' + _arrays.suffix(y))
    _hip.check(h, fn(h, _arrays.ptr(y), _arrays.ptr(m), _arrays.ptr(x), _arrays.ptr(d), Y.shape[0], F, K, code,
                     nx, _arrays.ptr(gp), _arrays.ptr(gn)), 'dcp_nmf_grads')
    torch.cuda.synchronize()
    return x.cpu().numpy(), gp.cpu().numpy(), gn.cpu().numpy()


def _data(N, F, K, masked, seed):
    """Positive float32-representable inputs (float64 copies are exact); D rows of unit norm, as in the loop."""
    rng = np.random.RandomState(seed)
    Y = rng.uniform(0.1, 1.0, (N, F)).astype(np.float32)
    D = rng.uniform(0.1, 1.0, (K, F))
    D = (D / np.sqrt(np.sum(D * D, axis=1, keepdims=True))).astype(np.float32)
    X = rng.uniform(0.1, 1.0, (N, K)).astype(np.float32)
    M = (rng.uniform(size=(N, F)) >= 0.3).astype(np.float32) if masked else None
    if M is not None:
        M[:, 0] = 1.0                      # no all-zero mask row: every x part stays positive
    return Y, M, X, D


def _x_ref(Y, M, X, D, spec, nx):
    y, x, d = (a.astype(np.float64) for a in (Y, X, D))
    m = None if M is None else M.astype(np.float64)
    for _ in range(nx):
        x = onmf.update_x(y, x, d, m, spec)
    return x


def _d_ref(Y, M, Xo, D, spec):
    y, x, d = (a.astype(np.float64) for a in (Y, Xo, D))
    m = None if M is None else M.astype(np.float64)
    p, n = onmf._parts_d(y, x, d, m, spec)
    return p, np.broadcast_to(n, p.shape)      # kl without a mask: the [K, 1] column sum on every column


# Paths (float32), from nmf_xupdate_splits, pick_tier, x6_tier and plan_splits_x6_tn (nmf_impl.hpp, gemm.hpp).
# x update Y . D^T: NT, M = N rows, N = K atoms, reduction F; split over F when the row tiles cannot fill the chip
# and F >= 1024 (EpiSlab partials, then mu_quotient_slabs_kernel -- split_gram needs X_out != X, never so here --
# or, masked l2 / beta with N % 256 == 0, the stacked [A_neg ; A_pos] . D^T and mu_quotient_stacked_kernel);
# unsplit, the quotient is fused into the GEMM (EpiMuNum).  Statistics X^T [B1 | B2]: TN, M = K, reduction N.
# l2 without a mask: grad_neg = (x^T x) D, a gemm<FORM_NN> that reads stats + F at lda = F + K.
# name, N, F, K, x-update path, statistics path, x update on the bf16x6 core, statistics on the bf16x6 core
CASES = [
    ('fixture', 30, 20, 3, 'unsplit EpiMuNum, 64x64', '64x64, one partial tile', False, False),
    ('one_row', 1, 257, 5, 'unsplit EpiMuNum, 64x64', 'FLAT 32x128', False, False),
    ('rows_lt_atoms', 40, 300, 64, 'unsplit EpiMuNum, 64x64', '64x64', False, False),
    ('speedtest_width', 1000, 5000, 10, 'split-F x8, TALL 128x32, slabs (N % 256 != 0: unstacked)', 'FLAT', False,
     False),
    ('split_f', 256, 4096, 64, 'split-F x8, 64x64; stacked for masked l2 / beta', '64x64', False, False),
    ('ragged', 513, 1030, 70, 'split-F x2, 64x64, slabs', '64x64', False, False),
    ('deep_stats', 300, 600, 520, 'unsplit EpiMuNum, 64x64', 'HUGE_DEEP', False, False),
    # too few tiles for the 128 x 128 tier: fp32 core throughout (a 1024-row minibatch is no bf16x6 case)
    ('whole128_small', 1024, 1024, 128, 'split-F x2, 64x64 (too few tiles for 128x128)', '64x64, 2 splits', False,
     False),
    # enough 128 x 128 tiles: both l2 products on the split-bf16 core
    ('bf16x6', 4096, 2048, 256, 'split-F x4, bf16x6 128x128, slabs', 'bf16x6 128x128, 8 splits', True, True),
]
BIG = ('bf16x6', 'whole128_small')


def _combos():
    out = []
    for c in CASES:
        for lik in LIKS:
            for masked in (False, True):
                for nx in (0, 1, 3):
                    if c[0] in BIG and not (lik == 'l2' and not masked) and nx != 1:
                        continue            # the big shapes: the l2 Gram path in full, the rest once
                    if c[0] == 'whole128_small' and lik != 'l2':
                        continue
                    out.append((c, lik, masked, nx))
    return out


COMBOS = _combos()


@pytest.mark.parametrize('combo', COMBOS, ids=['%s-%s-%s-nx%d' % (c[0], l, 'mask' if m else 'nomask', n)
                                               for c, l, m, n in COMBOS])
def test_grads_against_float64(combo):
    (name, N, F, K, _, _, x6_x, x6_s), lik, masked, nx = combo
    Y, M, X, D = _data(N, F, K, masked, seed=N + F + K + nx)
    spec = LIKS[lik][2]
    xref = _x_ref(Y, M, X, D, spec, nx)
    gram = lik == 'l2' and not masked
    outs = {}
    for dt, modes in ((np.float64, (None,)), (np.float32, (0, 1))):
        for mode in modes:
            args = [a if a is None else a.astype(dt) for a in (Y, M, X, D)]
            if mode is None:
                xo, gp, gn = _grads(*args, lik, nx)
            else:
                with _Mode(mode):
                    xo, gp, gn = _grads(*args, lik, nx)
            outs[(dt, mode)] = (xo, gp, gn)
            assert xo.dtype == dt and gp.shape == (K, F) and gn.shape == (K, F)
            ex = _rel(xo, xref)
            assert ex <= _x_bound(dt, F, K, nx), (name, dt, mode, 'X_out', ex, _x_bound(dt, F, K, nx))
            pref, nref = _d_ref(Y, M, xo, D, spec)
            bd = _d_bound(dt, N, F, K)
            ep, en = _rel(gp, pref), _rel(gn, nref)
            assert ep <= bd and en <= bd, (name, dt, mode, 'gpos / gneg', ep, en, bd)
    # the path claims: the two product modes run identical code unless a product takes the split-bf16 core
    (x0, p0, n0), (x1, p1, n1) = outs[(np.float32, 0)], outs[(np.float32, 1)]
    on_x = gram and x6_x and nx > 0
    assert np.array_equal(x0, x1) == (not on_x), (name, 'x-update path')
    if not on_x:
        on_s = gram and x6_s
        assert (np.array_equal(p0, p1) and np.array_equal(n0, n1)) == (not on_s), (name, 'statistics path')


@pytest.mark.parametrize('name', ['bf16x6', 'whole128_small'])
def test_grads_statistics_path_probe(name):
    """Integer Y and D (exact in bf16, sums below 2^24): the x update is exact on both cores and X_out is bitwise
    equal across the modes, so the D-side parts are bitwise equal if and only if the statistics product is on the
    fp32 core."""
    c = [c for c in CASES if c[0] == name][0]
    _, N, F, K, _, _, _, x6_s = c
    rng = np.random.RandomState(7)
    Y = rng.randint(0, 4, (N, F)).astype(np.float32)
    D = rng.randint(1, 4, (K, F)).astype(np.float32)
    X = rng.uniform(0.1, 1.0, (N, K)).astype(np.float32)
    with _Mode(0):
        x0, p0, n0 = _grads(Y, None, X, D, 'l2', 1)
    with _Mode(1):
        x1, p1, n1 = _grads(Y, None, X, D, 'l2', 1)
    assert np.array_equal(x0, x1)
    assert (np.array_equal(p0, p1) and np.array_equal(n0, n1)) == (not x6_s)


# ---- the public helpers ----------------------------------------------------------------------------------------
@pytest.mark.parametrize('shape', [(1000, 5000, 10), (513, 1030, 70), (300, 600, 520)],
                         ids=lambda s: 'x'.join(map(str, s)))
@pytest.mark.parametrize('dt', [np.float32, np.float64], ids=['float32', 'float64'])
def test_public_helpers_against_oracle(shape, dt):
    """Gaussian / Poisson / BetaDivergence .grad_x / .grad_d (dcp_nmf_grad_x_*, dcp_nmf_grads_* with no x update)
    and Gaussian.logp (dcp_nmf_gauss_logp_*) against the oracle's parts and the logp formula."""
    from decomp_amd.nmf_methods import grads as g
    N, F, K = shape
    for masked in (False, True):
        Y, M, X, D = _data(N, F, K, masked, seed=N + K)
        y, x, d = (a.astype(dt) for a in (Y, X, D))
        m = None if M is None else M.astype(dt)
        y64, x64, d64 = (a.astype(np.float64) for a in (Y, X, D))
        m64 = None if M is None else M.astype(np.float64)
        bx = 3 * _P(dt, max(F, K)) + 4 * U[dt]
        bd = _d_bound(dt, N, F, K)
        for obj, spec in ((g.Gaussian(), 'l2'), (g.Poisson(), 'kl'), (g.BetaDivergence(0.0), 0.0),
                          (g.BetaDivergence(0.5), 0.5)):
            for got, ref, b in ((obj.grad_x(y, x, d, m), onmf._parts_x(y64, x64, d64, m64, spec), bx),
                                (obj.grad_d(y, x, d, m), onmf._parts_d(y64, x64, d64, m64, spec), bd)):
                for gg, rr in zip(got, ref):
                    assert isinstance(gg, np.ndarray) and gg.dtype == dt and gg.shape == rr.shape
                    assert _rel(gg, rr) <= b, (type(obj).__name__, spec, masked, _rel(gg, rr), b)
        for scale in (1.0, 0.7):
            r = (y64 - x64.dot(d64)) / scale
            e = -0.5 * r * r - np.log(scale) - np.pi * 0.5
            if m64 is not None:
                e = e * m64
            ref = float(np.sum(e))
            got = float(g.Gaussian(scale=scale).logp(y, x, d, m))
            # the residual of a depth-K product, squared, summed in double: relative to sum |terms|
            tol = (3 * _P(dt, K) + 4 * U[dt]) * float(np.sum(np.abs(e))) + 1e-12 * abs(ref)
            assert abs(got - ref) <= tol, (scale, masked, got, ref, tol)


# ---- dcp_nmf_apply_* -------------------------------------------------------------------------------------------
APPLY_F = [1, 20, 255, 256, 257, 4096, 4097, 5000, 9000]
APPLY_K = [1, 3, 255, 256, 257, 1030]
ALPHAS = [-1.0, 0.0, 0.3, 1.0]


def _apply(D, P, Q, alpha):
    import torch
    from decomp_amd import _arrays, _hip
    d, p, q = _dev(D), _dev(P), _dev(Q)
    out = torch.empty_like(d)
    md = ctypes.c_double(-1.0)
    lib, h = _lib_h(d)
    fn = getattr(lib, 'dcp_nmf_apply_' + _arrays.suffix(d))
    K, F = D.shape
    _hip.check(h, fn(h, _arrays.ptr(d), _arrays.ptr(p), _arrays.ptr(q), float(alpha), _arrays.ptr(out), K, F,
                     ctypes.byref(md)), 'dcp_nmf_apply')
    return out.cpu().numpy(), md.value


def _rule(D, P, Q, alpha):
    """kasai.py:77-78 (alpha >= 0) / serizel.py:54-57 (alpha < 0) in float64."""
    D, P, Q = (a.astype(np.float64) for a in (D, P, Q))
    q = np.maximum(Q, 1e-15)
    if alpha < 0:
        return D * np.maximum(P, 0.0) / q
    return np.maximum(D * ((1.0 - alpha) + alpha * P / q), 0.0)


def _apply_inputs(K, F, dt, seed):
    """D not normalised (rows of any norm, the last one 10x: the largest change sits in the last row); P partly
    negative; Q with zeros and values below the 1e-15 clamp."""
    rng = np.random.RandomState(seed)
    D = rng.uniform(0.1, 1.0, (K, F))
    D[-1] *= 10.0
    P = rng.uniform(-0.5, 1.5, (K, F)) if F > 1 else rng.uniform(0.1, 1.5, (K, F))   # (F = 1: no zero rows)
    Q = rng.uniform(0.5, 1.5, (K, F))
    n = max(2, K * F // 1000)
    flat = Q.reshape(-1)
    idx = rng.choice(K * F, size=min(n, K * F), replace=False)
    flat[idx[0::2]] = 0.0
    flat[idx[1::2]] = 1e-20
    return D.astype(dt), P.astype(dt), Q.astype(dt)


@pytest.mark.parametrize('K', APPLY_K)
@pytest.mark.parametrize('F', APPLY_F)
def test_apply_against_float64(F, K):
    """Normalise path: row_normalize_kernel keeps rows of F <= 4096 in registers, and strides over longer ones;
    reduce_vector_kernel (MaxOp) reduces K rows.  D_new against l2_strict(rule) from the same inputs: the rule costs a
    few u
    per entry (relative to D (|1 - alpha| + alpha |P| / q) where it cancels), the norm P(F) + 2u, the division u.
    max|dD| must equal np.max(np.abs(D - D_new)) exactly; a row whose rule output is all zero gives NaN there and
    in max|dD|, as the reference's U / sqrt(0) does."""
    path = 'cached' if F <= 4096 else 'strided'
    for dt in (np.float32, np.float64):
        D, P, Q = _apply_inputs(K, F, dt, seed=F * 7 + K)
        for alpha in ALPHAS:
            Dn, md = _apply(D, P, Q, alpha)
            U64 = _rule(D, P, Q, alpha)
            ref = l2_strict(U64)
            nrm = np.sqrt(np.sum(U64 * U64, axis=1, keepdims=True))
            D64, P64 = D.astype(np.float64), P.astype(np.float64)
            scale = D64 * (abs(1.0 - alpha) + abs(alpha) * np.abs(P64) / np.maximum(Q.astype(np.float64), 1e-15))
            tol = (_P(dt, F) + 4 * U[dt]) * np.abs(ref) + 4 * U[dt] * scale / nrm
            err = np.abs(Dn.astype(np.float64) - ref)
            assert Dn.dtype == dt and np.all(err <= tol), (path, dt, alpha, float(np.max(err - tol)))
            assert md == float(np.max(np.abs(D - Dn))), (path, dt, alpha, md)
            # one all-zero rule row (D row of zeros: zero for every alpha), placed past row 256 where there is one
            z = min(K - 1, 256 + (K - 1) % 7) if K > 256 else K // 2
            Dz = D.copy()
            Dz[z] = 0
            Dn2, md2 = _apply(Dz, P, Q, alpha)
            assert np.all(np.isnan(Dn2[z])) and np.isnan(md2), (path, dt, alpha)
            keep = np.arange(K) != z
            assert np.array_equal(Dn2[keep], Dn[keep]), (path, dt, alpha)


# ---- dcp_axpby_* -----------------------------------------------------------------------------------------------
AXPBY_N = [1, 255, 257, 524289, 640000]


def _axpby(n, a, x, b, y):
    from decomp_amd import _arrays, _hip
    lib, h = _lib_h(y)
    fn = getattr(lib, 'dcp_axpby_' + _arrays.suffix(y))
    _hip.check(h, fn(h, n, float(a), _arrays.ptr(x), float(b), _arrays.ptr(y)), 'dcp_axpby')


@pytest.mark.parametrize('n', AXPBY_N)
@pytest.mark.parametrize('dt', [np.float32, np.float64], ids=['float32', 'float64'])
def test_axpby(n, dt):
    """y = a x + b y past grid_for's cap of 2048 x 256 = 524288 elements (the grid-stride loop), every zero / non-zero
    pattern of (a, b) with NaN and Inf in the operand that is not read, and x aliasing y.  Within 2 u (|a x| + |b y|)
    of the same expression in the dtype (the compiler may contract it to an FMA)."""
    import torch
    rng = np.random.RandomState(n % 1000)
    X = rng.uniform(0.1, 2.0, n).astype(dt)
    Y = rng.uniform(0.1, 2.0, n).astype(dt)
    bad = np.where(np.arange(n) % 2 == 0, np.nan, np.inf).astype(dt)
    for a, b in ((0.0, 0.0), (0.0, -1.3), (0.7, 0.0), (0.7, -1.3)):
        A, B = dt(a), dt(b)
        xs = bad if a == 0.0 else X
        ys = bad if b == 0.0 else Y
        x, y = _dev(xs), _dev(ys)
        _axpby(n, a, x, b, y)
        got = y.cpu().numpy()
        with np.errstate(invalid='ignore', over='ignore'):
            ref = (A * X if a != 0.0 else np.zeros(n, dt)) + (B * Y if b != 0.0 else np.zeros(n, dt))
        mag = np.abs(A * X.astype(np.float64)) * (a != 0.0) + np.abs(B * Y.astype(np.float64)) * (b != 0.0)
        assert np.all(np.isfinite(got)), (a, b)
        assert np.all(np.abs(got.astype(np.float64) - ref) <= 2 * U[dt] * mag), (a, b)
        # x aliasing y: y = (a + b) y, each coefficient read once
        y = _dev(Y)
        _axpby(n, a, y, b, y)
        got = y.cpu().numpy()
        ref = A * Y + B * Y if (a != 0.0 and b != 0.0) else (A * Y if b == 0.0 else B * Y)
        if a == 0.0 and b == 0.0:
            ref = np.zeros(n, dt)
        mag = (abs(a) + abs(b)) * np.abs(Y.astype(np.float64))
        assert np.all(np.abs(got.astype(np.float64) - ref) <= 2 * U[dt] * mag), ('alias', a, b)
    torch.cuda.synchronize()


# ---- dcp_mu_quotient_* -----------------------------------------------------------------------------------------
@pytest.mark.parametrize('shape', [(1, 1), (513, 70), (2100, 257), (1000, 1030)], ids=lambda s: 'x'.join(map(str, s)))
@pytest.mark.parametrize('dt', [np.float32, np.float64], ids=['float32', 'float64'])
def test_mu_quotient_multi_tile(shape, dt):
    """The user-Likelihood step of the minibatch loop on a multi-tile [N, K] (past grid_for's cap at 2100 x 257 and
    1000 x 1030), in place and out of place: cur o max(pos, 0) / max(neg, 1e-15), a product and a quotient, each
    correctly rounded, and the clamp constant's own rounding in the dtype (within 3 u relative)."""
    import torch
    from decomp_amd import _arrays, _hip
    N, K = shape
    rng = np.random.RandomState(N + K)
    cur = rng.uniform(0.1, 1.0, (N, K)).astype(dt)
    pos = rng.uniform(-0.5, 1.5, (N, K)).astype(dt)
    neg = rng.uniform(0.5, 1.5, (N, K)).astype(dt)
    neg.reshape(-1)[::97] = 0.0
    neg.reshape(-1)[1::89] = 1e-20
    ref = onmf._quotient(cur.astype(np.float64), pos.astype(np.float64), neg.astype(np.float64))
    for inplace in (False, True):
        c, p, q = _dev(cur), _dev(pos), _dev(neg)
        out = c if inplace else torch.empty_like(c)
        lib, h = _lib_h(c)
        fn = getattr(lib, 'dcp_mu_quotient_' + _arrays.suffix(c))
        _hip.check(h, fn(h, _arrays.ptr(c), _arrays.ptr(p), _arrays.ptr(q), N, K, _arrays.ptr(out)),
                   'dcp_mu_quotient')
        got = out.cpu().numpy()
        assert np.all(np.abs(got - ref) <= 3 * U[dt] * np.abs(ref)), (inplace, _rel(got, ref))
