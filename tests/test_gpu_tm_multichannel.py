"""GPU: decomp_amd.template_matching.pursuit / orthogonal_pursuit / predict with multichannel templates D [T, Ch, S]
and the raw entries dcp_tm_mc_* against the NumPy references of tm_multichannel_ref.py -- supports, coefficients, step
counts, per-signal properties and the residual stop on the shared cases, Ch = 1 against the one-channel call, the
channel-interleaved one-channel call on 'VALID', every template-block, channel-pass and c-tile boundary of the
correlation kernel, truncated atoms, the no-LDS fallback, the global tier of the step kernels, exact values and ties,
tol over all channels, predict and the error surface, in all four dtypes.

Signals whose reference selection margin is below delta (1e-4 single, 1e-8 double), and in tol runs signals whose
residual margin is below 1e-4, are left out of the support and coefficient comparison (at most 10 % per case, asserted
here and, without a GPU, in test_tm_multichannel_ref_host.py); the properties are checked on every signal.  The
bounds are 4 x what the Gram form in the test dtype on the CPU shows against the residual form in double, floor 64 eps
(tm_multichannel_ref.Analysis.bounds)."""
import ctypes

import numpy as np
import pytest

import tm_multichannel_ref as ref
import tm_omp_ref as op
import tm_pursuit_ref as mp

pytestmark = pytest.mark.gpu

DTYPES = ['float32', 'float64', 'complex64', 'complex128']
SFX = {'float32': 'f32', 'float64': 'f64', 'complex64': 'c64', 'complex128': 'c128'}
CODERS = ['mp', 'omp']


def _precision(dt):
    return 'single' if np.dtype(dt) in (np.dtype(np.float32), np.dtype(np.complex64)) else 'double'


def _query(name, dt, *args):
    from decomp_amd import _hip
    return getattr(_hip.load(), 'dcp_tm_%s_%s' % (name, SFX[np.dtype(dt).name]))(*args)


def _coder(coder):
    from decomp_amd import template_matching as tm
    return tm.pursuit if coder == 'mp' else tm.orthogonal_pursuit


def _check_against(an, dt, it, x, solve, tag):
    """Supports, coefficients, step counts and the per-signal properties of a GPU result against an Analysis.
    solve(y) runs the same call on other signals: a signal alone must give its row of the batch bit for bit, and the
    `it` of that call is the signal's step count."""
    precision = _precision(dt)
    N, stride, padding = an.geom
    assert x.dtype == np.dtype(dt) and x.shape == an.x.shape
    B = x.shape[0]
    keep = an.keep(precision)
    left_out = 1.0 - float(np.mean(keep))
    b_coef, b_orth, b_res = an.bounds(precision)
    nnz = np.count_nonzero(x.reshape(B, -1), axis=1)
    err = float(np.max(np.abs(x.astype(an.x.dtype) - an.x)[keep], initial=0.0)) / float(np.max(np.abs(an.x)))
    res, orth = an.metrics(x)
    print('%s %s %s: left out %.2f %%; coefficient error %.3g (bound %.3g); residual excess %.3g (bound %.3g); '
          'orthogonality %.3g (bound %s); steps %s; it %d'
          % (tag, an.coder, np.dtype(dt).name, 100 * left_out, err, b_coef, float(res.max()), b_res, float(orth.max()),
             b_orth, sorted(set(an.steps.tolist())), it))
    assert left_out <= ref.MAX_LEFT_OUT
    assert np.all(np.isfinite(x))
    assert np.array_equal((x != 0)[keep], (an.x != 0)[keep])
    steps = np.zeros(B, dtype=np.int64)
    for b in range(B):
        steps[b], xb = solve(an.y[b:b + 1].astype(dt))
        assert np.array_equal(xb[0], x[b]), 'signal %d alone differs from its row of the batch' % b
    assert np.array_equal(steps[keep], an.steps[keep])
    assert it == int(steps.max())
    assert np.all(nnz <= steps)
    assert err <= b_coef
    assert float(res.max()) <= b_res
    if an.coder == 'omp':
        assert float(orth.max()) <= b_orth
    return nnz


def _run(an, dt):
    """The Analysis' coder on its problem in dtype dt, with its n / tol: (it, x, solve) for _check_against."""
    N, stride, padding = an.geom
    D = an.D.astype(dt)
    kw = dict(positive=an.positive) if an.coder == 'mp' else {}

    def solve(y):
        return _coder(an.coder)(y, D, n_nonzero_coefs=an.n, tol=an.tol, stride=stride, padding=padding, **kw)
    it, x = solve(an.y.astype(dt))
    assert isinstance(x, np.ndarray)
    return it, x, solve


# ---- the shared cases ---------------------------------------------------------------------------------------------
@pytest.mark.parametrize('dt', DTYPES)
@pytest.mark.parametrize('case', sorted(ref.CASES))
@pytest.mark.parametrize('coder', CODERS)
def test_supports_coefficients_and_properties(coder, case, dt):
    nev = ref.CASES[case][-1]
    an = ref.case_analysis(coder, case, np.dtype(dt).kind == 'c', False)
    nnz = _check_against(an, dt, *_run(an, dt), tag='case %d' % case)
    assert np.all(nnz <= nev)


@pytest.mark.parametrize('dt', DTYPES)
@pytest.mark.parametrize('case', sorted(ref.CASES))
@pytest.mark.parametrize('coder', CODERS)
def test_residual_stop(coder, case, dt):
    """tol = 0.02 median|y|^2 over all channels and the step limit left at its default."""
    an = ref.case_analysis(coder, case, np.dtype(dt).kind == 'c', True)
    assert an.n is None
    _check_against(an, dt, *_run(an, dt), tag='case %d tol' % case)


# ---- Ch = 1 against the one-channel call ----------------------------------------------------------------------------
@pytest.mark.parametrize('dt', DTYPES)
@pytest.mark.parametrize('case', [0, 1, 2])
@pytest.mark.parametrize('coder', CODERS)
def test_one_channel_against_the_2d_call(coder, case, dt):
    """D [T, 1, S] runs the multichannel kernels, whose sums are in the order of the one-channel ones: bit for bit the
    2-D call's x and it in the real dtypes; in the complex ones (the existing pass leaves open which product of a
    complex multiply-add is fused) the same supports on the kept signals and coefficients within the bounds."""
    one = mp if coder == 'mp' else op
    B, T, S, N, stride, padding, nev = mp.CASES[case]
    cplx = np.dtype(dt).kind == 'c'
    an = one.case_analysis(case, cplx, False)
    y, D = an.y.astype(dt), an.D.astype(dt)
    for kw in (dict(n_nonzero_coefs=nev), dict(tol=one.case_tol(case, cplx))):
        it2, x2 = _coder(coder)(y, D, stride=stride, padding=padding, **kw)
        it3, x3 = _coder(coder)(y[:, None, :], D[:, None, :], stride=stride, padding=padding, **kw)
        assert x3.shape == x2.shape and x3.dtype == x2.dtype
        if not cplx:
            assert it3 == it2 and np.array_equal(x3, x2)
    # (the n run, whose Analysis is at hand)
    precision = _precision(dt)
    it3, x3 = _coder(coder)(y[:, None, :], D[:, None, :], n_nonzero_coefs=nev, stride=stride, padding=padding)
    keep = an.keep(precision)
    assert np.array_equal((x3 != 0)[keep], (an.x != 0)[keep])
    err = float(np.max(np.abs(x3.astype(an.x.dtype) - an.x)[keep], initial=0.0)) / float(np.max(np.abs(an.x)))
    assert err <= an.bounds(precision)[0]


# ---- the interleave identity ------------------------------------------------------------------------------------------
@pytest.mark.parametrize('dt', DTYPES)
@pytest.mark.parametrize('case', ref.VALID_CASES)
@pytest.mark.parametrize('coder', CODERS)
def test_interleaved_one_channel_call(coder, case, dt):
    """'VALID': the one-channel coder on the channel-interleaved signal with stride Ch is the same problem -- the same
    supports on the kept signals, both results within the coefficient bound of the (common) reference."""
    B, T, Ch, S, N, stride, padding, nev = ref.CASES[case]
    an = ref.case_analysis(coder, case, np.dtype(dt).kind == 'c', False)
    precision = _precision(dt)
    y, D = an.y.astype(dt), an.D.astype(dt)
    y1, D1 = ref.interleave(y, D)
    it, x = _coder(coder)(y, D, n_nonzero_coefs=nev, stride=stride, padding='VALID')
    it1, x1 = _coder(coder)(y1, D1, n_nonzero_coefs=nev, stride=stride * Ch, padding='VALID')
    assert x.shape == x1.shape
    keep = an.keep(precision)
    assert np.array_equal((x != 0)[keep], (x1 != 0)[keep]) and np.array_equal((x != 0)[keep], (an.x != 0)[keep])
    scale = float(np.max(np.abs(an.x)))
    b_coef = an.bounds(precision)[0]
    for got in (x, x1):
        assert float(np.max(np.abs(got.astype(an.x.dtype) - an.x)[keep], initial=0.0)) / scale <= b_coef
    if keep.all():
        assert it == it1


# ---- template-block, channel-pass and c-tile boundaries of the correlation kernel --------------------------------------
@pytest.mark.parametrize('dt', DTYPES)
@pytest.mark.parametrize('where', ['last', 'first'])
def test_block_and_pass_boundaries(dt, where):
    """T around the template block, Ch around the channels of a pass, C around the 256-wide c tile (S = 3, 'VALID': the
    smallest sizes that give them).  One noiseless event a on the last template at the last c; D is non-zero in the
    last (or the first) channel only, so a dropped channel, template or position loses the event outright.  The
    coefficient is alpha / rho2, two 3-term sums and a quotient: within (2 S + 1) eps < 64 eps of a."""
    dt = np.dtype(dt)
    TB = _query('mc_template_block', dt)
    S, stride = 3, 1
    CP = _query('mc_channels_per_pass', dt, S, stride)
    assert TB >= 2 and CP >= 2
    eps = float(np.finfo(dt).eps)
    rng = np.random.RandomState(3)
    a = 1.5
    seen = 0
    for T in sorted({1, TB - 1, TB, TB + 1, 2 * TB + 1}):
        for Ch in sorted({1, CP - 1, CP, CP + 1, 2 * CP + 1}):
            ch = Ch - 1 if where == 'last' else 0
            d = rng.randn(T, S) + (1j * rng.randn(T, S) if dt.kind == 'c' else 0)
            D = np.zeros((T, Ch, S), dtype=dt)
            D[:, ch] = d
            for C in (255, 256, 257):
                N = C + S - 1
                y = np.zeros((2, Ch, N), dtype=dt)
                y[0, :, N - S:] = a * D[T - 1]                  # atom (T - 1, C - 1); signal 1 is zero
                for coder in CODERS:
                    it, x = _coder(coder)(y, D, n_nonzero_coefs=1, stride=stride, padding='VALID')
                    assert it == 1 and x.shape == (2, T, C)
                    assert np.array_equal(np.flatnonzero(x), [(T - 1) * C + C - 1]), (T, Ch, C, coder)
                    assert abs(x[0, T - 1, C - 1] - a) <= 64 * eps * a, (T, Ch, C, coder)
                    seen += 1
    assert seen >= 2 * 3 * 4 * 4


# ---- truncated atoms: the explicit overlap sum over the channels --------------------------------------------------------
@pytest.mark.parametrize('dt', DTYPES)
@pytest.mark.parametrize('coder', CODERS)
def test_truncated_atoms(coder, dt):
    y, D, geom, x0 = ref.edge_problem(np.dtype(dt).kind == 'c')
    assert D.shape[1] == 3
    an = ref.Analysis(coder, y, D, geom, n=3)
    assert np.array_equal(an.x != 0, x0 != 0)
    _check_against(an, dt, *_run(an, dt), tag='edge')
    if coder == 'omp':
        # noiseless up to the rounding of y to single-exact entries: the re-fit recovers the events to 64 eps (single)
        it, x, _ = _run(an, dt)
        assert np.max(np.abs(x - x0)) <= 64 * float(np.finfo(np.float32).eps) * np.max(np.abs(x0))


# ---- the no-LDS fallback of the correlation kernel --------------------------------------------------------------------
@pytest.mark.parametrize('dt', DTYPES)
def test_no_lds_fallback(dt):
    """The smallest S for which one channel's window does not fit (channels_per_pass = 0), B = T = Ch = 2,
    N = S + 40.  Two noiseless events per signal on distinct templates, 12 positions apart.  The Gram-form CPU reference
    is out of reach at this S (its lag correlations are (2 S - 1) S outer products), so the bound is the forward error
    of the sums themselves: a coefficient is a quotient of two sums of Ch S terms and one Gram update, each within
    Ch S eps of its condition, taken here as 8 Ch S eps relative to max|x_ref|; the supports and steps are exact."""
    dt = np.dtype(dt)
    S = 48 * 1024 // dt.itemsize - 255 + 1
    assert _query('mc_channels_per_pass', dt, S - 1, 1) == 1 and _query('mc_channels_per_pass', dt, S, 1) == 0
    B, T, Ch, N = 2, 2, 2, S + 40
    rng = np.random.RandomState(8)
    D = rng.randn(T, Ch, S) + (1j * rng.randn(T, Ch, S) if dt.kind == 'c' else 0)
    x0 = np.zeros((B, T, 41))
    x0[0, 0, 5], x0[0, 1, 17] = 2.0, -1.5
    x0[1, 1, 40], x0[1, 0, 28] = 1.75, 1.25
    y = ref.predict(x0.astype(D.dtype), D, N, 1, 'VALID')
    y, D = ref.single_exact(y, D)
    for coder in CODERS:
        an = ref.Analysis(coder, y, D, (N, 1, 'VALID'), n=2)
        assert np.array_equal(an.x != 0, x0 != 0) and an.left_out(_precision(dt)) == 0.0
        it, x = _coder(coder)(y.astype(dt), D.astype(dt), n_nonzero_coefs=2, stride=1, padding='VALID')
        assert it == 2 and np.array_equal(x != 0, an.x != 0)
        err = float(np.max(np.abs(x - an.x))) / float(np.max(np.abs(an.x)))
        print('no LDS %s %s: S = %d, coefficient error %.3g' % (coder, dt.name, S, err))
        assert err <= 8 * Ch * S * float(np.finfo(dt).eps)
        for b in range(B):
            assert np.array_equal(_coder(coder)(y[b:b + 1].astype(dt), D.astype(dt), n_nonzero_coefs=2, stride=1,
                                                padding='VALID')[1][0], x[b])


# ---- the global tier of the step kernels --------------------------------------------------------------------------
@pytest.mark.parametrize('dt', DTYPES)
@pytest.mark.parametrize('coder', CODERS)
def test_global_tier_of_the_step_kernel(coder, dt):
    """T C one above the largest size whose correlations the step kernel keeps in LDS, Ch = 2, S = 3, B = 2."""
    K = _query('pursuit_lds_atoms' if coder == 'mp' else 'omp_lds_atoms', dt) + 1
    y, D, geom = ref.tier_problem(K, np.dtype(dt).kind == 'c')
    an = ref.Analysis(coder, y, D, geom, n=5)
    assert an.x.shape == (2, 1, K)
    _check_against(an, dt, *_run(an, dt), tag='T C = %d (global tier)' % K)


# ---- exact values and exact ties ------------------------------------------------------------------------------------
@pytest.mark.parametrize('padding', ['VALID', 'SAME'])
@pytest.mark.parametrize('dt', DTYPES)
def test_dyadic_reselection_exact_values(dt, padding):
    """D = ones [1, 2, 2], y = 2 atom(3) + 1.5 atom(4) on both channels: alpha is twice and rho2 twice that of one
    channel, so the coefficients are those of the one-channel test -- atom 3, then atom 4, then atom 3 again."""
    from decomp_amd import template_matching as tm
    y = np.zeros((1, 2, 10), dtype=dt)
    y[0, :, 3:5] += 2
    y[0, :, 4:6] += 1.5
    D = np.ones((1, 2, 2), dtype=dt)
    c = 3 if padding == 'VALID' else 4
    for n, want in ((1, (2.75, 0.0)), (2, (2.75, 1.125)), (3, (2.1875, 1.125))):
        it, x = tm.pursuit(y, D, n_nonzero_coefs=n, padding=padding)
        assert it == n
        assert x[0, 0, c] == want[0] and x[0, 0, c + 1] == want[1]
        assert np.count_nonzero(x) == np.count_nonzero(want)
    it, x = tm.orthogonal_pursuit(y, D, n_nonzero_coefs=1, padding=padding)   # pivot sqrt(4): exact
    assert it == 1 and x[0, 0, c] == 2.75 and np.count_nonzero(x) == 1


@pytest.mark.parametrize('dt', DTYPES)
@pytest.mark.parametrize('coder', CODERS)
def test_exact_ties_go_to_the_lowest_flat_index(coder, dt):
    dt = np.dtype(dt)
    D = np.ones((1, 4, 1), dtype=dt)            # rho2 = 4: the quotient and the pivot are exact
    for K, tied in ((4, (1, 2)), (130, (5, 70)), (130, (63, 64)), (300, (255, 256)), (1100, (1023, 1024)),
                    (130, tuple(range(130)))):
        y = np.ones((2, 4, K), dtype=dt)
        y[0][:, list(tied)] = 2
        y[1][:, list(tied)] = -2
        if dt.kind == 'c':
            y[1][:, list(tied)] = 2j            # the same magnitude, another phase
            y[1][:, tied[0]] = 2
        it, x = _coder(coder)(y, D, n_nonzero_coefs=1)
        assert it == 1 and x.shape == (2, 1, K)
        for b in range(2):
            assert np.array_equal(np.flatnonzero(x[b]), [tied[0]]), (K, tied, b)
            assert x[b, 0, tied[0]] == y[b, 0, tied[0]]
    # identical templates: template 0
    rng = np.random.RandomState(5)
    d = rng.randn(1, 3, 6).astype(dt)
    it, x = _coder(coder)(rng.randn(9, 3, 50).astype(dt), np.concatenate([d, d]), n_nonzero_coefs=4)
    assert it == 4 and np.all(x[:, 1] == 0) and np.all(np.count_nonzero(x[:, 0], axis=1) >= 1)


# ---- tol is over all channels -----------------------------------------------------------------------------------------
@pytest.mark.parametrize('dt', DTYPES)
@pytest.mark.parametrize('coder', CODERS)
def test_tol_is_over_all_channels(coder, dt):
    """D = ones [1, 4, 1] (rho2 = 4, every quotient and pivot dyadic).  Signal 0: channel 0 alone holds 0.5 < tol = 1,
    all channels 8.5 > tol: a step (alpha = 2.5 at c = 1).  Signal 1: 0.75 in all channels: none at tol = 1, one at 0.7."""
    D = np.ones((1, 4, 1), dtype=dt)
    y = np.zeros((2, 4, 6), dtype=dt)
    y[0, 0, 1], y[0, 0, 4] = 0.5, 0.5
    y[0, 1, 1], y[0, 1, 3] = 2.0, 2.0
    y[1, 0, 2], y[1, 1, 2], y[1, 1, 5] = 0.5, 0.5, 0.5
    it, x = _coder(coder)(y, D, tol=1.0, padding='VALID')
    assert it >= 1 and x[0, 0, 1] == 0.625 and np.all(x[1] == 0)
    it, x = _coder(coder)(y[1:], D, tol=1.0, padding='VALID')
    assert it == 0 and np.all(x == 0)
    it, x = _coder(coder)(y[1:], D, tol=0.7, padding='VALID')
    assert it == 1 and x[0, 0, 2] == 0.25 and np.count_nonzero(x) == 1


# ---- predict ------------------------------------------------------------------------------------------------------
def _predict_bound(x, D, N, stride, padding, dt):
    """|error| of a sum of at most T ceil(S / stride) = 21 products: 21 additions and a (complex) product within 3 eps
    each, under 32 eps sum |x| |D|; taken as 64 eps sum |x| |D|, the project's floor factor."""
    return 64 * float(np.finfo(dt).eps) * ref.predict(np.abs(x), np.abs(D), N, stride, padding)


@pytest.mark.parametrize('stride', [1, 3])
@pytest.mark.parametrize('padding', ['VALID', 'SAME'])
@pytest.mark.parametrize('dt', DTYPES)
def test_predict(dt, padding, stride):
    from decomp_amd import template_matching as tm
    dt = np.dtype(dt)
    T, Ch, S, N = 3, 5, 7, 300
    C = ref.otm.geometry(S, N, stride, padding)[0]
    rng = np.random.RandomState(2)
    D = rng.randn(T, Ch, S) + (1j * rng.randn(T, Ch, S) if dt.kind == 'c' else 0)
    x = rng.randn(2, 3, T, C) * (rng.rand(2, 3, T, C) < 0.3)
    x = (x + (1j * rng.randn(2, 3, T, C) if dt.kind == 'c' else 0)).astype(dt)
    D = D.astype(dt)
    out = tm.predict(x, D, N, stride, padding)
    assert isinstance(out, np.ndarray) and out.shape == (2, 3, Ch, N) and out.dtype == dt
    x6, D6 = x.reshape(6, T, C).astype(np.result_type(dt, np.float64)), D.astype(np.result_type(dt, np.float64))
    want = ref.predict(x6, D6, N, stride, padding)
    assert np.all(np.abs(out.reshape(6, Ch, N) - want) <= _predict_bound(x6, D6, N, stride, padding, dt) + 1e-300)
    assert np.array_equal(tm.predict(x[1, 2], D, N, stride, padding), out[1, 2])
    # Ch = 1 against the one-channel predict: the same sum in the same order, bit for bit in the real dtypes (which
    # product of a complex multiply-add is fused is the compiler's choice per kernel)
    one3 = tm.predict(x, np.ascontiguousarray(D[:, :1]), N, stride, padding)[..., 0, :]
    one2 = tm.predict(x, np.ascontiguousarray(D[:, 0]), N, stride, padding)
    if dt.kind == 'c':
        assert np.all(np.abs(one3 - one2).reshape(6, N) <= 2 * _predict_bound(x6, D6[:, :1], N, stride, padding, dt)[:, 0])
    else:
        assert np.array_equal(one3, one2)


def test_predict_promotes_mixed_dtypes_and_keeps_tensors_on_the_device():
    import torch
    from decomp_amd import template_matching as tm
    rng = np.random.RandomState(4)
    T, Ch, S, N = 2, 3, 5, 40
    C = ref.otm.geometry(S, N, 1, 'SAME')[0]
    x = rng.randn(4, T, C).astype(np.float32)
    for Dd in (rng.randn(T, Ch, S), (rng.randn(T, Ch, S) + 1j * rng.randn(T, Ch, S)).astype(np.complex64)):
        dt2 = Dd[:, 0].dtype
        out = tm.predict(x, Dd, N)
        assert out.dtype == tm.predict(x, np.ascontiguousarray(Dd[:, 0]), N).dtype == np.result_type(np.float32, dt2)
        assert out.shape == (4, Ch, N)
        want = ref.predict(x.astype(np.float64), Dd.astype(np.result_type(dt2, np.float64)), N, 1, 'SAME')
        assert np.allclose(out, want, rtol=0, atol=1e-4 * np.max(np.abs(want)))
    xt, Dt = torch.from_numpy(x).cuda(), torch.from_numpy(rng.randn(T, Ch, S).astype(np.float32)).cuda()
    out = tm.predict(xt, Dt, N)
    assert torch.is_tensor(out) and out.is_cuda and tuple(out.shape) == (4, Ch, N)
    it, xc = tm.pursuit(out, Dt, n_nonzero_coefs=3)
    assert torch.is_tensor(xc) and xc.is_cuda and tuple(xc.shape) == (4, T, C)
    it, xc = tm.orthogonal_pursuit(out.reshape(2, 2, Ch, N), Dt, n_nonzero_coefs=3)
    assert torch.is_tensor(xc) and tuple(xc.shape) == (2, 2, T, C)
    it, xc = tm.pursuit(out[:0], Dt, n_nonzero_coefs=3)         # an empty batch
    assert it == 0 and tuple(xc.shape) == (0, T, C)


@pytest.mark.parametrize('dt', DTYPES)
@pytest.mark.parametrize('coder', CODERS)
def test_predict_of_the_code_reproduces_a_noiseless_event(coder, dt):
    from decomp_amd import template_matching as tm
    dt = np.dtype(dt)
    rng = np.random.RandomState(6)
    T, Ch, S, N = 3, 4, 6, 50
    D = (rng.randn(T, Ch, S) + (1j * rng.randn(T, Ch, S) if dt.kind == 'c' else 0)).astype(dt)
    for padding, stride in (('SAME', 1), ('VALID', 2)):
        C = ref.otm.geometry(S, N, stride, padding)[0]
        x0 = np.zeros((1, T, C), dtype=dt)
        x0[0, 2, ref.inside_atoms(S, N, stride, padding)[7]] = -1.75
        y = tm.predict(x0, D, N, stride, padding)
        it, x = _coder(coder)(y, D, n_nonzero_coefs=1, stride=stride, padding=padding)
        assert it == 1 and np.array_equal(x != 0, x0 != 0)
        back = tm.predict(x, D, N, stride, padding)
        assert np.max(np.abs(back - y)) <= 64 * float(np.finfo(dt).eps) * np.max(np.abs(y))


# ---- the error surface ------------------------------------------------------------------------------------------------
def test_python_checks_fire_before_any_gpu_call(monkeypatch):
    from decomp_amd import _arrays, template_matching as tm
    from decomp_amd.utils import exceptions

    def boom(*a, **k):
        raise AssertionError('a GPU call was made before the argument check')
    monkeypatch.setattr(_arrays, 'to_device', boom)
    y = np.zeros((4, 3, 30), dtype=np.float32)
    D = np.ones((2, 3, 5), dtype=np.float32)
    for coder in (tm.pursuit, tm.orthogonal_pursuit):
        for yy, DD in ((y, D[0, 0]), (y, D[None]), (y[0, 0], D), (y[:, :2], D), (y[:, :0], D[:, :0])):
            with pytest.raises((ValueError, exceptions.DimInvalidError)):
                coder(yy, DD, 3)
        with pytest.raises(AssertionError, match='GPU call'):
            coder(y, D, 3)


def _raw(name, y, D, B, T, Ch, S, N, stride, pad, n, *flags, null=None):
    """dcp_tm_mc_<name>_* on host arrays: (rc, message, it, x)."""
    import torch
    from decomp_amd import _arrays
    yd = torch.from_numpy(np.ascontiguousarray(y)).cuda()
    Dd = torch.from_numpy(np.ascontiguousarray(D)).cuda()
    x = torch.full((64, 64), float('nan'), dtype=yd.dtype, device='cuda')
    lib, h = _arrays.lib_handle(yd)
    it = ctypes.c_int(-1)
    ptrs = {'Y': _arrays.ptr(yd), 'D': _arrays.ptr(Dd), 'X': _arrays.ptr(x), 'it': ctypes.byref(it)}
    if null is not None:
        ptrs[null] = None
    rc = getattr(lib, 'dcp_tm_mc_%s_%s' % (name, _arrays.suffix(yd)))(h, ptrs['Y'], ptrs['D'], ptrs['X'], B, T, Ch, S, N,
                                                                     stride, pad, n, -1.0, *(flags + (ptrs['it'],)))
    return rc, lib.dcp_last_error_string(h).decode(), it.value, x.cpu().numpy()


@pytest.mark.parametrize('dt', DTYPES)
def test_raw_entries_invalid_arguments_return_an_error(dt):
    import torch
    from decomp_amd import _arrays
    y = np.ones((3, 2, 20), dtype=dt)
    D = np.ones((2, 2, 4), dtype=dt)
    for name, flags in (('pursuit', (0,)), ('omp', ())):
        for Ch in (0, -1, 2 ** 31):
            rc, msg, _, _ = _raw(name, y, D, 3, 2, Ch, 4, 20, 1, 1, 2, *flags)
            assert rc == -1 and 'Ch' in msg
        rc, msg, _, _ = _raw(name, y, D, 3, 2, 2, 21, 20, 1, 1, 2, *flags)
        assert rc == -1 and 'geometry' in msg
        rc, msg, _, _ = _raw(name, y, D, 3, 2, 2, 4, 20, 1, 1, 0, *flags)
        assert rc == -1 and 'n_steps' in msg
        for null in ('Y', 'D', 'X', 'it'):
            rc, msg, _, _ = _raw(name, y, D, 3, 2, 2, 4, 20, 1, 1, 2, *flags, null=null)
            assert rc == -1 and 'null' in msg
        rc, msg, it, x = _raw(name, y, D, 3, 2, 2, 4, 20, 1, 1, 2, *flags)      # C = 23: all of X [3, 2, 23] is written
        assert rc == 0 and it >= 1 and np.all(np.isfinite(x.ravel()[:3 * 2 * 23])) and np.all(np.isnan(x.ravel()[3 * 2 * 23:]))
    if np.dtype(dt).kind == 'c':
        rc, msg, _, _ = _raw('pursuit', y, D, 3, 2, 2, 4, 20, 1, 1, 2, 1)
        assert rc == -1 and 'real' in msg
    xd = torch.zeros((3, 2, 23), dtype=torch.from_numpy(y).dtype, device='cuda')
    Dd = torch.from_numpy(D).cuda()
    out = torch.zeros((3, 2, 20), dtype=xd.dtype, device='cuda')
    lib, h = _arrays.lib_handle(xd)
    fn = getattr(lib, 'dcp_tm_mc_predict_' + _arrays.suffix(xd))
    assert fn(h, _arrays.ptr(xd), _arrays.ptr(Dd), 3, 2, 0, 4, 20, 1, 1, _arrays.ptr(out)) == -1
    assert fn(h, None, _arrays.ptr(Dd), 3, 2, 2, 4, 20, 1, 1, _arrays.ptr(out)) == -1
    assert fn(h, _arrays.ptr(xd), _arrays.ptr(Dd), 3, 2, 2, 4, 20, 1, 1, _arrays.ptr(out)) == 0
