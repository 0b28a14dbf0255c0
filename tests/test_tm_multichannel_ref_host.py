"""CPU: the NumPy references of tm_multichannel_ref.py pinned without a GPU -- at Ch = 1 they are tm_pursuit_ref /
tm_omp_ref, on 'VALID' they are those references on the channel-interleaved problem, on a tiny 'SAME' problem they are
plain matching pursuit on the explicit operator [T C, Ch N]; the share of signals their own margins leave out of the
GPU comparison stays within the project's cap for every shared problem; and the argument checks of the public entry
points fire before any GPU call."""
import ctypes

import numpy as np
import pytest

import tm_multichannel_ref as ref
import tm_omp_ref as op
import tm_pursuit_ref as mp

SFX = ('f32', 'f64', 'c64', 'c128')


# ---- Ch = 1: the one-channel references, exactly ------------------------------------------------------------------
@pytest.mark.parametrize('cplx', [False, True])
@pytest.mark.parametrize('geom', [(40, 5, 1, 'SAME'), (64, 8, 2, 'VALID'), (50, 4, 6, 'SAME')])
def test_one_channel_reproduces_the_one_channel_references(geom, cplx):
    N, S, stride, padding = geom
    y, D, _ = mp.make_problem(7, 6, 2, S, N, stride, padding, 4, cplx)
    y3, D3 = y[:, None, :], D[:, None, :]
    tol = 0.02 * float(np.median(np.sum(np.abs(y) ** 2, axis=1)))
    for kw in (dict(n=4), dict(tol=tol)):
        for got, want in ((ref.mp_residual(y3, D3, N, stride, padding, **kw), mp.mp_residual(y, D, N, stride, padding, **kw)),
                          (ref.omp_residual(y3, D3, N, stride, padding, **kw), op.omp_residual(y, D, N, stride, padding, **kw))):
            for g, w in zip(got, want):
                assert np.array_equal(g, w)
        for precision in ('single', 'double'):
            dt = ref.precision_dtype(cplx, precision)
            for got, want in ((ref.mp_gram(y3.astype(dt), D3.astype(dt), N, stride, padding, **kw),
                               mp.mp_gram(y.astype(dt), D.astype(dt), N, stride, padding, **kw)),
                              (ref.omp_gram(y3.astype(dt), D3.astype(dt), N, stride, padding, **kw),
                               op.omp_gram(y.astype(dt), D.astype(dt), N, stride, padding, **kw))):
                assert got[0].dtype == dt and np.array_equal(got[0], want[0]) and np.array_equal(got[1], want[1])
    x = ref.mp_residual(y3, D3, N, stride, padding, n=4)[0]
    assert np.array_equal(ref.predict(x, D3, N, stride, padding)[:, 0], mp.predict(x, D, N, stride, padding))
    assert np.array_equal(ref.orthogonality(x, y3, D3, N, stride, padding), op.orthogonality(x, y, D, N, stride, padding))


def test_edge_problem_at_one_channel_is_that_of_tm_omp_ref():
    for cplx in (False, True):
        y, D, geom, x0 = ref.edge_problem(cplx, Ch=1)
        y1, D1, geom1, x01 = op.edge_problem(cplx)
        assert np.array_equal(y[:, 0], y1) and np.array_equal(D[:, 0], D1) and geom == geom1 and np.array_equal(x0, x01)


# ---- 'VALID': the one-channel references on the interleaved problem ----------------------------------------------------
@pytest.mark.parametrize('cplx', [False, True])
@pytest.mark.parametrize('case', ref.VALID_CASES)
def test_valid_cases_equal_the_interleaved_one_channel_problem(case, cplx):
    B, T, Ch, S, N, stride, padding, nev = ref.CASES[case]
    y, D = ref.case_problem(case, cplx)
    assert y.shape == (B, Ch, N) and D.shape == (T, Ch, S)
    y1, D1 = ref.interleave(y, D)
    assert np.array_equal(y1, mp.make_problem(300 + case, B, T, S * Ch, N * Ch, stride * Ch, 'VALID', nev, cplx)[0])
    for coder, one in (('mp', mp.mp_residual), ('omp', op.omp_residual)):
        for with_tol in (False, True):
            an = ref.case_analysis(coder, case, cplx, with_tol)
            x1, steps1 = one(y1, D1, N * Ch, stride * Ch, 'VALID', n=an.n, tol=an.tol)[:2]
            assert np.array_equal(an.x != 0, x1 != 0) and np.array_equal(an.steps, steps1)
            assert np.max(np.abs(an.x - x1)) <= 1e-12 * np.max(np.abs(x1))
    # the operator itself
    x = ref.case_analysis('mp', case, cplx, False).x
    assert np.allclose(ref.interleave(ref.predict(x, D, N, stride, padding), D)[0],
                       mp.predict(x, D1, N * Ch, stride * Ch, 'VALID'), rtol=0, atol=1e-12)


# ---- 'SAME': plain matching pursuit on the explicit operator ---------------------------------------------------------
@pytest.mark.parametrize('cplx', [False, True])
@pytest.mark.parametrize('stride', [1, 2])
def test_same_equals_matching_pursuit_on_the_dense_operator(stride, cplx):
    B, T, Ch, S, N, nev = 5, 2, 3, 4, 11, 3
    y, D, _ = ref.make_problem(11, B, T, Ch, S, N, stride, 'SAME', nev, cplx)
    A = ref.dense_operator(D, N, stride, 'SAME')
    C = A.shape[0] // T
    assert A.shape == (T * C, Ch * N) and np.any(np.sum(A != 0, axis=1) < Ch * S)      # truncated atoms exist
    x, steps = ref.mp_residual(y, D, N, stride, 'SAME', n=5)[:2]
    xd, stepsd = mp.mp_dense(y.reshape(B, -1), A, 5)
    assert np.array_equal(steps, stepsd) and np.array_equal(x.reshape(B, -1) != 0, xd != 0)
    assert np.max(np.abs(x.reshape(B, -1) - xd)) <= 1e-12 * np.max(np.abs(xd))
    assert np.allclose(ref.predict(x, D, N, stride, 'SAME').reshape(B, -1), x.reshape(B, -1) @ A, rtol=0, atol=1e-12)
    assert np.allclose(ref.correlate(y, D, N, stride, 'SAME').reshape(B, -1), y.reshape(B, -1) @ A.conj().T, rtol=0,
                       atol=1e-12)
    # the Gram forms in double are the residual forms to rounding (n = nev: the steps past the planted events fit the
    # noise, where the two forms may part on a near-tie)
    for gram, resid in ((ref.mp_gram, ref.mp_residual), (ref.omp_gram, ref.omp_residual)):
        xg, sg = gram(y, D, N, stride, 'SAME', n=nev)
        xr, sr = resid(y, D, N, stride, 'SAME', n=nev)[:2]
        assert np.array_equal(sg, sr) and np.max(np.abs(xg - xr)) <= 1e-10 * np.max(np.abs(xr))


# ---- the share of signals the margins leave out --------------------------------------------------------------------
@pytest.mark.parametrize('cplx', [False, True])
@pytest.mark.parametrize('case', sorted(ref.CASES))
def test_left_out_share_of_every_shared_case(case, cplx):
    for coder in ('mp', 'omp'):
        for with_tol in (False, True):
            an = ref.case_analysis(coder, case, cplx, with_tol)
            for precision in ('single', 'double'):
                share = an.left_out(precision)
                print('case %d %s %s %s %s: left out %.1f %%' % (case, 'complex' if cplx else 'real', coder,
                                                                 'tol' if with_tol else 'n', precision, 100 * share))
                assert share <= ref.MAX_LEFT_OUT
                if ref.CASES[case][6] == 'VALID':
                    assert share == 0.0
                coef, orth, res = an.bounds(precision)
                assert coef < 1e-2 and res < 1e-2 and (orth is None) == (coder == 'mp')


@pytest.mark.parametrize('cplx', [False, True])
def test_left_out_share_of_the_edge_problem(cplx):
    y, D, geom, x0 = ref.edge_problem(cplx)
    for coder in ('mp', 'omp'):
        an = ref.Analysis(coder, y, D, geom, n=3)
        for precision in ('single', 'double'):
            assert an.left_out(precision) == 0.0
        assert np.array_equal(an.x != 0, x0 != 0)
    an = ref.Analysis('omp', y, D, geom, n=3)
    assert np.max(np.abs(an.x - x0)) < 1e-6       # noiseless: the re-fit recovers the truncated events


@pytest.mark.parametrize('coder', ['mp', 'omp'])
@pytest.mark.parametrize('sfx', SFX)
def test_left_out_share_of_the_tier_problems(sfx, coder):
    """T C one above the largest size whose correlations the step kernel keeps in LDS."""
    from decomp_amd import _hip
    K = getattr(_hip.load(), 'dcp_tm_%s_lds_atoms_%s' % ('pursuit' if coder == 'mp' else 'omp', sfx))() + 1
    y, D, geom = ref.tier_problem(K, sfx[0] == 'c')
    an = ref.Analysis(coder, y, D, geom, n=5)
    assert an.left_out('single' if sfx in ('f32', 'c64') else 'double') == 0.0


# ---- argument checks before any GPU call ---------------------------------------------------------------------------
@pytest.fixture
def no_gpu(monkeypatch):
    from decomp_amd import _arrays, _hip

    def boom(*a, **k):
        raise AssertionError('a GPU call was made before the argument check')
    monkeypatch.setattr(_arrays, 'to_device', boom)
    monkeypatch.setattr(_hip, 'load', boom)


def test_errors_before_any_gpu_call(no_gpu):
    from decomp_amd import template_matching as tm
    from decomp_amd.utils import exceptions
    rng = np.random.RandomState(0)
    y = rng.randn(4, 3, 30).astype(np.float32)
    D = rng.randn(2, 3, 5).astype(np.float32)
    for coder in (tm.pursuit, tm.orthogonal_pursuit):
        with pytest.raises(exceptions.DimInvalidError):
            coder(y, D[0, 0], 3)                                      # D.ndim = 1
        with pytest.raises(exceptions.DimInvalidError):
            coder(y, D[None], 3)                                      # D.ndim = 4
        with pytest.raises(ValueError):
            coder(y[0, 0], D, 3)                                      # y.ndim = 1 with a 3-D D
        with pytest.raises(ValueError):
            coder(y[:, :2], D, 3)                                     # y.shape[-2] != Ch
        with pytest.raises(ValueError):
            coder(y, D[:, :2], 3)
        with pytest.raises(ValueError):
            coder(y[:, :0], D[:, :0], 3)                              # Ch = 0
        with pytest.raises(exceptions.DtypeMismatchError):
            coder(y, D.astype(np.float64), 3)
        with pytest.raises(ValueError):
            coder(y, D, 3, padding='FULL')
        with pytest.raises(ValueError):
            coder(y, D, 3, stride=0)
        with pytest.raises(ValueError):
            coder(y[:, :, :4], D, 3)                                  # S > N
        with pytest.raises(ValueError, match='n_nonzero_coefs or tol'):
            coder(y, D)
        with pytest.raises(ValueError):
            coder(y, D, 0)
        with pytest.raises(ValueError):
            coder(y, D, 3, tol=-1.0)
        with pytest.raises(AssertionError, match='GPU call'):         # a valid call reaches the GPU
            coder(y, D, 3)
        with pytest.raises(AssertionError, match='GPU call'):
            coder(y[0], D[:, :, :], tol=0.5, stride=2, padding='VALID')
    with pytest.raises(ValueError, match='real'):
        tm.pursuit(y.astype(np.complex64), D.astype(np.complex64), 3, positive=True)
    with pytest.raises(ValueError):
        tm.pursuit(y, D, 2 * 34 + 1)                                  # T C = 68 with 'SAME'
    with pytest.raises(exceptions.DimInvalidError):
        tm.predict(np.zeros((2, 34), dtype=np.float32), D[None], 30)
    with pytest.raises(ValueError):
        tm.predict(np.zeros((2, 34), dtype=np.float32), D[:, :0], 30)


def test_solve_keeps_refusing_multichannel_templates(monkeypatch):
    """solve with a 3-D D and a LASSO coder (the default acc_ista, and cd) raises NotImplementedError before any GPU
    call.  (The greedy coders do learn multichannel templates: test_tm_mc_learn_host.py, test_gpu_tm_mc_learn.py.)"""
    from decomp_amd import template_matching as tm, _arrays, _hip

    def boom(*a, **k):
        raise AssertionError('a GPU call was made before the argument check')
    monkeypatch.setattr(_arrays, 'to_device', boom)
    monkeypatch.setattr(_hip, 'load', boom)
    rng = np.random.RandomState(0)
    y = rng.randn(4, 3, 30)
    D = rng.randn(2, 3, 5)
    for kw in (dict(), dict(lasso_method='cd')):
        with pytest.raises(NotImplementedError, match='multichannel'):
            tm.solve(y, D, 0.1, maxiter=1, **kw)


# ---- the C ABI lists the new entries ------------------------------------------------------------------------------
def test_header_bindings_and_library_list_the_entries():
    from decomp_amd import _hip
    lib = _hip.load()
    for sfx, elem in zip(SFX, (4, 8, 8, 16)):
        for name, nargs in (('pursuit', 15), ('omp', 14), ('predict', 11), ('template_block', 0), ('channels_per_pass', 2)):
            full = 'dcp_tm_mc_%s_%s' % (name, sfx)
            assert hasattr(lib, full) and len(_hip.SIGNATURES[full][1]) == nargs
        tb = getattr(lib, 'dcp_tm_mc_template_block_' + sfx)()
        assert tb >= 2
        cpp = getattr(lib, 'dcp_tm_mc_channels_per_pass_' + sfx)
        assert cpp(5, 1) >= 2 and cpp(5, 1) >= cpp(5, 3) >= cpp(2000, 3) >= 0
        assert cpp(1 << 20, 1) == 0 and cpp(0, 1) == 0 and cpp(5, 0) == 0
    # no handle: DCP_ERR_INVALID, never a crash
    it = ctypes.c_int(0)
    assert lib.dcp_tm_mc_pursuit_f32(None, None, None, None, 1, 1, 1, 1, 1, 1, 0, 1, -1.0, 0, ctypes.byref(it)) == -1
    assert lib.dcp_tm_mc_omp_f32(None, None, None, None, 1, 1, 1, 1, 1, 1, 0, 1, -1.0, ctypes.byref(it)) == -1
    assert lib.dcp_tm_mc_predict_f32(None, None, None, 1, 1, 1, 1, 1, 1, 0, None) == -1
