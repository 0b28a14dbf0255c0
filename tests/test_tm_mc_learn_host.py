"""CPU: template_matching.solve with multichannel templates D [T, Ch, S] -- its argument checks run before any GPU
call; header, bindings and library list dcp_tm_mc_dstep_events_* / dcp_tm_mc_gather_windows_*; the calls a 3-D D makes;
and the NumPy loop of tm_mc_learn_ref.py, the yardstick of the GPU tests: tied to the one-channel reference through
the channel-interleaved problem, and learning the planted templates."""
import ctypes
import os
import re

import numpy as np
import pytest

import tm_learn_ref
import tm_mc_learn_ref as ref
import tm_multichannel_ref as mc

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
GREEDY = ('omp', 'mp', 'mp_pos')


@pytest.fixture
def no_gpu(monkeypatch):
    from decomp_amd import _arrays, _hip

    def boom(*a, **k):
        raise AssertionError('a GPU call was made before the argument check')
    monkeypatch.setattr(_arrays, 'to_device', boom)
    monkeypatch.setattr(_hip, 'load', boom)


def _problem(dtype=np.float32, N=30, Ch=3):
    rng = np.random.RandomState(0)
    return rng.randn(4, Ch, N).astype(dtype), rng.randn(2, Ch, 5).astype(dtype)   # N = 30: C = 34 ('SAME'), T C = 68


def _fastpath(tm, y, D, alpha, x=None, minibatch=None, size_of_minibatch=None, stride=1, padding='SAME', mask=None,
              **kw):
    return tm.solve_fastpath(y, D, alpha, x, stride, padding, 1e-4, minibatch, size_of_minibatch, 5,
                             kw['lasso_method'], kw.get('lasso_iter', 10), kw.get('lasso_tol', 1e-5),
                             np.random.RandomState(0), None, mask=mask)


def _both(tm, exc, y, D, alpha, match=None, **kw):
    """solve and solve_fastpath raise exc before any GPU call."""
    with pytest.raises(exc, match=match):
        tm.solve(y, D, alpha, **kw)
    x = np.zeros((y.shape[0], D.shape[0], 1), y.dtype)
    with pytest.raises(exc, match=match):
        _fastpath(tm, y, D, alpha, x=x, **kw)


# ---- argument checks -----------------------------------------------------------------------------------------------------
@pytest.mark.parametrize('method', GREEDY)
def test_errors_before_any_gpu_call(no_gpu, method):
    from decomp_amd import template_matching as tm
    from decomp_amd.utils.assertion import DimInvalidError
    from decomp_amd.utils.exceptions import DtypeMismatchError
    y, D = _problem()
    ok = dict(lasso_method=method, lasso_iter=3, lasso_tol=None)
    # y: 2 or 3 dimensions, Ch channels
    _both(tm, DimInvalidError, y[0, 0], D, 0, match='dimension', **ok)
    _both(tm, DimInvalidError, y[None], D, 0, match='dimension', **ok)
    _both(tm, DimInvalidError, y[:, :2], D, 0, match='channels', **ok)
    _both(tm, DimInvalidError, y[0, :2], D, 0, match='channels', **ok)
    # D: [T, S] or [T, Ch, S], Ch >= 1 (the rules of _channels)
    _both(tm, ValueError, y[:, :0], D[:, :0], 0, match='Ch >= 1', **ok)
    _both(tm, DimInvalidError, y, D[None], 0, match='2 .* or 3', **ok)
    _both(tm, DimInvalidError, y, D[0, 0], 0, match='2 .* or 3', **ok)
    # the checks of the 2-D greedy solve, on S = D.shape[-1] = 5 and C = 34
    for alpha in (0.1, -1.0, None, '0'):
        _both(tm, ValueError, y, D, alpha, match='alpha must be 0', **ok)
    for n in (0, -1, 69, 2.0, True, '3'):                                   # T C = 68
        _both(tm, ValueError, y, D, 0, match='n_nonzero_coefs', **dict(ok, lasso_iter=n))
    _both(tm, ValueError, y, D, 0, match='lasso_iter', **dict(ok, lasso_iter=None))
    for tol in (-1.0, float('nan'), 'x', True):
        _both(tm, ValueError, y, D, 0, **dict(ok, lasso_tol=tol))
    for stride in (0, -1, 1.5, None):
        _both(tm, ValueError, y, D, 0, stride=stride, **ok)
    _both(tm, ValueError, y, D, 0, padding='FULL', **ok)
    _both(tm, ValueError, y[..., :4], D, 0, **ok)                           # S = 5 > N = 4 (Ch = 3 < 5 is not S)
    _both(tm, ValueError, y, D, 0, match='n_nonzero_coefs', minibatch=3, size_of_minibatch=10, padding='VALID',
          **dict(ok, lasso_iter=13))                                        # a window: C = 6, T C = 12
    with pytest.raises(NotImplementedError, match='mask'):
        tm.solve(y, D, 0, mask=np.ones_like(y), **ok)
    with pytest.raises(NotImplementedError, match='mask'):
        _fastpath(tm, y, D, 0, mask=np.ones_like(y), **ok)
    with pytest.raises(ValueError, match='size_of_minibatch'):
        tm.solve(y, D, 0, minibatch=3, **ok)
    with pytest.raises(DtypeMismatchError):
        tm.solve(y, D.astype(np.float64), 0, **ok)
    # the loops themselves check too
    x = np.zeros((4, 2, 34), np.float32)
    with pytest.raises(ValueError, match='alpha must be 0'):
        tm.solve_batch(y, D, 0.1, x, 1, 'SAME', 1e-4, 3, method, 3, None, None)
    with pytest.raises(ValueError, match='n_nonzero_coefs'):
        tm.solve_minibatch(y, D, 0, x, 1, 'SAME', 1e-4, 3, 10, 3, method, 1000, None, np.random.RandomState(0), None)


@pytest.mark.parametrize('method', ['ista', 'acc_ista', 'fista', 'fista_pos', 'cd', 'parallel_cd', 'admm', 'nonsense'])
def test_lasso_coders_have_no_multichannel_form(no_gpu, method):
    from decomp_amd import template_matching as tm
    y, D = _problem()
    _both(tm, NotImplementedError, y, D, 0.1, match='multichannel', lasso_method=method)


@pytest.mark.parametrize('dt,cap', [(np.float32, 64), (np.float64, 64), (np.complex64, 32), (np.complex128, 32)])
def test_omp_cap_and_positive(no_gpu, dt, cap):
    from decomp_amd import template_matching as tm
    y, D = _problem(dt)                                                     # T C = 68 > cap
    _both(tm, ValueError, y, D, 0, match='cap', lasso_method='omp', lasso_iter=cap + 1, lasso_tol=None)
    with pytest.raises(AssertionError, match='GPU call'):
        tm.solve(y, D, 0, lasso_method='omp', lasso_iter=cap, lasso_tol=None)
    with pytest.raises(AssertionError, match='GPU call'):                   # plain pursuit has no cap
        tm.solve(y, D, 0, lasso_method='mp', lasso_iter=cap + 1, lasso_tol=None)
    if np.dtype(dt).kind == 'c':
        _both(tm, ValueError, y, D, 0, match='real dtype', lasso_method='mp_pos', lasso_iter=3, lasso_tol=None)


def test_valid_calls_reach_the_gpu(no_gpu):
    from decomp_amd import template_matching as tm
    y, D = _problem()
    for kw in (dict(lasso_method='omp', lasso_iter=64, lasso_tol=None), dict(lasso_method='mp', lasso_iter=68),
               dict(lasso_method='mp_pos', lasso_iter=None, lasso_tol=0.5),
               dict(lasso_method='omp', lasso_iter=np.int64(3), lasso_tol=0.0, stride=2, padding='VALID'),
               dict(lasso_method='mp', lasso_iter=2, minibatch=3, size_of_minibatch=10)):
        with pytest.raises(AssertionError, match='GPU call'):
            tm.solve(y, D, 0, **kw)
    with pytest.raises(AssertionError, match='GPU call'):                   # one signal [Ch, N]
        tm.solve(y[0], D, 0, lasso_method='omp', lasso_iter=3, lasso_tol=None)
    with pytest.raises(AssertionError, match='GPU call'):                   # Ch = 1
        tm.solve(y[:, :1], D[:, :1], 0, lasso_method='omp', lasso_iter=3, lasso_tol=None)


def test_multichannel_loops_call_the_mc_coder_and_the_mc_event_step(monkeypatch):
    """What reaches the library for a 3-D D, recorded without a GPU: per outer iteration one mc coder call and one
    mc_dstep_events with max_events = min(s, C); the minibatch loop gathers with mc_gather_windows and scatters with the
    one-channel scatter_windows; the sums are XXt [T S, T S] and yX [T Ch S]."""
    import torch
    from decomp_amd import template_matching as tm, _arrays
    calls = []

    def to_device(a, device=None, copy=False):
        t = a if _arrays.is_torch(a) else torch.from_numpy(np.ascontiguousarray(a))
        return t.clone() if copy else t.contiguous()

    def record(t, name, *args):
        calls.append((name, [a for a in args if not _arrays.is_torch(a)],
                      [tuple(a.shape) for a in args if _arrays.is_torch(a)]))
    monkeypatch.setattr(_arrays, 'to_device', to_device)
    monkeypatch.setattr(tm, '_call', record)
    monkeypatch.setattr(tm.normalize, 'l2_strict', lambda U, axis=-1: U)         # (a library call too)
    y, D = _problem()
    for method, name, flags in (('omp', 'mc_omp', []), ('mp', 'mc_pursuit', [0]), ('mp_pos', 'mc_pursuit', [1])):
        del calls[:]
        it, Dn, x = tm.solve(y, D, 0, maxiter=3, tol=0, lasso_method=method, lasso_iter=5, lasso_tol=0.25)
        assert it == 3 and x.shape == (4, 2, 34) and Dn.shape == D.shape
        assert [c[0] for c in calls] == [name, 'mc_dstep_events'] * 2
        coder, step = calls[0][1], calls[1][1]
        assert coder[:9] == [4, 2, 3, 5, 30, 1, 1, 5, 0.25] and coder[9:-1] == flags
        assert step[:-1] == [4, 2, 3, 5, 30, 1, 1, 0, 5]
        assert calls[1][2] == [(4, 3, 30), (4, 2, 34), (2, 3, 5), (10, 10), (30,)]       # y, x, D, XXt, yX
    del calls[:]
    it, _, x = tm.solve(y[0], D, 0, maxiter=2, tol=0, lasso_method='mp', lasso_iter=40, lasso_tol=None)
    assert x.shape == (2, 34) and calls[0][1][:2] == [1, 2] and calls[1][1][8] == 34     # B = 1; max_events = C
    del calls[:]
    tm.solve(y, D, 0, maxiter=3, tol=0, lasso_method='mp', lasso_iter=4, minibatch=3, size_of_minibatch=10,
             random_seed=0)
    assert [c[0] for c in calls] == ['mc_gather_windows', 'mc_pursuit', 'scatter_windows', 'mc_dstep_events'] * 2
    assert calls[0][1] == [3, 4, 2, 3, 5, 30, 10, 1, 1] and calls[0][2][-2:] == [(3, 3, 10), (3, 2, 14)]
    assert calls[1][1][:8] == [3, 2, 3, 5, 10, 1, 1, 4]
    assert calls[2][1] == [3, 4, 2, 5, 30, 10, 1, 1]
    assert [calls[3][1][7], calls[7][1][7]] == [1, 2] and calls[3][1][8] == 4            # acc_it, max_events


# ---- the C ABI lists the new entries ----------------------------------------------------------------------------------
def test_header_bindings_and_library_list_the_entries():
    from decomp_amd import _hip
    text = open(os.path.join(ROOT, 'include', 'decomp_hip.h')).read()
    lib = _hip.load()
    for sfx in ('f32', 'f64', 'c64', 'c128'):
        name = 'dcp_tm_mc_dstep_events_' + sfx
        assert re.search(r'\bint %s\(dcp_handle\* h, const void\* Y, const void\* X, void\* D, void\* XXt, void\* yX, '
                         r'int64_t B, int64_t T, int64_t Ch, int64_t S, int64_t N, int64_t stride, int padding, '
                         r'int acc_it, int64_t max_events, double\* maxdiff\);' % name, text)
        res, args = _hip.SIGNATURES[name]
        one = _hip.SIGNATURES['dcp_tm_dstep_events_' + sfx][1]
        assert res is ctypes.c_int and args == one[:8] + [ctypes.c_int64] + one[8:]
        assert hasattr(lib, name)
        out = ctypes.c_double(0.0)
        # no handle: DCP_ERR_INVALID, never a crash
        assert getattr(lib, name)(None, None, None, None, None, None, 1, 1, 1, 1, 1, 1, 1, 0, 1,
                                  ctypes.byref(out)) == -1
        name = 'dcp_tm_mc_gather_windows_' + sfx
        assert re.search(r'\bint %s\(dcp_handle\* h, const void\* Y, const void\* X, const int64_t\* idx_b, '
                         r'const int64_t\* idx_n, int64_t m, int64_t B, int64_t T, int64_t Ch, int64_t S, int64_t N, '
                         r'int64_t w, int64_t stride, int padding, void\* Yw, void\* Xw\);' % name, text)
        res, args = _hip.SIGNATURES[name]
        one = _hip.SIGNATURES['dcp_tm_gather_windows_' + sfx][1]
        assert res is ctypes.c_int and args == one[:8] + [ctypes.c_int64] + one[8:]
        assert getattr(lib, name)(None, None, None, None, None, 1, 1, 1, 1, 1, 1, 1, 1, 1, None, None) == -1
    doc = open(os.path.join(ROOT, 'INTEGRATION.md')).read()
    assert 'dcp_tm_mc_dstep_events_' in doc and 'dcp_tm_mc_gather_windows_' in doc


# ---- the reference loop -------------------------------------------------------------------------------------------------
def _valid_problem(cplx):
    """A small 'VALID' problem with stride 2: (y [B, Ch, N], D0 [T, Ch, S], stride, nev)."""
    B, T, Ch, S, N, stride, nev = 12, 2, 3, 6, 48, 2, 3
    y, D, _ = mc.make_problem(210 + cplx, B, T, Ch, S, N, stride, 'VALID', nev, cplx)
    rng = np.random.RandomState(7)
    e = rng.randn(T, Ch, S) + (1j * rng.randn(T, Ch, S) if cplx else 0)
    return y, ref.normalize_templates(D) + 0.5 * e / np.sqrt(Ch * S), stride, nev


@pytest.mark.parametrize('coder', ['omp', 'mp'])
@pytest.mark.parametrize('cplx', [False, True])
def test_reference_loop_is_the_one_channel_loop_on_the_interleaved_problem(cplx, coder):
    """'VALID': with the channels interleaved into one signal (y'[n Ch + ch] = y[ch, n], D'[t, k Ch + ch] = D[t, ch, k])
    and stride Ch s, the one-channel problem is this one -- its XXt [(T Ch S)^2] is the block-diagonal operator, its row
    norm the joint one over Ch S.  Four iterations of tm_learn_ref.solve_batch on it give, de-interleaved, the D and x
    of tm_mc_learn_ref.solve_batch to 1e-10 in double (the sums differ in their order only)."""
    y, D0, stride, nev = _valid_problem(cplx)
    Ch = D0.shape[1]
    trace, trace1 = [], []
    it, D, x = ref.solve_batch(y, D0, stride, 'VALID', coder, nev, None, 0.0, 5, trace)
    y1, D1 = mc.interleave(y, D0)
    it1, Dl, x1 = tm_learn_ref.solve_batch(y1, D1, Ch * stride, 'VALID', coder, nev, None, 0.0, 5, trace1)
    assert it == it1 == 5 and x.shape == x1.shape and np.count_nonzero(x) > 0
    _, Dl = mc.deinterleave(y1, Dl, Ch)
    assert D.dtype == Dl.dtype and np.max(np.abs(D - Dl)) <= 1e-10
    assert np.max(np.abs(x - x1)) <= 1e-10 * np.max(np.abs(x))
    assert np.max(np.abs(np.array(trace) - np.array(trace1))) <= 1e-10
    assert np.all(np.linalg.norm(D.reshape(D.shape[0], -1), axis=1) <= 1.0 + 1e-12)       # |D_t|^2 <= 1 over Ch S


def test_reference_statistics_and_update_keep_the_dtype():
    y, D0, (stride, padding), nev = ref.planted(2)
    for dt in (np.complex64, np.complex128):
        yd, Dd = y.astype(dt), ref.normalize_templates(D0.astype(dt))
        x = ref.code('omp', yd, Dd, y.shape[-1], stride, padding, nev)
        XXt, yX = ref.statistics(yd, x, D0.shape[-1], stride, padding)
        Dn, diff = ref.d_update(Dd, XXt, yX)
        T, Ch, S = D0.shape
        assert XXt.shape == (T * S, T * S) and yX.shape == (T * Ch * S,)
        assert x.dtype == XXt.dtype == yX.dtype == Dn.dtype == dt and diff > 0


@pytest.mark.parametrize('problem', [0, 1, 2])
def test_reference_loop_learns_the_planted_templates(problem):
    """10 outer iterations of tm_mc_learn_ref.solve_batch with 'omp' from the disturbed templates at least halve the
    residual (coded_residual: the median |y - x * D| / |y| over all channels of a fresh code on D); on the two real
    problems they reach the noise level 0.05.  Observed on the CPU (start; after 10 iterations in double, in single):
      problem 0 (real, stride 1, Ch 3)      0.450770    0.04978088    0.04978089   (single - double: +6.3e-09)
      problem 1 (real, stride 2, Ch 2)      0.486271    0.04931927    0.04931928   (single - double: +1.1e-08)
      problem 2 (complex, 'VALID', Ch 4)    0.553198    0.06972247    0.06972247   (single - double: +1.8e-10)"""
    start, r64 = ref.planted_run(problem, 'double')
    _, r32 = ref.planted_run(problem, 'single')
    print('problem %d: start %.6f, double %.8f, single %.8f (single - double %.1e)' % (problem, start, r64, r32,
                                                                                       r32 - r64))
    assert r64 <= 0.5 * start and r32 <= 0.5 * start
    if problem < 2:
        assert r64 < 0.05


def test_reference_minibatch_loop_accumulates_the_running_sums():
    y, D0, (stride, padding), nev = ref.planted(0)
    trace = []
    it, D, x = ref.solve_minibatch(y, D0, stride, padding, 'omp', nev, None, 0.0, 8, 60, 4, np.random.RandomState(5),
                                   trace)
    assert it == 4 and len(trace) == 3 and np.all(np.isfinite(D)) and D.shape == D0.shape
    assert 0 < np.count_nonzero(x) <= 3 * 8 * nev
    for coder in ('mp', 'mp_pos'):
        it, D, x = ref.solve_batch(y[:4], D0, stride, padding, coder, nev, None, 0.0, 3)
        assert it == 3 and np.count_nonzero(x.reshape(4, -1), axis=1).max() <= nev
        if coder == 'mp_pos':
            assert x.min() >= 0
