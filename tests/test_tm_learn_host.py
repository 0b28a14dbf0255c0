"""CPU: template_matching.solve with a greedy coder (lasso_method 'omp', 'mp', 'mp_pos') -- its argument checks run
before any GPU call; header, bindings and library list dcp_tm_dstep_events_*; and the NumPy loop of tm_learn_ref.py, the
yardstick of the GPU tests, learns the planted templates."""
import ctypes
import os
import re

import numpy as np
import pytest

import tm_learn_ref as ref

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
GREEDY = ('omp', 'mp', 'mp_pos')


@pytest.fixture
def no_gpu(monkeypatch):
    from decomp_amd import _arrays, _hip

    def boom(*a, **k):
        raise AssertionError('a GPU call was made before the argument check')
    monkeypatch.setattr(_arrays, 'to_device', boom)
    monkeypatch.setattr(_hip, 'load', boom)


def _problem(dtype=np.float32, N=30):
    rng = np.random.RandomState(0)
    return rng.randn(4, N).astype(dtype), rng.randn(2, 5).astype(dtype)     # N = 30: C = 34 ('SAME'), T C = 68


def _fastpath(tm, y, D, alpha, x=None, minibatch=None, size_of_minibatch=None, stride=1, padding='SAME', **kw):
    return tm.solve_fastpath(y, D, alpha, x, stride, padding, 1e-4, minibatch, size_of_minibatch, 5,
                             kw['lasso_method'], kw.get('lasso_iter', 10), kw.get('lasso_tol', 1e-5),
                             np.random.RandomState(0), None)


def _both(tm, exc, y, D, alpha, match=None, **kw):
    """solve and solve_fastpath raise exc before any GPU call."""
    with pytest.raises(exc, match=match):
        tm.solve(y, D, alpha, **kw)
    x = np.zeros((y.shape[0], D.shape[0], 1), y.dtype)
    with pytest.raises(exc, match=match):
        _fastpath(tm, y, D, alpha, x=x, **kw)


@pytest.mark.parametrize('method', GREEDY)
def test_errors_before_any_gpu_call(no_gpu, method):
    from decomp_amd import template_matching as tm
    from decomp_amd.utils.exceptions import DtypeMismatchError
    y, D = _problem()
    ok = dict(lasso_method=method, lasso_iter=3, lasso_tol=None)
    for alpha in (0.1, -1.0, 1e-300, None, '0', np.zeros(2)):
        _both(tm, ValueError, y, D, alpha, match='alpha must be 0', **ok)
    for n in (0, -1, 69, 2.0, True, '3'):                                   # T C = 68
        _both(tm, ValueError, y, D, 0, match='n_nonzero_coefs', **dict(ok, lasso_iter=n))
    _both(tm, ValueError, y, D, 0, match='lasso_iter', **dict(ok, lasso_iter=None))      # neither a count nor a tol
    for tol in (-1.0, float('nan'), float('inf'), 'x', True):
        _both(tm, ValueError, y, D, 0, **dict(ok, lasso_tol=tol))
        _both(tm, ValueError, y, D, 0, **dict(ok, lasso_iter=None, lasso_tol=tol))
    for stride in (0, -1, 1.5, None):
        _both(tm, ValueError, y, D, 0, stride=stride, **ok)
    _both(tm, ValueError, y, D, 0, padding='FULL', **ok)
    _both(tm, ValueError, y[:, :4], D, 0, **ok)                             # S > N
    # a window is what the coder sees: its T C bounds lasso_iter ('VALID': C = 6 for 10 samples)
    _both(tm, ValueError, y, D, 0, match='n_nonzero_coefs', minibatch=3, size_of_minibatch=10, padding='VALID',
          **dict(ok, lasso_iter=13))
    with pytest.raises(NotImplementedError):
        tm.solve(y, D, 0, mask=np.ones_like(y), **ok)
    with pytest.raises(ValueError, match='size_of_minibatch'):
        tm.solve(y, D, 0, minibatch=3, **ok)
    with pytest.raises(DtypeMismatchError):
        tm.solve(y, D.astype(np.float64), 0, **ok)
    with pytest.raises(DtypeMismatchError):
        tm.solve(y, D, 0, x=np.zeros((4, 2, 34), np.float64), **ok)
    # the loops themselves check too
    x = np.zeros((4, 2, 34), np.float32)
    with pytest.raises(ValueError, match='alpha must be 0'):
        tm.solve_batch(y, D, 0.1, x, 1, 'SAME', 1e-4, 3, method, 3, None, None)
    with pytest.raises(ValueError, match='n_nonzero_coefs'):
        tm.solve_minibatch(y, D, 0, x, 1, 'SAME', 1e-4, 3, 10, 3, method, 1000, None, np.random.RandomState(0), None)


@pytest.mark.parametrize('dt,cap', [(np.float32, 64), (np.float64, 64), (np.complex64, 32), (np.complex128, 32)])
def test_omp_one_past_the_cap_is_a_value_error(no_gpu, dt, cap):
    from decomp_amd import template_matching as tm
    y, D = _problem(dt)                                                     # T C = 68 > cap
    _both(tm, ValueError, y, D, 0, match='cap', lasso_method='omp', lasso_iter=cap + 1, lasso_tol=None)
    with pytest.raises(AssertionError, match='GPU call'):
        tm.solve(y, D, 0, lasso_method='omp', lasso_iter=cap, lasso_tol=None)
    with pytest.raises(AssertionError, match='GPU call'):                   # plain pursuit has no cap
        tm.solve(y, D, 0, lasso_method='mp', lasso_iter=cap + 1, lasso_tol=None)


@pytest.mark.parametrize('dt', [np.complex64, np.complex128])
def test_mp_pos_needs_a_real_dtype(no_gpu, dt):
    from decomp_amd import template_matching as tm
    y, D = _problem(dt)
    _both(tm, ValueError, y, D, 0, match='real dtype', lasso_method='mp_pos', lasso_iter=3, lasso_tol=None)


def test_valid_calls_reach_the_gpu(no_gpu):
    from decomp_amd import template_matching as tm
    y, D = _problem()
    for kw in (dict(lasso_method='omp', lasso_iter=64, lasso_tol=None), dict(lasso_method='mp', lasso_iter=68),
               dict(lasso_method='mp_pos', lasso_iter=None, lasso_tol=0.5),
               dict(lasso_method='omp', lasso_iter=np.int64(3), lasso_tol=0.0, stride=2, padding='VALID'),
               dict(lasso_method='mp', lasso_iter=2, minibatch=3, size_of_minibatch=10)):
        for alpha in (0, 0.0, np.float32(0)):
            with pytest.raises(AssertionError, match='GPU call'):
                tm.solve(y, D, alpha, **kw)
    with pytest.raises(AssertionError, match='GPU call'):
        tm.solve(y[0], D, 0, lasso_method='omp', lasso_iter=3, lasso_tol=None)
    # the other methods are not touched by the new checks
    with pytest.raises(AssertionError, match='GPU call'):
        tm.solve(y, D, 0.1, lasso_method='acc_ista', lasso_iter=10.5)


def test_greedy_loops_call_the_coder_and_the_event_step(monkeypatch):
    """What reaches the library, recorded without a GPU: per outer iteration one coder call with (n_steps, tol, flags)
    and one dstep_events with max_events = min(s, C); the other methods still make lasso + dstep."""
    import torch
    from decomp_amd import template_matching as tm, _arrays
    calls = []

    def to_device(a, device=None, copy=False):
        t = a if _arrays.is_torch(a) else torch.from_numpy(np.ascontiguousarray(a))
        return t.clone() if copy else t.contiguous()

    def record(t, name, *args):
        calls.append((name, [a for a in args if not _arrays.is_torch(a)]))
    monkeypatch.setattr(_arrays, 'to_device', to_device)
    monkeypatch.setattr(tm, '_call', record)
    monkeypatch.setattr(tm.normalize, 'l2_strict', lambda U, axis=-1: U)         # (a library call too)
    y, D = _problem()
    for method, name, flags in (('omp', 'omp', []), ('mp', 'pursuit', [0]), ('mp_pos', 'pursuit', [1])):
        del calls[:]
        it, _, x = tm.solve(y, D, 0, maxiter=3, tol=0, lasso_method=method, lasso_iter=5, lasso_tol=0.25)
        assert it == 3 and x.shape == (4, 2, 34)
        assert [c[0] for c in calls] == [name, 'dstep_events'] * 2
        coder, step = calls[0][1], calls[1][1]
        assert coder[:8] == [4, 2, 5, 30, 1, 1, 5, 0.25] and coder[8:-1] == flags
        assert step[:-1] == [4, 2, 5, 30, 1, 1, 0, 5]
    del calls[:]
    tm.solve(y, D, 0, maxiter=3, tol=0, lasso_method='mp', lasso_iter=40, lasso_tol=None)
    assert calls[0][1][6:8] == [40, -1.0] and calls[1][1][7] == 34          # max_events = C
    del calls[:]
    tm.solve(y, D, 0, maxiter=3, tol=0, lasso_method='mp', lasso_iter=4, minibatch=3, size_of_minibatch=10,
             random_seed=0)
    assert [c[0] for c in calls] == ['gather_windows', 'pursuit', 'scatter_windows', 'dstep_events'] * 2
    assert calls[1][1][:7] == [3, 2, 5, 10, 1, 1, 4]
    assert [calls[3][1][6], calls[7][1][6]] == [1, 2] and calls[3][1][7] == 4       # acc_it, max_events
    del calls[:]
    tm.solve(y, D, 0.1, maxiter=3, tol=0)
    assert [c[0] for c in calls] == ['lasso', 'dstep'] * 2


# ---- the C ABI lists the new entries ----------------------------------------------------------------------------------
def test_header_bindings_and_library_list_the_entries():
    from decomp_amd import _hip
    text = open(os.path.join(ROOT, 'include', 'decomp_hip.h')).read()
    lib = _hip.load()
    for sfx in ('f32', 'f64', 'c64', 'c128'):
        name = 'dcp_tm_dstep_events_' + sfx
        assert re.search(r'\bint %s\(dcp_handle\* h, const void\* Y, const void\* X, void\* D, void\* XXt, void\* yX, '
                         r'int64_t B, int64_t T, int64_t S, int64_t N, int64_t stride, int padding, int acc_it, '
                         r'int64_t max_events, double\* maxdiff\);' % name, text)
        res, args = _hip.SIGNATURES[name]
        dense = _hip.SIGNATURES['dcp_tm_dstep_' + sfx][1]
        assert res is ctypes.c_int and len(args) == 15
        assert args[:13] == dense[:13] and args[13] is ctypes.c_int64 and args[14] == dense[13]
        assert hasattr(lib, name)
        out = ctypes.c_double(0.0)
        # no handle: DCP_ERR_INVALID, never a crash
        assert getattr(lib, name)(None, None, None, None, None, None, 1, 1, 1, 1, 1, 1, 0, 1, ctypes.byref(out)) == -1
    doc = open(os.path.join(ROOT, 'INTEGRATION.md')).read()
    assert 'dcp_tm_dstep_events_' in doc


# ---- the reference loop -------------------------------------------------------------------------------------------------
@pytest.mark.parametrize('problem', [0, 1, 2])
def test_reference_loop_learns_the_planted_templates(problem):
    """10 outer iterations of tm_learn_ref.solve_batch with 'omp' from the disturbed templates at least halve the
    residual (tm_learn_ref.coded_residual, the median |y - x * D| / |y| of a fresh code on D); on the two real problems
    they reach the noise level 0.05.  Observed on the CPU (start; after 10 iterations in double, in single):
      problem 0 (real, stride 1)      0.488075    0.04886670    0.04886670   (single - double: -2.3e-09)
      problem 1 (real, stride 2)      0.346323    0.04887592    0.04887592   (single - double: -4.2e-10)
      problem 2 (complex, 'VALID')    0.534393    0.08043644    0.08043644   (single - double: +8.1e-09)
    and problem 2 after 30 iterations in double: 0.06840934."""
    start, r64 = ref.planted_run(problem, 'double')
    _, r32 = ref.planted_run(problem, 'single')
    print('problem %d: start %.6f, double %.8f, single %.8f (single - double %.1e)' % (problem, start, r64, r32,
                                                                                       r32 - r64))
    assert r64 <= 0.5 * start and r32 <= 0.5 * start
    if problem < 2:
        assert r64 < 0.05


def test_reference_minibatch_loop_accumulates_the_running_sums():
    """solve_minibatch of the reference: the draws are minibatch_index's, x holds the codes of the windows drawn, and
    with one window covering the whole signal set it is solve_batch with the statistics averaged as 1 / it."""
    y, D0, (stride, padding), nev = ref.planted(0)
    trace = []
    it, D, x = ref.solve_minibatch(y, D0, stride, padding, 'omp', nev, None, 0.0, 8, 60, 4, np.random.RandomState(5),
                                   trace)
    assert it == 4 and len(trace) == 3 and np.all(np.isfinite(D))
    assert 0 < np.count_nonzero(x) <= 3 * 8 * nev
    for coder in ('mp', 'mp_pos'):
        it, D, x = ref.solve_batch(y[:4], D0, stride, padding, coder, nev, None, 0.0, 3)
        assert it == 3 and np.count_nonzero(x.reshape(4, -1), axis=1).max() <= nev
        if coder == 'mp_pos':
            assert x.min() >= 0
