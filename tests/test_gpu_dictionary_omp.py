"""GPU: dictionary_learning.solve(lasso_method='omp') -- orthogonal matching pursuit as the inner coder of the
dictionary step -- against the CPU oracle loop with omp_ref.solve_fastpath_omp patched in (double precision), by its
properties (single precision), through the in-core and the out-of-core loop, and its refusals."""
import ctypes
import types

import numpy as np
import pytest

import omp_ref

pytestmark = pytest.mark.gpu

N, F, K, S = 120, 20, 6, 2
KW = dict(tol=0.0, minibatch=40, maxiter=3, lasso_method='omp', lasso_iter=S, random_seed=7)


def _err(a, b):
    return float(np.max(np.abs(np.asarray(a) - np.asarray(b)))) / max(1.0, float(np.max(np.abs(b))))


def _problem(dt):
    dt = np.dtype(dt)
    cplx = dt.kind == 'c'
    rng = np.random.RandomState(5)

    def randn(*s):
        return rng.randn(*s) + 1j * rng.randn(*s) if cplx else rng.randn(*s)
    Dt = randn(K, F)
    x0 = np.zeros((N, K))
    for i in range(N):
        x0[i, rng.choice(K, S, replace=False)] = (1 + rng.rand(S)) * rng.choice([-1, 1], S)
    y = x0 @ Dt + 0.05 * randn(N, F)
    D0 = Dt + 0.3 * randn(K, F)
    return y.astype(dt), D0.astype(dt)


def _oracle(monkeypatch, y, D0, lasso_tol):
    from oracle import dictionary_learning as odl
    monkeypatch.setattr(odl, 'lasso', types.SimpleNamespace(solve_fastpath=omp_ref.solve_fastpath_omp))
    return odl.solve(y.copy(), D0.copy(), 0.0, lasso_tol=-1.0 if lasso_tol is None else lasso_tol, **KW)


@pytest.mark.parametrize('lasso_tol', [None, 'spread'])
@pytest.mark.parametrize('dt', ['float64', 'complex128'])
def test_double_precision_equals_the_oracle_loop(monkeypatch, dt, lasso_tol):
    """it equal; D and x to the tolerance of test_gpu_dictionary.py's double-precision golden cases (1e-7).
    'spread': a residual tolerance of 0.3 median|y|^2, at which some rows stop after one atom."""
    from decomp_amd import dictionary_learning as dl
    y, D0 = _problem(dt)
    if lasso_tol == 'spread':
        lasso_tol = 0.3 * float(np.median(np.sum(np.abs(y) ** 2, axis=1)))
    it_o, D_o, x_o = _oracle(monkeypatch, y, D0, lasso_tol)
    it, D, x = dl.solve(y.copy(), D0.copy(), 0.0, lasso_tol=lasso_tol, **KW)
    print(dt, lasso_tol, 'it', it, it_o, 'err D %.3g x %.3g' % (_err(D, D_o), _err(x, x_o)),
          'nnz', sorted(set(np.count_nonzero(x, axis=1).tolist())))
    assert it == it_o
    assert D.dtype == y.dtype and x.shape == (N, K)
    assert np.all(np.count_nonzero(x, axis=1) <= S)
    assert np.array_equal(x != 0, x_o != 0)
    assert _err(D, D_o) < 1e-7 and _err(x, x_o) < 1e-7
    if lasso_tol is not None:
        assert len(set(np.count_nonzero(x, axis=1).tolist())) >= 2


@pytest.mark.parametrize('dt', ['float32', 'complex64'])
def test_single_precision_properties(dt):
    from decomp_amd import dictionary_learning as dl
    y, D0 = _problem(dt)
    it, D, x = dl.solve(y.copy(), D0.copy(), 0.0, lasso_tol=None, **KW)
    assert D.dtype == y.dtype and x.dtype == y.dtype
    assert np.all(np.isfinite(D)) and np.all(np.isfinite(x))
    nnz = np.count_nonzero(x, axis=1)
    assert np.all(nnz <= S) and np.all(nnz >= 1)
    # the start: the codes of the first pass on the normalised initial dictionary
    from decomp_amd import omp
    Dn = D0 / np.linalg.norm(D0, axis=1, keepdims=True)
    _, xs = omp.solve(y, Dn, n_nonzero_coefs=S)
    start = np.linalg.norm(y - xs @ Dn)
    end = np.linalg.norm(y - x @ D)
    print(dt, 'residual %.4g -> %.4g' % (start, end))
    assert end < start


@pytest.mark.parametrize('dt', ['float64', 'complex64'])
def test_out_of_core_loop_equals_in_core(dt):
    import torch
    from decomp_amd import dictionary_learning as dl
    y, D0 = _problem(dt)
    x0 = np.zeros((N, K), dtype=y.dtype)        # a host x: with a device D it is streamed like y (and not read)
    it0, D_in, x_in = dl.solve(y, D0.copy(), 0.0, x0.copy(), lasso_tol=None, **KW)
    it1, D_st, x_st = dl.solve(y, torch.from_numpy(D0).cuda(), 0.0, x0.copy(), lasso_tol=None, **KW)
    assert it0 == it1
    assert isinstance(x_st, np.ndarray) and torch.is_tensor(D_st)
    assert np.array_equal(D_st.cpu().numpy(), D_in)
    assert np.array_equal(x_st, x_in)
    assert np.all(np.count_nonzero(x_st, axis=1) <= S) and np.count_nonzero(x_st) > 0


def test_refusals():
    from decomp_amd import dictionary_learning as dl, sharded
    y, D0 = _problem('float32')
    with pytest.raises(ValueError):
        dl.solve(y, D0.copy(), 0.1, lasso_tol=None, **KW)
    with pytest.raises(NotImplementedError):
        dl.solve(y, D0.copy(), 0.0, lasso_tol=None, mask=np.ones(y.shape, dtype=np.float32), **KW)
    with pytest.raises(NotImplementedError):
        sharded.dictionary_learning_sharded(y, D0.copy(), 0.0, lasso_tol=None, **KW)


def test_step_entry_rejects_positive_mask_and_bad_sparsity():
    """DCP_LASSO_OMP | DCP_LASSO_POSITIVE, the masked step and a sparsity outside [1, min(K, cap)] are
    DCP_ERR_INVALID with a message; the plain code runs and reports the step count."""
    import torch
    from decomp_amd import _arrays, _hip
    y, D0 = _problem('float32')
    Y = torch.from_numpy(y[:40]).cuda()
    D = torch.from_numpy(D0).cuda()
    _arrays.l2_normalize_(D, strict=True)
    lib, h = _arrays.lib_handle(D)

    def step(code, s, name='dcp_dict_step_f32', mask=None):
        x = torch.ones((40, K), device='cuda')
        A = torch.zeros((K, K), device='cuda')
        B = torch.zeros((K, F), device='cuda')
        A3 = torch.zeros((K, F, K), device='cuda')
        Dn = torch.empty_like(D)
        md, lit = ctypes.c_double(0), ctypes.c_int(-5)
        if mask is None:
            rc = getattr(lib, name)(h, _arrays.ptr(Y), _arrays.ptr(x), _arrays.ptr(D), _arrays.ptr(Dn), _arrays.ptr(A),
                                    _arrays.ptr(B), 40, F, K, -39.0, 0.0, code, s, -1.0, ctypes.byref(md),
                                    ctypes.byref(lit))
        else:
            rc = lib.dcp_dict_mask_step_f32(h, _arrays.ptr(Y), _arrays.ptr(mask), _arrays.ptr(x), _arrays.ptr(D),
                                            _arrays.ptr(Dn), _arrays.ptr(A3), _arrays.ptr(B), 40, F, K, -39.0, 0.0,
                                            code, s, -1.0, ctypes.byref(md), ctypes.byref(lit))
        return rc, lit.value, x

    rc, lit, x = step(_hip.LASSO_OMP, S)
    assert rc == 0 and lit == S
    assert np.all(np.count_nonzero(x.cpu().numpy(), axis=1) == S)
    assert step(_hip.LASSO_OMP | _hip.LASSO_POSITIVE, S)[0] == -1
    for s in (0, K + 1, 65):
        assert step(_hip.LASSO_OMP, s)[0] == -1
        assert b'omp' in lib.dcp_last_error_string(h)
    assert step(_hip.LASSO_OMP, S, mask=torch.ones((40, F), device='cuda'))[0] == -1
    assert b'mask' in lib.dcp_last_error_string(h)
