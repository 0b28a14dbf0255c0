"""CPU: the NumPy restatements of convolutional matching pursuit (tests/tm_pursuit_ref.py) agree with each other, with
plain matching pursuit on the dense operator and with the exact dyadic case; the argument checks of
template_matching.pursuit run before any GPU call; header, bindings and library list the new entries."""
import ctypes
import inspect
import os
import re

import numpy as np
import pytest

import tm_pursuit_ref as ref
from oracle import template_matching as otm

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


# ---- the restatements ---------------------------------------------------------------------------------------------
@pytest.mark.parametrize('cplx', [False, True])
@pytest.mark.parametrize('case', [0, 1, 2, 3, 4, 5, 6])
def test_residual_and_gram_forms_agree_in_double(case, cplx):
    B, T, S, N, stride, padding, nev = ref.CASES[case]
    y, D = ref.case_problem(case, cplx)
    y = y[:8]
    for kw in (dict(n=nev), dict(tol=ref.case_tol(case, cplx))):
        x, steps, margin, _ = ref.mp_residual(y, D, N, stride, padding, **kw)
        xg, sg = ref.mp_gram(y, D, N, stride, padding, **kw)
        keep = margin >= 1e-8
        assert keep.sum() >= 6
        assert np.array_equal(steps[keep], sg[keep])
        assert np.max(np.abs(x - xg)[keep]) <= 1e-10 * np.max(np.abs(x))


@pytest.mark.parametrize('cplx', [False, True])
@pytest.mark.parametrize('stride,padding', [(1, 'SAME'), (2, 'SAME'), (1, 'VALID'), (3, 'VALID')])
def test_residual_form_is_matching_pursuit_on_the_dense_operator(stride, padding, cplx):
    T, S, N, nev = 2, 5, 24, 3
    y, D, _ = ref.make_problem(7, 6, T, S, N, stride, padding, nev, cplx)
    A = otm.temp2mat(D, N, stride, padding).reshape(-1, N)
    for n in (1, nev, 3 * nev):                                 # 3 nev: atoms are taken again
        x, steps, _, _ = ref.mp_residual(y, D, N, stride, padding, n)
        xd, sd = ref.mp_dense(y, A, n)
        assert np.array_equal(steps, sd)
        assert np.max(np.abs(x.reshape(xd.shape) - xd)) <= 1e-12 * np.max(np.abs(xd))
    # boundary atoms too: a signal that is one truncated atom (of two taps or more: one-tap atoms tie across templates)
    taps = ref._windows(S, N, stride, padding)[2].sum(axis=1)
    c = int(np.flatnonzero(taps >= 2)[0])
    assert padding == 'VALID' or taps[c] < S
    y1 = A[c:c + 1].copy()
    x, steps, _, _ = ref.mp_residual(y1, D, N, stride, padding, 1)
    xg, _ = ref.mp_gram(y1, D, N, stride, padding, 2)
    assert steps[0] == 1 and abs(x[0].ravel()[c] - 1) <= 1e-14 and np.count_nonzero(x) == 1
    assert abs(xg[0].ravel()[c] - 1) <= 1e-12 and np.max(np.abs(np.delete(xg[0].ravel(), c))) <= 1e-12


def dyadic(padding, dtype=np.float64):
    """D = [[1, 1]], N = 10, y = 2 atom(3) + 1.5 atom(4) under 'VALID' (one index later under 'SAME')."""
    y = np.zeros((1, 10), dtype=dtype)
    y[0, 3:5] += 2
    y[0, 4:6] += 1.5
    return y, np.ones((1, 2), dtype=dtype), (3 if padding == 'VALID' else 4)


DYADIC_STEPS = {1: (2.75, 0.0), 2: (2.75, 1.125), 3: (2.1875, 1.125)}


@pytest.mark.parametrize('padding', ['VALID', 'SAME'])
def test_dyadic_reselection(padding):
    y, D, c = dyadic(padding)
    for n, want in DYADIC_STEPS.items():
        for x, steps in (ref.mp_residual(y, D, 10, 1, padding, n)[:2], ref.mp_gram(y, D, 10, 1, padding, n)):
            assert steps[0] == n
            assert (x[0, 0, c], x[0, 0, c + 1]) == want
            assert np.count_nonzero(x) == np.count_nonzero(want)


@pytest.mark.parametrize('cplx', [False, True])
def test_energy_is_the_residual_norm(cplx):
    B, T, S, N, stride, padding, nev = ref.CASES[2]
    y, D = ref.case_problem(2, cplx)
    for n in (1, nev, 4 * nev):
        x, _, _, _, E = ref.mp_residual(y, D, N, stride, padding, n, energy=True)
        pred = otm.predict(x, D, N, stride, padding)
        assert np.max(np.abs(ref.predict(x, D, N, stride, padding) - pred)) <= 1e-13 * np.max(np.abs(pred))
        r2 = np.sum(np.abs(y - pred) ** 2, axis=1)
        assert np.max(np.abs(E - r2)) <= 1e-10 * np.max(np.sum(np.abs(y) ** 2, axis=1))


def test_positive_takes_positive_correlations_only():
    y, D, x0 = ref.make_problem(3, 5, 2, 6, 80, 1, 'SAME', 6, False, noise=0.0)
    assert np.all(x0.min(axis=(1, 2)) < 0) and np.all(x0.max(axis=(1, 2)) > 0)
    for form in (ref.mp_residual, ref.mp_gram):
        x, steps = form(y, D, 80, 1, 'SAME', 6, positive=True)[:2]
        assert np.all(x >= 0) and np.all(steps >= 1)
        assert np.all(form(y, D, 80, 1, 'SAME', 6)[0].min(axis=(1, 2)) < 0)
        assert np.all(form(-np.abs(y), np.abs(D), 80, 1, 'SAME', 6, positive=True)[1] == 0)


# ---- argument checks before any GPU call ------------------------------------------------------------------------
@pytest.fixture
def no_gpu(monkeypatch):
    from decomp_amd import _arrays, _hip

    def boom(*a, **k):
        raise AssertionError('a GPU call was made before the argument check')
    monkeypatch.setattr(_arrays, 'to_device', boom)
    monkeypatch.setattr(_hip, 'load', boom)


def _problem(dtype=np.float32):
    rng = np.random.RandomState(0)
    return rng.randn(4, 30).astype(dtype), rng.randn(2, 5).astype(dtype)     # C = 34 ('SAME'), T C = 68


def test_signature():
    from decomp_amd import template_matching as tm
    assert str(inspect.signature(tm.pursuit)) == ("(y, D, n_nonzero_coefs=None, tol=None, stride=1, padding='SAME', "
                                                  "positive=False)")
    assert 'not OMP' in tm.pursuit.__doc__


def test_errors_before_any_gpu_call(no_gpu):
    from decomp_amd import template_matching as tm
    from decomp_amd.utils import exceptions
    y, D = _problem()
    with pytest.raises(exceptions.DtypeMismatchError):
        tm.pursuit(y, D.astype(np.float64), 3)
    with pytest.raises(exceptions.DtypeMismatchError):
        tm.pursuit(y.astype(np.int32), D.astype(np.int32), 3)
    with pytest.raises(exceptions.DimInvalidError):
        tm.pursuit(y, D[0], 3)
    with pytest.raises(exceptions.DimInvalidError):
        tm.pursuit(y, D[None], 3)
    with pytest.raises(exceptions.DimInvalidError):
        tm.pursuit(np.asarray(y[0, 0]), D, 3)
    for padding in ('same', 'FULL', None, 1):
        with pytest.raises(ValueError):
            tm.pursuit(y, D, 3, padding=padding)
    for stride in (0, -1, 1.0, True, None, '1'):
        with pytest.raises(ValueError):
            tm.pursuit(y, D, 3, stride=stride)
    with pytest.raises(ValueError):
        tm.pursuit(y[:, :4], D, 3)                                # S > N
    with pytest.raises(ValueError, match='n_nonzero_coefs or tol'):
        tm.pursuit(y, D)
    for n in (0, -1, 69, 2.0, True, '3'):
        with pytest.raises(ValueError):
            tm.pursuit(y, D, n)
    with pytest.raises(ValueError):
        tm.pursuit(y, D, 53, padding='VALID')                     # T C = 52 there
    for tol in (-1.0, float('nan'), float('inf'), 'x', True):
        with pytest.raises(ValueError):
            tm.pursuit(y, D, 3, tol=tol)
        with pytest.raises(ValueError):
            tm.pursuit(y, D, tol=tol)
    for positive in (1, 0, None, 'yes'):
        with pytest.raises(ValueError):
            tm.pursuit(y, D, 3, positive=positive)
    yc, Dc = _problem(np.complex64)
    with pytest.raises(ValueError, match='real'):
        tm.pursuit(yc, Dc, 3, positive=True)


def test_valid_calls_reach_the_gpu(no_gpu):
    from decomp_amd import template_matching as tm
    y, D = _problem()
    for kw in (dict(n_nonzero_coefs=68), dict(tol=0.0), dict(n_nonzero_coefs=1, tol=1.5, stride=2, padding='VALID',
                                                            positive=True),
               dict(n_nonzero_coefs=np.int64(3), positive=np.bool_(False))):
        with pytest.raises(AssertionError, match='GPU call'):
            tm.pursuit(y, D, **kw)
    yc, Dc = _problem(np.complex128)
    with pytest.raises(AssertionError, match='GPU call'):
        tm.pursuit(yc[0], Dc, 5)


def test_mixed_numpy_and_torch_is_a_type_error():
    import torch
    from decomp_amd import template_matching as tm
    y, D = _problem()
    with pytest.raises(TypeError):
        tm.pursuit(torch.from_numpy(y), D, 3)


# ---- the C ABI lists the new entries ----------------------------------------------------------------------------
def test_header_bindings_and_library_list_the_entries():
    from decomp_amd import _hip
    text = open(os.path.join(ROOT, 'include', 'decomp_hip.h')).read()
    lib = _hip.load()
    for sfx, elem in (('f32', 4), ('f64', 8), ('c64', 8), ('c128', 16)):
        name = 'dcp_tm_pursuit_' + sfx
        assert re.search(r'\bint %s\(dcp_handle\* h, const void\* Y, const void\* D, void\* X, int64_t B' % name, text)
        assert len(_hip.SIGNATURES[name][1]) == 14
        assert _hip.SIGNATURES[name][1][10] is ctypes.c_int64 and _hip.SIGNATURES[name][1][11] is ctypes.c_double
        assert hasattr(lib, name)
        atoms = getattr(lib, 'dcp_tm_pursuit_lds_atoms_' + sfx)()
        assert atoms == 144 * 1024 // elem
    # no handle: DCP_ERR_INVALID, never a crash
    it = ctypes.c_int(0)
    assert lib.dcp_tm_pursuit_f32(None, None, None, None, 1, 1, 1, 1, 1, 1, 1, -1.0, 0, ctypes.byref(it)) == -1
