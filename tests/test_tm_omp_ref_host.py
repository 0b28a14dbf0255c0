"""CPU: the NumPy restatements of orthogonal convolutional pursuit (tests/tm_omp_ref.py) agree with OMP on the dense
operator and with each other; leaving out the support atoms whose coefficient a step did not change is exact; the
argument checks of template_matching.orthogonal_pursuit run before any GPU call; header, bindings and library list the
new entries."""
import ctypes
import inspect
import os
import re

import numpy as np
import pytest

import omp_ref
import tm_omp_ref as ref
from oracle import template_matching as otm

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


# ---- the restatements ---------------------------------------------------------------------------------------------
@pytest.mark.parametrize('cplx', [False, True])
@pytest.mark.parametrize('case', [0, 2])
def test_residual_form_is_omp_on_the_dense_operator(case, cplx):
    B, T, S, N, stride, padding, nev = ref.CASES[case]
    y, D = ref.case_problem(case, cplx)
    y = y[:12]
    A = otm.temp2mat(D, N, stride, padding).reshape(-1, N)
    for kw in (dict(n=nev), dict(tol=ref.case_tol(case, cplx), n=3 * nev)):
        x, steps, margin, rmargin = ref.omp_residual(y, D, N, stride, padding, **kw)
        xd, sd, md, rd = omp_ref.omp_lstsq(y, A, kw['n'], tol=kw.get('tol'))
        assert np.array_equal(steps, sd) and steps.max() >= nev
        assert np.array_equal((x != 0).reshape(xd.shape), xd != 0)
        assert np.max(np.abs(x.reshape(xd.shape) - xd)) <= 1e-12 * np.max(np.abs(xd))
        assert np.max(np.abs(margin - md)) <= 1e-12 and np.allclose(rmargin, rd, rtol=0, atol=1e-12)


@pytest.mark.parametrize('cplx', [False, True])
@pytest.mark.parametrize('case', [0, 1, 2, 3, 4, 5, 6])
def test_residual_and_gram_forms_agree_in_double(case, cplx):
    B, T, S, N, stride, padding, nev = ref.CASES[case]
    y, D = ref.case_problem(case, cplx)
    y = y[:8]
    for kw in (dict(n=nev), dict(tol=ref.case_tol(case, cplx))):
        x, steps, margin, _ = ref.omp_residual(y, D, N, stride, padding, **kw)
        xg, sg = ref.omp_gram(y, D, N, stride, padding, **kw)
        keep = margin >= 1e-8
        assert keep.sum() >= 6
        assert np.array_equal(steps[keep], sg[keep])
        assert np.max(np.abs(x - xg)[keep]) <= 1e-10 * np.max(np.abs(x))


@pytest.mark.parametrize('dt', ['float32', 'float64', 'complex64', 'complex128'])
def test_skipping_unchanged_coefficients_is_exact(dt):
    """Events in separate clusters: a step re-fits its own cluster alone, the other coefficients keep their bits."""
    cplx = np.dtype(dt).kind == 'c'
    T, S, N, nev = 2, 5, 400, 10
    y, D, _ = ref.mp.make_problem(3, 4, T, S, N, 1, 'SAME', nev, cplx)
    y, D = y.astype(dt), D.astype(dt)
    xs, ss = ref.omp_gram(y, D, N, 1, 'SAME', nev, skip_unchanged=True)
    xa, sa = ref.omp_gram(y, D, N, 1, 'SAME', nev, skip_unchanged=False)
    assert np.array_equal(ss, sa) and np.array_equal(xs, xa)
    # and a step does leave the other clusters' coefficients as they were
    x1 = ref.omp_gram(y, D, N, 1, 'SAME', nev - 1)[0]
    unchanged = (x1 != 0) & (x1 == xs)
    assert unchanged.reshape(4, -1).sum(axis=1).min() >= 1


def test_edge_atoms_use_the_explicit_gram_sum():
    """'SAME', T = 1, S = 5: truncated atoms at both ends and an inside atom that overlaps the first."""
    y, D, geom, x0 = ref.edge_problem(False)
    x, steps, margin, _ = ref.omp_residual(y, D, *geom, n=3)
    xg, sg = ref.omp_gram(y, D, *geom, n=3)
    assert np.array_equal(steps, [3, 3]) and np.array_equal(sg, steps)
    assert np.array_equal(x != 0, x0 != 0)
    assert np.max(np.abs(x - x0)) <= 1e-6 and np.max(np.abs(xg - x)) <= 1e-12     # (y is rounded to single-exact)


# ---- argument checks before any GPU call ------------------------------------------------------------------------
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


def test_signature():
    from decomp_amd import template_matching as tm
    assert str(inspect.signature(tm.orthogonal_pursuit)) == ("(y, D, n_nonzero_coefs=None, tol=None, stride=1, "
                                                             "padding='SAME')")
    assert 're-fitting' in tm.orthogonal_pursuit.__doc__


def test_errors_before_any_gpu_call(no_gpu):
    from decomp_amd import template_matching as tm
    from decomp_amd.utils import exceptions
    y, D = _problem()
    with pytest.raises(exceptions.DtypeMismatchError):
        tm.orthogonal_pursuit(y, D.astype(np.float64), 3)
    with pytest.raises(exceptions.DtypeMismatchError):
        tm.orthogonal_pursuit(y.astype(np.int32), D.astype(np.int32), 3)
    with pytest.raises(exceptions.DimInvalidError):
        tm.orthogonal_pursuit(y, D[0], 3)
    with pytest.raises(exceptions.DimInvalidError):
        tm.orthogonal_pursuit(y, D[None], 3)
    with pytest.raises(exceptions.DimInvalidError):
        tm.orthogonal_pursuit(np.asarray(y[0, 0]), D, 3)
    for padding in ('same', 'FULL', None, 1):
        with pytest.raises(ValueError):
            tm.orthogonal_pursuit(y, D, 3, padding=padding)
    for stride in (0, -1, 1.0, True, None, '1'):
        with pytest.raises(ValueError):
            tm.orthogonal_pursuit(y, D, 3, stride=stride)
    with pytest.raises(ValueError):
        tm.orthogonal_pursuit(y[:, :4], D, 3)                     # S > N
    with pytest.raises(ValueError, match='n_nonzero_coefs or tol'):
        tm.orthogonal_pursuit(y, D)
    for n in (0, -1, 65, 69, 2.0, True, '3'):                     # 65 = cap + 1 <= T C = 68
        with pytest.raises(ValueError):
            tm.orthogonal_pursuit(y, D, n)
    yv, Dv = _problem(N=20)
    with pytest.raises(ValueError):
        tm.orthogonal_pursuit(yv, Dv, 33, padding='VALID')        # T C = 32 there, below the cap
    for tol in (-1.0, float('nan'), float('inf'), 'x', True):
        with pytest.raises(ValueError):
            tm.orthogonal_pursuit(y, D, 3, tol=tol)
        with pytest.raises(ValueError):
            tm.orthogonal_pursuit(y, D, tol=tol)
    with pytest.raises(TypeError):
        tm.orthogonal_pursuit(y, D, 3, positive=True)             # no such keyword


@pytest.mark.parametrize('dt,cap', [(np.float32, 64), (np.float64, 64), (np.complex64, 32), (np.complex128, 32)])
def test_one_past_the_cap_is_a_value_error(no_gpu, dt, cap):
    from decomp_amd import template_matching as tm
    y, D = _problem(dt)                                           # T C = 68 > cap
    with pytest.raises(ValueError, match='cap'):
        tm.orthogonal_pursuit(y, D, cap + 1)
    with pytest.raises(AssertionError, match='GPU call'):
        tm.orthogonal_pursuit(y, D, cap)


def test_valid_calls_reach_the_gpu(no_gpu):
    from decomp_amd import template_matching as tm
    y, D = _problem()
    for kw in (dict(n_nonzero_coefs=64), dict(tol=0.0), dict(n_nonzero_coefs=1, tol=1.5, stride=2, padding='VALID'),
               dict(n_nonzero_coefs=np.int64(3))):
        with pytest.raises(AssertionError, match='GPU call'):
            tm.orthogonal_pursuit(y, D, **kw)
    yc, Dc = _problem(np.complex128)
    with pytest.raises(AssertionError, match='GPU call'):
        tm.orthogonal_pursuit(yc[0], Dc, 5)


def test_mixed_numpy_and_torch_is_a_type_error():
    import torch
    from decomp_amd import template_matching as tm
    y, D = _problem()
    with pytest.raises(TypeError):
        tm.orthogonal_pursuit(torch.from_numpy(y), D, 3)


# ---- the C ABI lists the new entries ----------------------------------------------------------------------------
def test_header_bindings_and_library_list_the_entries():
    from decomp_amd import _hip
    text = open(os.path.join(ROOT, 'include', 'decomp_hip.h')).read()
    lib = _hip.load()
    for sfx, elem in (('f32', 4), ('f64', 8), ('c64', 8), ('c128', 16)):
        name = 'dcp_tm_omp_' + sfx
        assert re.search(r'\bint %s\(dcp_handle\* h, const void\* Y, const void\* D, void\* X, int64_t B' % name, text)
        assert re.search(r'\bint dcp_tm_omp_lds_atoms_%s\(void\);' % sfx, text)
        assert len(_hip.SIGNATURES[name][1]) == 13
        assert _hip.SIGNATURES[name][1][10] is ctypes.c_int64 and _hip.SIGNATURES[name][1][11] is ctypes.c_double
        assert _hip.SIGNATURES['dcp_tm_omp_lds_atoms_' + sfx] == (ctypes.c_int, [])
        assert hasattr(lib, name)
        atoms = getattr(lib, 'dcp_tm_omp_lds_atoms_' + sfx)()
        assert atoms == 112 * 1024 // elem
        # no handle: DCP_ERR_INVALID, never a crash
        it = ctypes.c_int(0)
        assert getattr(lib, name)(None, None, None, None, 1, 1, 1, 1, 1, 1, 1, -1.0, ctypes.byref(it)) == -1
