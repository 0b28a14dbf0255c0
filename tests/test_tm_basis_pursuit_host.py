"""CPU: template_matching.basis_pursuit without a GPU -- its argument checks fire before any GPU call, a 2-D D reaches
``_lasso`` with the arguments given, the oracle (oracle.lasso on the dense operator [T C, Ch N]) reproduces the
reference's own outputs in tests/golden/tm_basis_pursuit_golden.npz, the NumPy statement of the Gram-form iteration
(tm_basis_pursuit_ref.gram_form: Corr where an atom lies inside, explicit sums where neither does, zero beyond dh)
is the oracle to 1e-12 on every geometry of the GPU tests, and the stop-bookkeeping problems keep every stop statistic
at least 1 % away from tol."""
import numpy as np
import pytest

import tm_basis_pursuit_ref as ref
import tm_multichannel_ref as mc
from tm_pursuit_ref import inside_atoms


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
    x = np.zeros((4, 2, 34), dtype=np.float32)
    bp = tm.basis_pursuit
    with pytest.raises(exceptions.DimInvalidError):
        bp(y, D[0, 0], 0.1)                                           # D.ndim = 1
    with pytest.raises(exceptions.DimInvalidError):
        bp(y, D[None], 0.1)                                           # D.ndim = 4
    with pytest.raises(ValueError):
        bp(y[0, 0], D, 0.1)                                           # y.ndim = 1 with a 3-D D
    with pytest.raises(ValueError):
        bp(y[:, :2], D, 0.1)                                          # y.shape[-2] != Ch
    with pytest.raises(ValueError):
        bp(y[:, :0], D[:, :0], 0.1)                                   # Ch = 0
    with pytest.raises(exceptions.DtypeMismatchError):
        bp(y, D.astype(np.float64), 0.1)
    with pytest.raises(exceptions.DtypeMismatchError):
        bp(y, D, 0.1, x=x.astype(np.float64))
    with pytest.raises(ValueError):
        bp(y, D, 0.1, padding='FULL')
    with pytest.raises(ValueError):
        bp(y, D, 0.1, stride=0)
    with pytest.raises(ValueError):
        bp(y, D, 0.1, stride=1.5)
    with pytest.raises(ValueError):
        bp(y[:, :, :4], D, 0.1)                                       # S > N
    with pytest.raises(ValueError, match='alpha'):
        bp(y, D, -0.1)
    with pytest.raises(ValueError, match='alpha'):
        bp(y, D, None)
    with pytest.raises(ValueError, match='tol'):
        bp(y, D, 0.1, tol=-1.0)
    for bad in (0, -3, 2.5, None, True):
        with pytest.raises(ValueError, match='maxiter'):
            bp(y, D, 0.1, maxiter=bad)
    with pytest.raises(ValueError, match='methods'):
        bp(y, D, 0.1, method='omp')
    with pytest.raises(ValueError, match='real'):
        bp(y.astype(np.complex64), D.astype(np.complex64), 0.1, method='ista_pos')
    with pytest.raises(ValueError, match='real'):                     # ... with templates [T, S] too
        bp(y[:, 0].astype(np.complex64), D[:, 0].astype(np.complex64), 0.1, method='fista_pos')
    for wrong in (x[:3], x[:, :, :33], x[0], x[:, :1]):
        with pytest.raises(ValueError, match='x'):
            bp(y, D, 0.1, x=wrong)
    with pytest.raises(ValueError, match='x'):
        bp(y[0], D, 0.1, x=x)                                         # one signal takes x [T, C]
    for method in ('cd', 'parallel_cd', 'admm', 'cd_pos'):            # the dense methods have no multichannel form
        with pytest.raises(NotImplementedError, match='multichannel'):
            bp(y, D, 0.1, method=method)
    with pytest.raises(TypeError):
        import torch
        bp(y, torch.from_numpy(D), 0.1)                               # mixed array kinds
    for kw in (dict(), dict(x=x), dict(method='fista_pos', stride=2, padding='VALID')):   # valid calls reach the GPU
        with pytest.raises(AssertionError, match='GPU call'):
            bp(y, D, 0.1, **kw)
    with pytest.raises(AssertionError, match='GPU call'):
        bp(y[0], D, 0.1, x=x[0])
    with pytest.raises(AssertionError, match='GPU call'):
        bp(y[:, 0], D[:, 0], 0.1, method='cd')                        # templates [T, S] keep the dense methods


def test_solve_keeps_refusing_multichannel_lasso(no_gpu):
    from decomp_amd import template_matching as tm
    rng = np.random.RandomState(0)
    with pytest.raises(NotImplementedError, match='multichannel'):
        tm.solve(rng.randn(4, 3, 30), rng.randn(2, 3, 5), 0.1, maxiter=1)


@pytest.mark.parametrize('method', ['acc_ista', 'fista_pos', 'cd'])
def test_templates_2d_reach_lasso_with_the_arguments_given(monkeypatch, method):
    """D [T, S]: basis_pursuit is ``_lasso`` on y flattened to [B, N] and a copy of x, nothing else."""
    import torch
    from decomp_amd import template_matching as tm, _arrays
    seen = {}

    def to_device(a, device=None, copy=False):
        if a is None:
            return None
        t = a if _arrays.is_torch(a) else torch.from_numpy(np.ascontiguousarray(a))
        return t.clone() if copy else t

    def fake_lasso(y, D, x, alpha, stride, padding, lasso_method, lasso_iter, lasso_tol):
        seen.update(y=y, D=D, x=x.clone(), args=(alpha, stride, padding, lasso_method, lasso_iter, lasso_tol))
        x += 1
        return 7

    def boom(*a, **k):
        raise AssertionError('the multichannel entry was called for templates [T, S]')
    monkeypatch.setattr(_arrays, 'to_device', to_device)
    monkeypatch.setattr(tm, '_lasso', fake_lasso)
    monkeypatch.setattr(tm, '_call', boom)
    rng = np.random.RandomState(1)
    y, D = rng.randn(2, 3, 30), rng.randn(2, 5)
    x = rng.randn(2, 3, 2, 13)
    x_in = x.copy()
    it, xn = tm.basis_pursuit(y, D, 0.25, x=x, tol=1e-4, maxiter=12, method=method, stride=2, padding='VALID')
    assert it == 7 and isinstance(xn, np.ndarray) and xn.shape == x.shape
    assert np.array_equal(x, x_in) and np.array_equal(xn, x_in + 1)   # x is copied, the copy is what _lasso updates
    assert seen['args'] == (0.25, 2, 'VALID', method, 12, 1e-4)
    assert tuple(seen['y'].shape) == (6, 30) and np.array_equal(seen['y'].numpy(), y.reshape(6, 30))
    assert np.array_equal(seen['D'].numpy(), D) and np.array_equal(seen['x'].numpy(), x_in.reshape(6, 2, 13))
    it, xn = tm.basis_pursuit(y[0, 0], D, 0.25, method=method)        # one signal, x = None: zeros [T, C]
    assert xn.shape == (2, 34) and np.array_equal(xn, np.ones((2, 34))) and seen['args'][1:3] == (1, 'SAME')


# ---- the oracle against the reference's own outputs ----------------------------------------------------------------------
@pytest.mark.parametrize('case', ref.GOLDEN_CASES, ids=[c[0] for c in ref.GOLDEN_CASES])
def test_oracle_reproduces_the_golden_vectors(case):
    tag, dtype, method, stride, padding, maxiter, tol = case
    gold = np.load(ref.GOLDEN)
    y, D, x0, alpha = ref.golden_inputs(ref.GOLDEN_CASES.index(case), dtype, stride, padding)
    for name, a in (('y', y), ('D', D), ('x0', x0), ('alpha', np.array(alpha))):
        assert np.array_equal(gold['%s_%s' % (tag, name)], a)          # the fixture's inputs are this recipe's
    assert gold[tag + '_A'].shape == (x0.shape[1] * x0.shape[2], y.shape[1] * y.shape[2])
    assert np.array_equal(gold[tag + '_A'], mc.dense_operator(D, y.shape[-1], stride, padding))
    it, x = ref.oracle(y, D, alpha, x0, tol, maxiter, method, stride, padding)
    want = gold[tag + '_x'].reshape(x0.shape)
    assert it == int(gold[tag + '_it'])
    assert ref.rel_err(x, want) < (1e-10 if np.dtype(dtype).itemsize // (2 if np.dtype(dtype).kind == 'c' else 1) == 8
                                   else 2e-4)


# ---- the Gram-form iteration is the oracle ---------------------------------------------------------------------------------
def test_the_geometries_are_what_their_names_say():
    from oracle import template_matching as otm
    for name, (B, T, Ch, S, N, stride, padding) in ref.GEOMS.items():
        C, _ = otm.geometry(S, N, stride, padding)
        n_inside = len(inside_atoms(S, N, stride, padding))
        assert (n_inside == C) == (padding == 'VALID')                # an edge table with 'SAME' only
        assert (n_inside == 0) == (name == 'none_inside')
        assert ((S - 1) // stride == 0) == (name == 'diagonal')       # dh = 0
        assert (C > 256) == (name in ('tiles_same', 'tiles_valid_s1'))


@pytest.mark.parametrize('cplx', [False, True])
@pytest.mark.parametrize('name', [n for n in sorted(ref.GEOMS) if n != 'no_lds'])
def test_gram_form_is_the_oracle(name, cplx):
    y, D, x0, alpha = ref.problem(name, cplx)
    stride, padding = ref.GEOMS[name][5:]
    for method in ref.METHODS + (() if cplx else ('acc_ista_pos',)):
        for maxiter, tol in ((4, 0.0), (12, 1e-3)):
            it, x = ref.oracle(y, D, alpha, x0, tol, maxiter, method, stride, padding, A=ref.operator(name, cplx))
            itg, xg = ref.gram_form(y, D, alpha, x0, tol, maxiter, method, stride, padding)
            assert itg == it
            assert ref.rel_err(xg, x) < 1e-12, (method, maxiter, ref.rel_err(xg, x))
        assert np.any(x == 0) and np.any(x != 0)                      # alpha leaves a sparse, non-trivial code


def test_gram_form_needs_the_explicit_edge_sums():
    """Taking Corr for every pair (no edge table) is a different iteration wherever two atoms reach outside."""
    y, D, x0, alpha = ref.problem('tile_s1_same', False)
    G, inside = ref.banded_gram(D, 40, 1, 'SAME')
    A = ref.operator('tile_s1_same', False)
    assert np.max(np.abs(G - A @ A.conj().T)) < 1e-12 * np.max(np.abs(G)) and not inside.all() and inside.any()


# ---- the stop bookkeeping problems ---------------------------------------------------------------------------------------
@pytest.mark.parametrize('method', ref.METHODS)
def test_stop_statistics_stay_away_from_tol(method):
    y, D, A, C = ref.stop_problem(method)
    B, T = y.shape[0], D.shape[0]
    stride, padding = ref.STOP_SHAPE[5:]
    its = {}
    for maxiter in ref.STOP_MAXITER:
        for tol in ref.STOP_TOL:
            trace = []
            it, _ = ref.oracle(y, D, ref.STOP_ALPHA, np.zeros((B, T, C)), tol, maxiter, method, stride, padding,
                               trace=trace, A=A)
            assert ref.stop_margin_ok([float(np.max(t)) for t in trace], tol), (maxiter, tol)
            its[maxiter, tol] = it
    # the cases the bookkeeping is about: exhaustion, an exit at iteration 0, a check on the very last iteration (11),
    # the test met on the last iteration (21), an exit at iteration 20 with iteration 21 discarded (31)
    assert all(its[m, 0.0] == m - 1 for m in ref.STOP_MAXITER) and all(its[m, 1e3] == 0 for m in ref.STOP_MAXITER)
    assert its[11, 3e-3] == 10 and its[12, 3e-3] == 11 and its[21, 3e-3] == 20 and its[31, 3e-3] == 20
