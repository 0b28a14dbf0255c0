"""CPU: the NumPy restatement of approximate K-SVD (tests/ksvd_ref.py) -- its sweep never increases the objective,
maintains R = y - x D, has Y = X D as a fixed point, keeps unused atoms and atoms with u = 0 -- and the argument
checks of ksvd.solve and dictionary_learning.solve(method='ksvd'), which run before any GPU call."""
import numpy as np
import pytest

import ksvd_ref
import omp_ref


# ---- the restatement ----------------------------------------------------------------------------------------
@pytest.mark.parametrize('case', sorted(ksvd_ref.CASES))
@pytest.mark.parametrize('start', ['planted', 'random'])
def test_sweep_never_increases_the_objective_and_maintains_the_residual(case, start):
    y, x, D = ksvd_ref.sweep_inputs(case, start)
    before = ksvd_ref.objective(y, x, D)
    xs, Ds, R = ksvd_ref.sweep(y, x, D)
    after = ksvd_ref.objective(y, xs, Ds)
    print('case %d %s: objective %.4g -> %.4g' % (case, start, before, after))
    assert after <= before * (1 + 1e-12)
    assert after < before
    assert np.max(np.abs(R - (y - xs @ Ds))) <= 1e-13 * np.max(np.abs(y))
    assert np.array_equal(xs == 0, x == 0) or np.all((xs != 0) <= (x != 0))     # the supports do not grow
    used = np.any(x != 0, axis=0)
    assert np.allclose(np.linalg.norm(Ds[used], axis=1), 1.0, atol=1e-14)


def test_every_atom_step_is_monotone():
    """The guarantee is per atom: sweeping the atoms one at a time, no single step increases |y - x D|^2."""
    y, x, D = ksvd_ref.sweep_inputs(1)
    x, D = x.copy(), D.copy()
    last = ksvd_ref.objective(y, x, D)
    for k in range(D.shape[0]):
        xk = np.zeros_like(x)
        xk[:, k] = x[:, k]
        # the sweep of a problem that holds atom k alone, on the data the other atoms leave: y - x D + x_k d_k
        rest = y - x @ D + np.outer(x[:, k], D[k])
        xs, Ds, _ = ksvd_ref.sweep(rest, xk[:, k:k + 1], D[k:k + 1])
        x[:, k], D[k] = xs[:, 0], Ds[0]
        now = ksvd_ref.objective(y, x, D)
        assert now <= last * (1 + 1e-12), k
        last = now
    xs, Ds, _ = ksvd_ref.sweep(*ksvd_ref.sweep_inputs(1))
    assert np.allclose(x, xs, atol=1e-12) and np.allclose(D, Ds, atol=1e-12)


@pytest.mark.parametrize('cplx', [False, True])
def test_exact_factorisation_is_a_fixed_point(cplx):
    """Y = X D exactly: R = 0, u = |g|^2 d, so D and X stay."""
    rng = np.random.RandomState(5)
    D = ksvd_ref.random_start(5, 9, 16, cplx)
    D = ksvd_ref.normalise(D)
    x = rng.randn(60, 9) * (rng.rand(60, 9) < 0.3)
    x = x.astype(D.dtype)
    y = x @ D
    xs, Ds, R = ksvd_ref.sweep(y, x, D)
    assert np.max(np.abs(Ds - D)) <= 1e-14 and np.max(np.abs(xs - x)) <= 1e-13
    assert np.max(np.abs(R)) <= 1e-13


def test_empty_column_leaves_its_atom_untouched():
    y, x, D = ksvd_ref.sweep_inputs(1)
    x = x.copy()
    x[:, 7] = 0
    xs, Ds, _ = ksvd_ref.sweep(y, x, D)
    assert np.array_equal(Ds[7], D[7]) and np.all(xs[:, 7] == 0)
    assert not np.array_equal(Ds[6], D[6])


def zero_u_problem(dtype):
    """K = 1, y = 0, with entries whose products are exact: u = -sum |g_i|^2 d + |g|^2 d = 0 in every dtype."""
    d = np.full((1, 4), 0.5, dtype=dtype)
    x = np.array([[1.0], [2.0], [0.0], [-3.0], [4.0]], dtype=dtype)
    return np.zeros((5, 4), dtype=dtype), x, d


@pytest.mark.parametrize('dtype', ['float32', 'float64', 'complex64', 'complex128'])
def test_zero_u_keeps_the_atom(dtype):
    y, x, d = zero_u_problem(dtype)
    xs, ds, R = ksvd_ref.sweep(y, x, d)
    assert np.array_equal(ds, d)
    # g' = R d^H + g |d|^2 = -g + g = 0: the coefficients vanish, the residual returns to y = 0
    assert np.all(xs == 0) and np.all(R == 0)


def test_nan_u_keeps_the_atom():
    y, x, d = zero_u_problem('float64')
    y = y.copy()
    y[1, 2] = np.nan
    _, ds, _ = ksvd_ref.sweep(y, x, d)
    assert np.array_equal(ds, d)


def test_loop_improves_and_stops():
    y, A, D0 = ksvd_ref.case_problem(1)
    log = ksvd_ref.loop_reference(1, 'double')
    objs = [ksvd_ref.objective(y, x, D) for D, x, _, _ in log]
    print('objectives', objs, 'maxdiff', [m for _, _, m, _ in log])
    assert objs[-1] < objs[0]
    # the stop rule: a tol between the first two maxdiff values stops at iteration 2
    md = [m for _, _, m, _ in log]
    assert md[1] < md[0]
    it, D, x = ksvd_ref.solve(y, D0, ksvd_ref.CASES[1][4], tol=0.5 * (md[0] + md[1]), maxiter=10)
    assert it == 2 and np.array_equal(D, log[1][0]) and np.array_equal(x, log[1][1])
    assert np.mean(ksvd_ref.recovery(A, log[-1][0])) > np.mean(ksvd_ref.recovery(A, D0))


# ---- argument checks before any GPU call ------------------------------------------------------------------------
def _problem(dtype=np.float32, K=6):
    rng = np.random.RandomState(0)
    return rng.randn(40, 12).astype(dtype), rng.randn(K, 12).astype(dtype)


@pytest.fixture
def no_gpu(monkeypatch):
    from decomp_amd import _arrays, _hip

    def boom(*a, **k):
        raise AssertionError('a GPU call was made before the argument check')
    monkeypatch.setattr(_arrays, 'to_device', boom)
    monkeypatch.setattr(_hip, 'load', boom)


def test_ksvd_is_exported():
    import decomp_amd
    assert decomp_amd.ksvd.solve is not None


def test_solve_errors_before_any_gpu_call(no_gpu):
    from decomp_amd import ksvd
    from decomp_amd.utils import exceptions
    y, D = _problem()
    for s in (0, -1, 7, 65, 2.0, True, None, '3'):
        with pytest.raises(ValueError):
            ksvd.solve(y, D, s)
    yc, Dc = _problem(np.complex64, K=40)
    with pytest.raises(ValueError):
        ksvd.solve(np.tile(yc, (1, 4)), np.tile(Dc, (1, 4)), 33)      # the complex cap
    for ct in (-1.0, float('nan'), float('inf'), 'x', True):
        with pytest.raises(ValueError):
            ksvd.solve(y, D, 3, coef_tol=ct)
    for tol in (float('nan'), None, 'x', True):
        with pytest.raises(ValueError):
            ksvd.solve(y, D, 3, tol=tol)
    for maxiter in (0, -3, 2.5, None, True):
        with pytest.raises(ValueError):
            ksvd.solve(y, D, 3, maxiter=maxiter)
    with pytest.raises(exceptions.DtypeMismatchError):
        ksvd.solve(y, D.astype(np.float64), 3)
    with pytest.raises(exceptions.DtypeMismatchError):
        ksvd.solve(y.astype(np.int32), D.astype(np.int32), 3)
    with pytest.raises(exceptions.DimInvalidError):
        ksvd.solve(y[None], D, 3)
    with pytest.raises(exceptions.DimInvalidError):
        ksvd.solve(y, D[0], 3)
    with pytest.raises(exceptions.ShapeMismatchError):
        ksvd.solve(y[:, :11], D, 3)


def test_dictionary_learning_ksvd_errors_before_any_gpu_call(no_gpu):
    from decomp_amd import dictionary_learning as dl
    y, D = _problem()
    ok = dict(method='ksvd', lasso_method='omp', lasso_iter=3, lasso_tol=None)
    with pytest.raises(NotImplementedError, match='minibatch'):
        dl.solve(y, D, 0, minibatch=10, **ok)
    for lm in ('cd', 'ista', 'parallel_cd', 'nonsense'):
        with pytest.raises(NotImplementedError, match='omp'):
            dl.solve(y, D, 0, **dict(ok, lasso_method=lm))
    with pytest.raises(NotImplementedError, match='omp'):
        dl.solve(y, D, 0, method='ksvd')                              # the default lasso_method is 'cd'
    for alpha in (0.1, -1.0, None):
        with pytest.raises(ValueError, match='alpha'):
            dl.solve(y, D, alpha, **ok)
    with pytest.raises(NotImplementedError, match='mask'):
        dl.solve(y, D, 0, mask=np.ones_like(y), **ok)
    for s in (0, 7, 2.5):
        with pytest.raises(ValueError):
            dl.solve(y, D, 0, **dict(ok, lasso_iter=s))
    with pytest.raises(ValueError):
        dl.solve(y, D, 0, **dict(ok, lasso_tol=-1.0))


def test_existing_combinations_keep_their_exceptions(no_gpu):
    from decomp_amd import dictionary_learning as dl
    y, D = _problem()
    with pytest.raises(NotImplementedError, match='minibatch is required'):
        dl.solve(y, D, 0.1)
    with pytest.raises(NotImplementedError, match='minibatch is required'):
        dl.solve(y, D, 0, lasso_method='omp', lasso_iter=3)
    with pytest.raises(NotImplementedError, match='parallel_cd'):
        dl.solve(y, D, 0.1, minibatch=10, method='parallel_cd')
    with pytest.raises(NotImplementedError, match='minibatch is required'):
        dl.solve(y, D, 0.1, method='parallel_cd')


def test_valid_calls_reach_the_gpu(no_gpu):
    from decomp_amd import dictionary_learning as dl, ksvd
    y, D = _problem()
    with pytest.raises(AssertionError, match='GPU call'):
        ksvd.solve(y, D, 3)
    with pytest.raises(AssertionError, match='GPU call'):
        ksvd.solve(y, D, 6, tol=0.0, maxiter=1, coef_tol=0.0)
    with pytest.raises(AssertionError, match='GPU call'):
        dl.solve(y, D, 0, method='ksvd', lasso_method='omp', lasso_iter=3, lasso_tol=None)
    with pytest.raises(AssertionError, match='GPU call'):
        dl.solve(y, D, 0.0, method='ksvd', lasso_method='omp', lasso_iter=3)
