"""CPU: the NumPy references of orthogonal matching pursuit (omp_ref.py) against closed forms, the share of rows
the GPU tests leave out of the support comparison, and every argument error of decomp_amd.omp.solve and of
dictionary_learning.solve(lasso_method='omp'), raised before any GPU call."""
import numpy as np
import pytest

import omp_ref


@pytest.fixture
def no_gpu(monkeypatch):
    from decomp_amd import _arrays, _hip

    def boom(*a, **k):
        raise AssertionError('a GPU call was made before the argument check')
    monkeypatch.setattr(_arrays, 'to_device', boom)
    monkeypatch.setattr(_hip, 'load', boom)


def _small(cplx, N=9, F=20, K=12, seed=3):
    rng = np.random.RandomState(seed)
    A = rng.randn(K, F)
    y = rng.randn(N, F)
    if cplx:
        A = A + 1j * rng.randn(K, F)
        y = y + 1j * rng.randn(N, F)
    return y, A


# ---- the references ----------------------------------------------------------------------------------------
@pytest.mark.parametrize('cplx', [False, True])
def test_full_support_is_the_least_squares(cplx):
    y, A = _small(cplx)
    x, steps, _, _ = omp_ref.omp_lstsq(y, A, A.shape[0])
    want = np.linalg.lstsq(A.T, y.T, rcond=None)[0].T
    assert np.all(steps == A.shape[0])
    assert np.max(np.abs(x - want)) <= 1e-10 * np.max(np.abs(want))


@pytest.mark.parametrize('cplx', [False, True])
def test_one_step_is_the_argmax_rule(cplx):
    y, A = _small(cplx, N=40)
    A = A * (0.5 + np.arange(A.shape[0]))[:, None]      # unequal norms: the rule divides by them
    x, steps, _, _ = omp_ref.omp_lstsq(y, A, 1)
    nrm = np.linalg.norm(A, axis=1)
    k = np.argmax(np.abs(y @ A.conj().T) / nrm, axis=1)
    assert np.all(steps == 1)
    assert np.array_equal(np.argmax(x != 0, axis=1), k) and np.all(np.count_nonzero(x, axis=1) == 1)
    coef = np.einsum('nf,nf->n', y, A[k].conj()) / nrm[k] ** 2
    assert np.max(np.abs(x[np.arange(len(k)), k] - coef)) <= 1e-12 * np.max(np.abs(coef))


@pytest.mark.parametrize('cplx', [False, True])
@pytest.mark.parametrize('with_tol', [False, True])
def test_gram_form_agrees_with_lstsq_form(cplx, with_tol):
    y, A = omp_ref.make_problem(5, 30, 24, 40, 4, cplx)
    yn2 = np.sum(np.abs(y) ** 2, axis=1)
    tol = 0.02 * float(np.median(yn2)) if with_tol else None
    x, steps, _, _ = omp_ref.omp_lstsq(y, A, 8, tol=tol)
    xg, sg = omp_ref.omp_gram(y @ A.conj().T, A @ A.conj().T, yn2, 8, tol=tol)
    assert np.array_equal(steps, sg)
    assert np.all(steps < 8) if with_tol else np.all(steps == 8)
    assert np.array_equal(x != 0, xg != 0)
    assert np.max(np.abs(x - xg)) <= 1e-11 * np.max(np.abs(x))


def test_duplicate_and_zero_atoms():
    y, A = _small(False, N=5, F=10, K=4, seed=7)
    A[2] = A[0]
    A[3] = 0
    x, steps, _, _ = omp_ref.omp_lstsq(y, A, 4)
    assert np.all(x[:, 3] == 0) and np.all((x[:, 0] == 0) | (x[:, 2] == 0)) and np.all(steps <= 2)
    xg, sg = omp_ref.omp_gram(y @ A.T, A @ A.T, np.sum(y * y, axis=1), 4)
    assert np.array_equal(steps, sg) and np.all(np.isfinite(xg))


def test_solve_fastpath_omp_has_the_oracle_signature():
    import inspect
    from oracle import lasso as olasso
    assert (list(inspect.signature(omp_ref.solve_fastpath_omp).parameters) ==
            list(inspect.signature(olasso.solve_fastpath).parameters))
    y, A = _small(False)
    it, x = omp_ref.solve_fastpath_omp(y, A, 0.0, np.ones((9, 12)), -1.0, 3, 'omp')
    assert it == 3 and np.all(np.count_nonzero(x, axis=1) == 3)


@pytest.mark.parametrize('case', sorted(omp_ref.CASES))
def test_left_out_shares_are_under_the_cap(case):
    """At most 10 % of a case's rows may be left out of the support comparison."""
    precisions = ('single', 'double') if case in omp_ref.SINGLE_CASES else ('double',)
    for with_tol in (False, True):
        an = omp_ref.case_analysis(case, with_tol)
        steps = an.steps
        if with_tol:
            assert 2 <= len(set(steps.tolist()))
        for precision in precisions:
            keep = an.keep(precision)
            share = 1.0 - float(np.mean(keep))
            print('case', case, precision, 'tol' if with_tol else 's', 'left out %.2f %%' % (100 * share),
                  'step counts', sorted(set(steps.tolist())))
            assert share <= omp_ref.MAX_LEFT_OUT, (case, precision, with_tol, share)


# ---- argument errors, before any GPU call --------------------------------------------------------------------
def test_omp_solve_argument_errors(no_gpu):
    from decomp_amd import omp
    y, A = _small(False)
    yc, Ac = _small(True, K=40, F=50)
    with pytest.raises(ValueError):
        omp.solve(y, A)
    for bad in (0, -1, 13, 2.0, '3', True, None):
        if bad is None:
            continue
        with pytest.raises(ValueError, match='64'):
            omp.solve(y, A, n_nonzero_coefs=bad)
    with pytest.raises(ValueError, match='32'):
        omp.solve(yc, Ac, n_nonzero_coefs=33)
    yw, Aw = _small(False, K=80, F=90)
    with pytest.raises(ValueError, match='64'):
        omp.solve(yw, Aw, n_nonzero_coefs=65)
    for bad in (-1e-3, float('nan'), float('inf'), '0.1'):
        with pytest.raises(ValueError):
            omp.solve(y, A, tol=bad)
        with pytest.raises(ValueError):
            omp.solve(y, A, n_nonzero_coefs=2, tol=bad)
    # the assertion.* errors of lasso.solve
    from decomp_amd.utils.exceptions import ShapeMismatchError, DtypeMismatchError, DimInvalidError
    with pytest.raises(ShapeMismatchError):
        omp.solve(y, A[:, :-1], n_nonzero_coefs=2)
    with pytest.raises(DimInvalidError):
        omp.solve(y, A[0], n_nonzero_coefs=2)
    with pytest.raises(DtypeMismatchError):
        omp.solve(y.astype(np.float32), A, n_nonzero_coefs=2)
    with pytest.raises(DtypeMismatchError):
        omp.solve(y.astype(np.int64), A.astype(np.int64), n_nonzero_coefs=2)
    # valid arguments reach the device copy
    for kw in (dict(n_nonzero_coefs=3), dict(tol=0.5), dict(n_nonzero_coefs=np.int64(12), tol=np.float32(0.0))):
        with pytest.raises(AssertionError, match='GPU call'):
            omp.solve(y, A, **kw)
    with pytest.raises(AssertionError, match='GPU call'):
        omp.solve(yc, Ac, n_nonzero_coefs=32)


def test_dictionary_learning_omp_argument_errors(no_gpu):
    from decomp_amd import dictionary_learning as dl, lasso, sharded
    rng = np.random.RandomState(0)
    y, D = rng.randn(40, 10), rng.randn(4, 10)
    kw = dict(minibatch=8, maxiter=3, lasso_method='omp', lasso_iter=2, lasso_tol=None, random_seed=0)
    for alpha in (0.1, -1.0, float('nan'), None):
        with pytest.raises(ValueError):
            dl.solve(y, D, alpha, **kw)
    with pytest.raises(NotImplementedError):
        dl.solve(y, D, 0.0, mask=np.ones_like(y), **kw)
    for bad in (0, 5, 1.5):
        with pytest.raises(ValueError):
            dl.solve(y, D, 0.0, **dict(kw, lasso_iter=bad))
    for bad in (-1.0, float('inf')):
        with pytest.raises(ValueError):
            dl.solve(y, D, 0.0, **dict(kw, lasso_tol=bad))
    with pytest.raises(NotImplementedError):
        sharded.dictionary_learning_sharded(y, D, 0.0, **kw)
    for alpha in (0.0, 0):
        with pytest.raises(AssertionError, match='GPU call'):
            dl.solve(y, D, alpha, **kw)
    # lasso.solve is unchanged: 'omp' is not one of its methods
    assert 'omp' not in lasso.AVAILABLE_METHODS
    with pytest.raises(ValueError):
        lasso.solve(y, D, 0.0, method='omp')
    assert lasso._dict_method_code('omp') == 6
