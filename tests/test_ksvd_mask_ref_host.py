"""CPU: the NumPy restatement of masked approximate K-SVD (tests/ksvd_mask_ref.py) -- its sweep never increases the
weighted objective, equals the unmasked sweep under an all-ones mask, treats a 1-D mask as its broadcast, handles the
degenerate columns and rows, and does not read y at hidden entries -- the argument checks of ksvd.solve(mask=...),
which run before any GPU call, and the eight new symbols of the C ABI."""
import os
import re

import numpy as np
import pytest

import ksvd_mask_ref as mr
import ksvd_ref

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


# ---- the restatement ----------------------------------------------------------------------------------------
@pytest.mark.parametrize('case', sorted(mr.CASES))
@pytest.mark.parametrize('kind', mr.KINDS)
@pytest.mark.parametrize('start', ['planted', 'random'])
def test_sweep_never_increases_the_weighted_objective(case, kind, start):
    y, x, D, m = mr.sweep_inputs(case, kind, start)
    before = mr.objective(y, x, D, m)
    xs, Ds, R = mr.sweep(y, x, D, m)
    after = mr.objective(y, xs, Ds, m)
    print('case %d %s %s: weighted objective %.4g -> %.4g' % (case, kind, start, before, after))
    assert after <= before * (1 + 1e-12)
    assert after < before
    assert np.max(np.abs(R - (y - xs @ Ds))) <= 1e-13 * np.max(np.abs(y))
    assert np.all((xs != 0) <= (x != 0))                                        # the supports do not grow
    used = np.any(x != 0, axis=0)
    assert np.allclose(np.linalg.norm(Ds[used], axis=1), 1.0, atol=1e-14)


def test_the_issues_first_iteration_figure():
    """Case 1, binary mask, first iteration: 0.01015 -> 0.00127."""
    y, x, D, m = mr.sweep_inputs(1, 'binary', 'planted')
    xs, Ds, _ = mr.sweep(y, x, D, m)
    assert abs(mr.objective(y, x, D, m) - 0.01015) < 5e-6 and abs(mr.objective(y, xs, Ds, m) - 0.00127) < 5e-6


@pytest.mark.parametrize('kind', mr.KINDS)
def test_every_atom_step_is_monotone(kind):
    """The guarantee is per atom: sweeping one atom at a time, no single step increases the weighted objective."""
    y, x, D, m = mr.sweep_inputs(2, kind, 'random')
    x, D = x.copy(), D.copy()
    last = mr.objective(y, x, D, m)
    for k in range(D.shape[0]):
        rest = y - x @ D + np.outer(x[:, k], D[k])
        xs, Ds, _ = mr.sweep(rest, x[:, k:k + 1], D[k:k + 1], m)
        x[:, k], D[k] = xs[:, 0], Ds[0]
        now = mr.objective(y, x, D, m)
        assert now <= last * (1 + 1e-12), k
        last = now
    xs, Ds, _ = mr.sweep(*mr.sweep_inputs(2, kind, 'random'))
    assert np.allclose(x, xs, atol=1e-12) and np.allclose(D, Ds, atol=1e-12)


@pytest.mark.parametrize('case', sorted(mr.CASES))
@pytest.mark.parametrize('start', ['planted', 'random'])
def test_all_ones_mask_is_the_unmasked_sweep(case, start):
    y, x, D = ksvd_ref.sweep_inputs(case, start)
    xs, Ds, Rs = ksvd_ref.sweep(y, x, D)
    for ones in (np.ones(y.shape), np.ones(y.shape[1])):
        xm, Dm, Rm = mr.sweep(y, x, D, ones)
        assert np.max(np.abs(Dm - Ds)) <= 1e-12 and np.max(np.abs(xm - xs)) <= 1e-12
        assert np.max(np.abs(Rm - Rs)) <= 1e-12
    assert abs(mr.objective(y, x, D, np.ones(y.shape)) - ksvd_ref.objective(y, x, D)) <= 1e-15


@pytest.mark.parametrize('case', [1, 2])
def test_one_dimensional_mask_is_its_broadcast(case):
    y, x, D, m = mr.sweep_inputs(case, 'weights', 'planted')
    m1 = m[0].copy()
    m1[5] = 0.0
    a = mr.sweep(y, x, D, m1)
    b = mr.sweep(y, x, D, np.ascontiguousarray(np.broadcast_to(m1, y.shape)))
    for u, v in zip(a, b):
        assert np.array_equal(u, v)


def _small(cplx=False, seed=3, N=30, F=12, K=4):
    rng = np.random.RandomState(seed)

    def randn(*s):
        return rng.randn(*s) + 1j * rng.randn(*s) if cplx else rng.randn(*s)
    D = ksvd_ref.normalise(randn(K, F))
    x = randn(N, K) * (rng.rand(N, K) < 0.4)
    y = randn(N, F)
    m = np.where(rng.rand(N, F) < 0.7, 0.25 + 0.75 * rng.rand(N, F), 0.0)
    return y, x, D, m


@pytest.mark.parametrize('cplx', [False, True])
def test_column_hidden_in_all_support_rows_keeps_its_value_before_normalisation(cplx):
    """K = 1: u_f = d_f where c_f = 0, so d'_f / d_f = 1 / |u| there."""
    y, x, D, m = _small(cplx, K=1)
    I = np.flatnonzero(x[:, 0])
    m[I, 4] = 0.0
    m[I, 9] = 0.0
    xs, Ds, _ = mr.sweep(y, x, D, m)
    mR = m[I] * (y - x @ D)[I]
    c = (np.abs(x[I, 0]) ** 2) @ m[I]
    assert c[4] == 0 and c[9] == 0 and np.all(np.delete(c, [4, 9]) > 0)
    u = np.where(c > 0, (x[I, 0].conj() @ mR + c * D[0]) / np.where(c > 0, c, 1), D[0])
    assert u[4] == D[0, 4] and u[9] == D[0, 9]
    assert np.allclose(Ds[0], u / np.linalg.norm(u), atol=1e-14)
    assert np.all(np.isfinite(xs)) and abs(np.linalg.norm(Ds[0]) - 1) <= 1e-14


@pytest.mark.parametrize('cplx', [False, True])
def test_fully_hidden_support_row_gets_zero(cplx):
    y, x, D, m = _small(cplx)
    i = int(np.flatnonzero(x[:, 1])[2])
    m[i, :] = 0.0
    before = mr.objective(y, x, D, m)
    xs, Ds, _ = mr.sweep(y, x, D, m)
    assert np.all(xs[i] == 0)                                   # q_i = 0 for every atom of the row
    assert np.all(np.isfinite(xs)) and np.all(np.isfinite(Ds))
    assert mr.objective(y, xs, Ds, m) <= before * (1 + 1e-12)


def test_unused_atom_is_kept():
    y, x, D, m = mr.sweep_inputs(1, 'weights', 'planted')
    x = x.copy()
    x[:, 7] = 0
    xs, Ds, _ = mr.sweep(y, x, D, m)
    assert np.array_equal(Ds[7], D[7]) and np.all(xs[:, 7] == 0)
    assert not np.array_equal(Ds[6], D[6])


@pytest.mark.parametrize('case', [1, 2])
@pytest.mark.parametrize('kind', mr.KINDS)
def test_y_at_hidden_entries_is_not_read(case, kind):
    y, x, D, m = mr.sweep_inputs(case, kind, 'planted')
    rng = np.random.RandomState(9)
    y2 = np.where(m > 0, y, y + 100.0 * rng.randn(*y.shape))
    assert not np.array_equal(y, y2)
    a, b = mr.sweep(y, x, D, m), mr.sweep(y2, x, D, m)
    assert np.array_equal(a[0], b[0]) and np.array_equal(a[1], b[1])
    # through the coder too
    S = mr.CASES[case][4]
    ita, Da, xa = mr.solve(y[:60], D, m[:60], S, tol=0.0, maxiter=3)
    itb, Db, xb = mr.solve(y2[:60], D, m[:60], S, tol=0.0, maxiter=3)
    assert np.allclose(Da, Db, atol=1e-12) and np.allclose(xa, xb, atol=1e-11)


def test_training_with_holes_recovers_the_planted_atoms():
    """Mean recovery rises in every case, to 0.998 or more at three digits; the worst single atom need not rise
    (case 3), so it is not asserted."""
    for case in sorted(mr.CASES):
        y, A, D0 = ksvd_ref.case_problem(case)
        for kind in mr.KINDS:
            log = mr.loop_reference(case, kind, 'double')
            rec0, rec = ksvd_ref.recovery(A, D0), ksvd_ref.recovery(A, log[-1][0])
            print('case %d %s: mean recovery %.4f -> %.4f, worst %.3f -> %.3f; smallest margin %.2g'
                  % (case, kind, rec0.mean(), rec.mean(), rec0.min(), rec.min(), min(e[3] for e in log)))
            assert rec.mean() > rec0.mean() and rec.mean() >= 0.9975
            assert min(e[3] for e in log) >= 1e-8                    # double precision compares every row


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


def test_mask_errors_before_any_gpu_call(no_gpu):
    from decomp_amd import ksvd
    from decomp_amd.utils import exceptions
    y, D = _problem()
    ones = np.ones_like(y)
    for bad in (ones.astype(np.int32), ones.astype(bool), ones.astype(np.complex64)):
        with pytest.raises(exceptions.DtypeMismatchError):
            ksvd.solve(y, D, 3, mask=bad)
    neg = ones.copy()
    neg[3, 4] = -0.5
    with pytest.raises(Exception) as e:
        ksvd.solve(y, D, 3, mask=neg)
    assert not isinstance(e.value, AssertionError) or 'GPU call' not in str(e.value)
    with pytest.raises(Exception) as e:
        ksvd.solve(y, D, 3, mask=-np.ones(12, dtype=np.float32))
    assert not isinstance(e.value, AssertionError) or 'GPU call' not in str(e.value)
    for shape in ((40, 11), (39, 12), (40,), (11,), (1, 40, 12), (12, 40)):
        with pytest.raises(exceptions.ShapeMismatchError):
            ksvd.solve(y, D, 3, mask=np.ones(shape, dtype=np.float32))
    yc, Dc = _problem(np.complex64)
    with pytest.raises(exceptions.DtypeMismatchError):
        ksvd.solve(yc, Dc, 3, mask=np.ones_like(yc))               # the mask is real, also for complex y
    # the other checks still come first or alike with a mask
    with pytest.raises(ValueError):
        ksvd.solve(y, D, 7, mask=ones)
    with pytest.raises(ValueError):
        ksvd.solve(y, D, 3, coef_tol=-1.0, mask=ones)


def test_negative_mask_raises_what_omp_solve_raises(no_gpu):
    from decomp_amd import ksvd, omp
    y, D = _problem()
    neg = np.ones_like(y)
    neg[0, 0] = -1.0
    with pytest.raises(Exception) as a:
        omp.solve(y, D, 3, mask=neg)
    with pytest.raises(Exception) as b:
        ksvd.solve(y, D, 3, mask=neg)
    assert type(a.value) is type(b.value) and 'GPU call' not in str(b.value)


def test_valid_masked_calls_reach_the_gpu(no_gpu):
    from decomp_amd import ksvd
    y, D = _problem()
    for mask in (np.ones_like(y), np.ones(12, dtype=np.float32), np.ones(y.shape, dtype=np.float64),
                 np.zeros_like(y)):
        with pytest.raises(AssertionError, match='GPU call'):
            ksvd.solve(y, D, 3, mask=mask)
    yc, Dc = _problem(np.complex128)
    with pytest.raises(AssertionError, match='GPU call'):
        ksvd.solve(yc, Dc, 3, mask=np.ones(yc.shape, dtype=np.float32))


def test_dictionary_learning_still_refuses_masks_for_ksvd_and_omp(no_gpu):
    from decomp_amd import dictionary_learning as dl
    y, D = _problem()
    with pytest.raises(NotImplementedError, match='mask'):
        dl.solve(y, D, 0, mask=np.ones_like(y), method='ksvd', lasso_method='omp', lasso_iter=3, lasso_tol=None)
    with pytest.raises(NotImplementedError, match='mask'):
        dl.solve(y, D, 0, mask=np.ones_like(y), minibatch=10, lasso_method='omp', lasso_iter=3, lasso_tol=None)


# ---- the C ABI lists the new entry points -----------------------------------------------------------------------
NEW_SYMBOLS = ['dcp_ksvd_mask_%s_%s' % (what, sfx) for what in ('sweep', 'step') for sfx in ('f32', 'f64', 'c64', 'c128')]


def test_header_and_signatures_list_the_new_symbols():
    from decomp_amd import _hip
    header = open(os.path.join(ROOT, 'include', 'decomp_hip.h')).read()
    assert len(NEW_SYMBOLS) == 8
    for name in NEW_SYMBOLS:
        assert re.search(r'\bint %s\(dcp_handle\* h,' % name, header), name
        assert name in _hip.SIGNATURES, name
        n_args = len(_hip.SIGNATURES[name][1])
        assert n_args == (11 if '_sweep_' in name else 14), (name, n_args)
