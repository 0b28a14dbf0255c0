"""CPU: the references of masked orthogonal matching pursuit (omp_mask_ref.py) agree with each other, the shares of
rows left out of the support comparison are what the GPU tests rely on, the restatement shows the degenerate-row
behaviours, and omp.solve validates its mask as lasso.solve does, before the library is loaded.

The shares are those of the issue's table except case 16 / weights / tol in double: 4 of 131 rows (0.031) here, where
the table says 0.023 (3 rows); both are far below the 10 % cap."""
import inspect

import numpy as np
import pytest

import omp_mask_ref as mr
import omp_ref

# worst share over (fixed sparsity, tol), per case: single (binary, weights), double (binary, weights)
SHARES = {11: ((0.000, 0.000), (0.000, 0.000)),
          12: ((0.054, 0.039), (0.039, 0.012)),
          14: ((0.062, 0.078), (0.016, 0.023)),
          13: ((0.156, 0.210), (0.039, 0.047)),
          15: ((0.351, 0.511), (0.046, 0.069)),
          16: ((0.336, 0.351), (0.015, 0.031))}


@pytest.mark.parametrize('case', [11, 14])
@pytest.mark.parametrize('kind', mr.KINDS)
@pytest.mark.parametrize('with_tol', [False, True])
def test_restatement_in_double_agrees_with_the_reference(case, kind, with_tol):
    an = mr.case_analysis(case, kind, with_tol)
    x, steps = an.cpu('double')
    keep = an.keep('double')
    assert keep.mean() >= 0.9
    assert np.array_equal((x != 0)[keep], (an.x != 0)[keep])
    assert np.array_equal(steps[keep], an.steps[keep])
    err = float(np.max(np.abs(x - an.x)[keep])) / float(np.max(np.abs(an.x)))
    print('case %d %s tol %s: restatement against lstsq %.3g' % (case, kind, with_tol, err))
    assert err <= 1e-10


@pytest.mark.parametrize('case', mr.CASES)
def test_left_out_shares(case):
    for pi, precision in enumerate(('single', 'double')):
        for ki, kind in enumerate(mr.KINDS):
            shares = {t: mr.case_analysis(case, kind, t).left_out(precision) for t in (False, True)}
            print('case %d %s %s: fixed %.3f tol %.3f' % (case, precision, kind, shares[False], shares[True]))
            assert abs(max(shares.values()) - SHARES[case][pi][ki]) < 5e-4
            for t in (False, True):
                runs = precision == 'double' or (kind, t) in mr.SINGLE_RUNS.get(case, [])
                if runs:
                    assert shares[t] <= omp_ref.MAX_LEFT_OUT
                else:
                    assert shares[t] > omp_ref.MAX_LEFT_OUT
    if case == 13:
        assert abs(mr.case_analysis(13, 'binary', False).left_out('single') - 0.086) < 5e-4


def _random(rng, cplx, *shape):
    return rng.randn(*shape) + 1j * rng.randn(*shape) if cplx else rng.randn(*shape)


@pytest.mark.parametrize('dt', ['float32', 'float64', 'complex64', 'complex128'])
def test_restatement_degenerate_rows(dt):
    dt = np.dtype(dt)
    cplx = dt.kind == 'c'
    rng = np.random.RandomState(5)
    K, F, N = 6, 16, 4
    A = _random(rng, cplx, K, F)
    y = _random(rng, cplx, N, F)
    m = (rng.rand(N, F) < 0.8).astype(float)
    # row 1: no weight at all
    m[1] = 0
    # row 2: atom 4 would win unmasked (y = 3 a_4 + small), but all of its support is hidden in that row
    A[4] = 0
    A[4, :3] = [5, -4, 3]
    y[2] = 3 * A[4] + 0.1 * y[2]
    m[2] = 1
    m[2, :3] = 0
    x, steps = mr.restate(y, A, m, K, dtype=dt)
    x_open, _ = mr.restate(y, A, np.ones_like(m), 1, dtype=dt)
    assert np.flatnonzero(x_open[2]).tolist() == [4]
    assert np.all(x[1] == 0) and steps[1] == 0
    assert x[2, 4] == 0 and steps[2] == K - 1
    assert np.all(np.isfinite(x))
    # the rows do not see each other: the neighbours of the empty row, alone
    x02, _ = mr.restate(y[[0, 2]], A, m[[0, 2]], K, dtype=dt)
    assert np.array_equal(x02, x[[0, 2]])
    # two atoms equal on the observed channels, different on the hidden ones: the second fails the pivot test
    A3 = _random(rng, cplx, 3, F)
    A3[2] = A3[0]
    A3[2, :4] += 1.0
    m3 = np.ones((1, F))
    m3[0, :4] = 0
    y3 = _random(rng, cplx, 1, F)
    x3, steps3 = mr.restate(y3, A3, m3, 3, dtype=dt)
    xr, stepsr, _, _ = mr.reference(y3.astype(dt).astype(np.result_type(dt, np.float64)),
                                    A3.astype(dt).astype(np.result_type(dt, np.float64)), m3, 3)
    # (which of the twins is taken is a tie that a BLAS may break either way: they are folded together)
    assert steps3[0] == 2 and stepsr[0] == 2 and np.all(np.isfinite(x3))
    assert (x3[0, 0] == 0) != (x3[0, 2] == 0) and x3[0, 1] != 0

    def fold(x):
        return np.array([x[0, 0] + x[0, 2], x[0, 1]])
    assert np.max(np.abs(fold(x3) - fold(xr))) <= 1e4 * float(np.finfo(dt).eps) * np.max(np.abs(xr))


def test_bad_masks_raise_what_lasso_raises_before_the_library_is_loaded(monkeypatch):
    from decomp_amd import _hip, lasso, omp

    def no_load(*a, **k):
        raise RuntimeError('the library was loaded')
    monkeypatch.setattr(_hip, 'load', no_load)
    monkeypatch.setattr(_hip, 'handle', no_load)
    y = np.ones((4, 6), dtype=np.float32)
    A = np.ones((3, 6), dtype=np.float32)
    bad = {'complex dtype': np.ones((4, 6), dtype=np.complex64),
           'negative entry': -np.ones((4, 6), dtype=np.float32),
           'wrong shape': np.ones((4, 5), dtype=np.float32),
           '1-D of the wrong length': np.ones(5, dtype=np.float32)}
    for what, mask in bad.items():
        with pytest.raises(Exception) as e_lasso:
            lasso.solve(y, A, 0.1, mask=mask)
        with pytest.raises(Exception) as e_omp:
            omp.solve(y, A, 2, mask=mask)
        assert e_omp.type is e_lasso.type and e_omp.type is not RuntimeError, what
        assert str(e_omp.value) == str(e_lasso.value), what


def test_solve_takes_a_mask_keyword():
    from decomp_amd import omp
    p = inspect.signature(omp.solve).parameters
    assert list(p) == ['y', 'A', 'n_nonzero_coefs', 'tol', 'mask'] and p['mask'].default is None
