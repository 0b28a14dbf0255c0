"""tests/cd_ref.py (the cheap coordinate-descent reference of test_gpu_lasso_cd.py) against oracle.lasso.solve, the
as-written restatement of the reference's sweep: same iteration counts, codes within 1e-12.  No GPU."""
import numpy as np
import pytest

import cd_ref
from oracle import lasso as olasso

SHAPES = [(7, 30, 12), (5, 9, 20)]        # (N, F, K): K < F and K > F


def _problem(dt, shape, positive, seed):
    rng = np.random.RandomState(seed)
    N, F, K = shape
    cplx = dt == 'complex128'

    def randn(*s):
        return (rng.randn(*s) + 1j * rng.randn(*s)) if cplx else rng.randn(*s)
    A = randn(K, F).astype(dt)
    xt = randn(N, K) * (rng.uniform(size=(N, K)) < 0.2)
    if positive:
        xt = np.abs(xt)
    y = (xt @ A + 0.05 * randn(N, F)).astype(dt)
    x0 = (xt + 0.3 * randn(N, K)).astype(dt)
    mask1 = (rng.uniform(size=F) > 0.3).astype(np.float64)
    mask2 = (rng.uniform(size=(N, F)) > 0.3).astype(np.float64)
    return y, A, x0, mask1, mask2


CASES = [(dt, method) for dt in ('float64', 'complex128') for method in ('cd', 'cd_pos')
         if not (dt == 'complex128' and method == 'cd_pos')]


@pytest.mark.parametrize('shape', SHAPES)
@pytest.mark.parametrize('start', ['zeros', 'given'])
@pytest.mark.parametrize('mname', ['nomask', 'mask1d', 'mask2d'])
@pytest.mark.parametrize('dt,method', CASES)
def test_helper_equals_oracle(dt, method, mname, start, shape):
    y, A, x0, mask1, mask2 = _problem(dt, shape, method == 'cd_pos', seed=shape[2])
    mask = {'nomask': None, 'mask1d': mask1, 'mask2d': mask2}[mname]
    x_in = None if start == 'zeros' else x0
    seen = set()
    for tol, maxiter in ((1e-3, 200), (1e-7, 200), (0.0, 13), (1e-7, 11)):
        ito, xo = olasso.solve(y.copy(), A.copy(), 0.05, x=None if x_in is None else x_in.copy(), tol=tol,
                               method=method, maxiter=maxiter, mask=None if mask is None else mask.copy())
        if mname == 'mask2d':
            res = cd_ref.solve_masked(y, A, 0.05, mask, x=x_in, tol=tol, method=method, maxiter=maxiter)
        else:
            res = cd_ref.solve(y, A, 0.05, x=x_in, tol=tol, method=method, maxiter=maxiter, mask=mask)
        assert res.it == ito, (tol, maxiter, res.it, ito)
        assert res.x.shape == xo.shape and res.x.dtype == xo.dtype
        assert np.max(np.abs(res.x - xo)) <= 1e-12, (tol, maxiter, float(np.max(np.abs(res.x - xo))))
        assert len(res.moved) == res.it + 1 and len(res.stop) == res.it // 10 + 1
        # the recorded stop quantities are the decisions the run took
        assert all(q >= 0.0 for q in res.stop[:-1])
        if res.it < maxiter - 1:
            assert res.stop[-1] < 0.0
        elif res.it % 10 != 0:
            assert res.stop[-1] >= 0.0
        seen.add(ito)
    assert len(seen) > 1          # the four runs did not all end at the same sweep


def test_helper_snapshots_moved_share_and_working_precision():
    """`keep` hands back the codes after the named sweeps (what a shorter solve returns), `moved` counts the
    non-zero steps, and `dtype=` runs in single precision: close to, but not equal to, the double run."""
    y, A, x0, mask1, _ = _problem('float64', (7, 30, 12), False, seed=1)
    full = cd_ref.solve(y, A, 0.05, x=np.ones_like(x0), tol=0.0, maxiter=12, keep=(0, 3))
    for i in (0, 3):
        part = cd_ref.solve(y, A, 0.05, x=np.ones_like(x0), tol=0.0, maxiter=i + 1)
        assert np.array_equal(full.after[i], part.x)
    assert full.moved[0] == 1.0 and full.it == 11 and len(full.stop) == 2
    zero = cd_ref.solve(np.zeros_like(y), A, 0.05, tol=1e-3, maxiter=30)
    assert zero.it == 0 and zero.moved == [0.0] and not zero.x.any()
    for dt, wdt in (('float64', 'float32'), ('complex128', 'complex64')):
        y, A, x0, mask1, mask2 = _problem(dt, (7, 30, 12), False, seed=2)
        for fn, kw in ((cd_ref.solve, {'mask': mask1}), (cd_ref.solve_masked, {'mask': mask2})):
            d = fn(y, A, 0.05, tol=0.0, maxiter=5, **kw)
            w = fn(y, A, 0.05, tol=0.0, maxiter=5, dtype=wdt, **kw)
            assert w.x.dtype == np.dtype(wdt) and d.x.dtype == np.dtype(dt)
            assert 0.0 < cd_ref.err(w.x, d.x) < 1e-5
