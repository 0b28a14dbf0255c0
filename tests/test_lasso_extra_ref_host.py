"""tests/lasso_extra_ref.py (the reference of test_gpu_lasso_extra_shapes.py) against oracle.lasso, and the conditions
the GPU file relies on, for every case it runs.  No GPU.

  the reference equals the oracle: same `it`, x within 1e-12, every shape, mask, method, real and complex
  p margin: 1 < p < K and frac(K / bound) in [0.1, 0.9], in double and in single arithmetic: the device forms the
      bound in the problem's precision, and a problem near an integer would test rounding, not the kernel
  stop margin: |m_i - 1| >= 0.05 at every check up to the stopping one, and the same `it` with the iterates rounded
      to single after every iteration -- so all four dtypes must return the reference's `it`
  support: the codes hold zeros and non-zeros
  parallel_cd at a met test: the full update is more than 100 x the limit away from the committed iterate on either
      side of the iteration, so a kernel that returns the wrong buffer fails

Measured here (the figures test_gpu_lasso_extra_shapes.py and DESIGN.md quote):
  ADMM in single-precision arithmetic against the double run, 15 iterations from x0 (rel_err), float32 / complex64:
      over   no mask   rho 0.1: 1.1e-5 / 7.2e-6   rho 1: 2.5e-6 / 1.6e-6   rho 10: 2.5e-6 / 1.6e-6
      k130   no mask   rho 0.1: 1.4e-6 / 1.9e-6   rho 1: 1.0e-6 / 1.2e-6   rho 10: 1.6e-6 / 1.6e-6
      k130   2-D mask  rho 0.1: 5.8e-7 / 3.7e-7   rho 1: 4.2e-7 / 2.5e-7   rho 10: 7.1e-7 / 7.8e-7
  4 x the largest is 4.5e-5, below the 2e-4 floor: the single-precision limit of test_admm_rho is 2e-4 in every case.
  inverse, batch (b) (rows reversed), max|round_single(inv) X - I| in real / complex: n = 257: 5.6e-8 / 5.6e-8,
      n = 300: 5.8e-8 / 5.7e-8"""
import numpy as np
import pytest

import lasso_extra_ref as ref
from oracle import lasso as olasso

DOUBLE = {False: 'float64', True: 'complex128'}
SINGLE = {False: 'float32', True: 'complex64'}


def _oracle_admm(y, A, alpha, x0, tol, maxiter, positive, mask2, rho):
    """oracle.lasso's ADMM with rho, through its private entry point (oracle.lasso.solve has no rho)."""
    s = np.sqrt(np.sum(np.real(np.conj(A) * A), axis=-1))
    n_valid = A.shape[1] if mask2 is None else np.sum(mask2, axis=-1, keepdims=True)
    it, x = olasso._admm(y, A / s[:, None], alpha / s * n_valid, x0 * s, tol * s, maxiter, positive, mask2, rho=rho)
    return it, x / s


@pytest.mark.parametrize('cplx', [False, True], ids=['real', 'complex'])
@pytest.mark.parametrize('name', list(ref.SHAPES))
def test_reference_equals_oracle_on_the_shape_cases(name, cplx):
    y, A, x0, mask1, mask2 = ref.problem(name, cplx)
    worst = 0.0
    for mname in ref.MASKS:
        for method, maxiter, rows in ref.shape_runs(name, cplx, mname):
            yc, xc, mc = ref.cut_rows(rows, y, x0, ref.pick_mask(mname, mask1, mask2))
            r = ref.solve(yc, A, ref.ALPHA[method.replace('_pos', '')], x=xc, tol=0.0, method=method,
                          maxiter=maxiter, mask=mc)
            ito, xo = olasso.solve(yc.copy(), A.copy(), ref.ALPHA[method.replace('_pos', '')], x=xc.copy(), tol=0.0,
                                   method=method, maxiter=maxiter, mask=None if mc is None else mc.copy())
            assert r.it == ito == maxiter - 1, (mname, method)
            assert r.x.shape == xo.shape and r.x.dtype == xo.dtype
            worst = max(worst, float(np.max(np.abs(r.x - xo))))
            assert np.max(np.abs(r.x - xo)) <= 1e-12, (mname, method, float(np.max(np.abs(r.x - xo))))
            assert len(r.stats) == (maxiter - 1) // 10 + 1 and min(r.stats) >= 1.0
            # support: zeros and non-zeros (parallel_cd keeps exact zeros; ADMM returns x, dense, and z is the
            # sparse one: there the zeros are those of a soft threshold applied to it)
            nz = np.count_nonzero(r.x) if method.startswith('parallel_cd') else \
                np.count_nonzero(np.abs(r.x) > 1e-3)
            assert 0 < nz < r.x.size, (mname, method, nz)
            assert not np.array_equal(r.x, xc)
    print('%s %s: max |x - oracle| = %.2e' % (name, DOUBLE[cplx], worst))


@pytest.mark.parametrize('cplx', [False, True], ids=['real', 'complex'])
@pytest.mark.parametrize('name', list(ref.SHAPES))
def test_p_margin(name, cplx):
    K = ref.SHAPES[name][2]
    for dt in (DOUBLE[cplx], SINGLE[cplx]):
        y, A, x0, mask1, mask2 = ref.problem(name, cplx, dt)
        for mask in (None, mask1):
            for arith in (DOUBLE[cplx], SINGLE[cplx]):
                ratio, p = ref.pcd_width(A, mask, arith)
                assert 1 < p < K, (dt, arith, ratio)
                assert 0.1 <= ratio - p <= 0.9, (dt, arith, ratio)
        r = ref.solve(y, A, 0.2, tol=0.0, maxiter=1, mask=mask2)     # a 2-D mask does not enter p
        ratio, p = ref.pcd_width(A, None)
        assert r.p == p and abs(r.ratio - ratio) < 1e-12


@pytest.mark.parametrize('key', sorted(ref.STOP_TOL), ids=lambda k: '%s-%s-%s-%s' % (
    k[0], 'complex' if k[1] else 'real', k[2], 'mask2d' if k[3] else 'nomask'))
def test_stop_margin(key):
    name, cplx, method, masked = key
    tol = ref.STOP_TOL[key]
    dtypes = [DOUBLE[cplx]] if name == 'k130' else [DOUBLE[cplx], SINGLE[cplx]]
    for dt in dtypes:
        y, A, x0, mask1, mask2 = ref.problem(name, cplx, dt)
        mask = mask2 if masked else None
        r = ref.solve(y, A, ref.ALPHA[method], tol=tol, method=method, maxiter=400, mask=mask)
        assert 0 < r.it < 399 and r.it % 10 == 0
        assert all(abs(m - 1.0) >= 0.05 for m in r.stats), r.stats
        assert all(m > 1.0 for m in r.stats[:-1]) and r.stats[-1] < 1.0
        rr = ref.solve(y, A, ref.ALPHA[method], tol=tol, method=method, maxiter=400, mask=mask, round_iterates=True)
        assert rr.it == r.it
        assert all(abs(m - 1.0) >= 0.05 for m in rr.stats), rr.stats
        if dt == DOUBLE[cplx]:
            for t, maxiter, it_want in ref.stop_runs(r.it):
                t = tol if t is None else t
                q = ref.solve(y, A, ref.ALPHA[method], tol=t, method=method, maxiter=maxiter, mask=mask)
                ito, xo = olasso.solve(y.copy(), A.copy(), ref.ALPHA[method], tol=t, method=method, maxiter=maxiter,
                                       mask=None if mask is None else mask.copy())
                assert q.it == ito == it_want, (t, maxiter, q.it, ito)
                assert np.max(np.abs(q.x - xo)) <= 1e-12
        zero = ref.solve(y, A, ref.ALPHA[method], tol=1.0e3, method=method, maxiter=50, mask=mask)
        assert zero.it == 0 and zero.stats[0] <= 0.95
        if method == 'parallel_cd':
            for q in (r, zero):
                assert np.array_equal(q.x, q.full)
                for other in (q.before, q.after):
                    assert ref.rel_err(other, q.full) > 100.0 * ref.LIMIT[dt], ref.rel_err(other, q.full)


@pytest.mark.parametrize('cplx', [False, True], ids=['real', 'complex'])
@pytest.mark.parametrize('name,mname', ref.RHO_CASES)
def test_rho_reference_and_the_cost_of_single_precision(name, mname, cplx):
    """ADMM with rho: the reference equals the oracle's private entry point, and the same iteration in single-precision
    arithmetic stays far below the 2e-4 floor (figures in the module docstring)."""
    y, A, x0, mask1, mask2 = ref.problem(name, cplx)
    rows = ref.MASKED_ADMM_ROWS if mname == 'mask2d' else None
    y, x0, mask = ref.cut_rows(rows, y, x0, ref.pick_mask(mname, mask1, mask2))
    for rho in ref.RHOS:
        r = ref.solve(y, A, 0.05, x=x0, tol=0.0, method='admm', maxiter=ref.RHO_ITER, mask=mask, rho=rho)
        ito, xo = _oracle_admm(y, A, 0.05, x0, 0.0, ref.RHO_ITER, False, mask, rho)
        assert r.it == ito == ref.RHO_ITER - 1
        assert np.max(np.abs(r.x - xo)) <= 1e-12
        y1, A1, x1 = y.astype(SINGLE[cplx]), A.astype(SINGLE[cplx]), x0.astype(SINGLE[cplx])
        d = ref.solve(y1, A1, 0.05, x=x1, tol=0.0, method='admm', maxiter=ref.RHO_ITER, mask=mask, rho=rho)
        w = ref.solve(y1, A1, 0.05, x=x1, tol=0.0, method='admm', maxiter=ref.RHO_ITER, mask=mask, rho=rho,
                      dtype=SINGLE[cplx])
        assert w.x.dtype == np.dtype(SINGLE[cplx]) and d.x.dtype == np.dtype(DOUBLE[cplx])
        e = ref.rel_err(w.x, d.x)
        print('%s %s %s rho %g: single arithmetic against double %.2e' % (name, mname, SINGLE[cplx], rho, e))
        assert 0.0 < e and 4.0 * e < 2e-4
    # different rho, different iterate: the keyword is live
    a = ref.solve(y, A, 0.05, x=x0, tol=0.0, method='admm', maxiter=ref.RHO_ITER, mask=mask, rho=0.1)
    assert ref.rel_err(a.x, r.x) > 1e-3


def test_fallback_problem_has_p_at_most_one():
    for cplx, dt in ((False, 'float32'), (True, 'complex128')):
        A = ref.parallel_atoms(130, 70, cplx, dt)
        mask1 = ref.problem('k33', cplx)[3]
        for mask in (None, mask1):
            for arith in (DOUBLE[cplx], SINGLE[cplx]):
                ratio, p = ref.pcd_width(A, mask, arith)
                assert p <= 1 and ratio <= 1.9, (dt, arith, ratio)     # (|G_ij| <= 1: the ratio is 1 at the least)
        y = np.ones((3, 70), dt)
        with pytest.raises(TypeError):
            ref.solve(y, A, 0.1, mask=np.ones((3, 70)))
        with pytest.raises(ValueError):
            ref.solve(y, A, 0.1)


@pytest.mark.parametrize('n', [257, 300])
def test_inverse_batches(n):
    """Batch (b): Gauss-Jordan with partial pivoting takes the pivot of column k from row n - 1 - k, for n = 300 the
    first 44 from rows >= 256, the only non-zero entries of their columns; all three are well conditioned, so np.linalg.inv in double is a reference to 1e-10."""
    for dt in ('float32', 'complex128'):
        a, b, c = ref.inverse_batches(n, dt).astype(ref._double(np.dtype(dt)))
        for m, bound in ((a, 1e5), (b, 10.0), (c, 10.0)):
            assert np.linalg.cond(m) < bound
        W = b.copy()
        pivots = []
        for k in range(n):                       # the elimination as inv_batched_kernel does it
            mag = np.abs(W[k:, k].real) + np.abs(W[k:, k].imag)
            p = k + int(np.argmax(mag))
            pivots.append(p)
            W[[k, p]] = W[[p, k]]
            W[k] = W[k] / W[k, k]
            col = W[:, k].copy()
            col[k] = 0
            W -= col[:, None] * W[k]
        assert pivots[:(n - 1) // 2] == [n - 1 - k for k in range((n - 1) // 2)]
        assert all(p >= 256 for p in pivots[:n - 256])
        # ... and nowhere else: a search over the rows < 256 alone would divide by zero
        assert not b[:256, :n - 256].any()
        inv1 = np.linalg.inv(b).astype(ref._single(np.dtype(dt)))
        res = float(np.max(np.abs(inv1.astype(b.dtype).dot(b) - np.eye(n))))
        print('n = %d %s: residual of the rounded double inverse %.2e' % (n, dt, res))
        assert res < 1e-6
