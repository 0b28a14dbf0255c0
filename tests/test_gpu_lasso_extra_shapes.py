"""GPU: lasso.solve(method='parallel_cd' | 'admm' [+ '_pos']) and math_utils.linalg.inv at the shapes where their
kernels change path, against tests/lasso_extra_ref.py (pinned to oracle.lasso by test_lasso_extra_ref_host.py, which
also proves, on the CPU, every margin this file relies on: p away from an integer, stop statistics away from 1, the
full update of parallel_cd away from the committed iterate).

shape (N, F, K)         what it reaches
tall  (160, 40, 20)     K <= 32: the 32-wide tall tiles under the step epilogues (fp32 TIER_TALL, fp64 F64_TALL32)
k33   (200, 70, 33)     N and K off the tile grid, one atom past the 32-wide tile; F = 64 + 6: a second, partial pass
                        of admm_mask_system_kernel's lane loop
k130  (150, 150, 130)   two column tiles, the second nearly empty; F of two passes and a part
k260  (130, 600, 260)   K > 256: a second pass of every `+= 256` loop (admm_mask_step_kernel, gj_batched_kernel); the
                        float32 TILE_SMALL Gram branch; F > 512: a split reduction.  Masked ADMM takes 16 rows
over  (40, 48, 260)     K > F: A A^H is singular and the inverse rests on rho; F < 64
test_step_product_routes holds the float32 / float64 step product [N, K].[K, K] of each shape to these tiles, so a
later routing change cannot turn the shapes into duplicates of each other.

Every solve starts from a non-zero x0 unless it tests the stop (those start from x = None, as the tolerances in
lasso_extra_ref.STOP_TOL were chosen); limits are test_gpu_lasso_extra.py's: 2e-4 single, 1e-9 double, of
max|x - ref| / max(1, max|ref|).  Every error is printed (pytest -s)."""
import ctypes
import functools

import numpy as np
import pytest

import lasso_extra_ref as ref

pytestmark = pytest.mark.gpu

# the launched tile (BM, BN) of the step product, float32 (core 0) and float64 (core 1)
STEP_TILE = {'tall': ((128, 32), (128, 32)), 'k33': ((64, 64), (128, 64)), 'k130': ((64, 64), (64, 64)),
             'k260': ((64, 64), (64, 64)), 'over': ((64, 64), (64, 128))}


def _cplx(dt):
    return np.dtype(dt).kind == 'c'


@functools.lru_cache(maxsize=None)
def _problem(name, dt):
    arrays = ref.problem(name, _cplx(dt), dt)
    for a in arrays:
        a.setflags(write=False)
    return arrays


def _solve(y, A, alpha, **kw):
    """lasso.solve on copies, with a check that it left the caller's arrays alone."""
    from decomp_amd import lasso
    given = dict((k, v) for k, v in dict(kw, y=y, A=A).items() if isinstance(v, np.ndarray))
    copies = dict((k, v.copy()) for k, v in given.items())
    kw.update((k, v) for k, v in copies.items() if k in kw)
    it, x = lasso.solve(copies['y'], copies['A'], alpha, **kw)
    for k, v in given.items():
        assert np.array_equal(copies[k], v), k
    return it, x


@pytest.mark.parametrize('name', list(ref.SHAPES))
def test_step_product_routes(name):
    from decomp_amd import _hip
    N, F, K = ref.SHAPES[name]
    for dtype_code, want in zip((0, 1), STEP_TILE[name]):
        out = (ctypes.c_int32 * 13)()
        rc = _hip.load().dcp_debug_gemm_route(dtype_code, 1, N, K, K, 0, 0, 0, 0, 0, 0,
                                              ctypes.cast(out, ctypes.c_void_p))
        assert rc == 0 and out[0] == dtype_code            # the MFMA core of the dtype, not the generic one
        assert (out[2], out[3]) == want, (name, dtype_code, out[2], out[3])
        assert N % out[2] != 0 and K % out[3] != 0         # bounds-checked tiles in both directions


@pytest.mark.parametrize('mname', ref.MASKS)
@pytest.mark.parametrize('dt', ref.DTYPES)
@pytest.mark.parametrize('name', list(ref.SHAPES))
def test_shapes_against_the_reference(name, dt, mname):
    """Non-zero start, tol = 0, maxiter 10 / 11: parallel_cd returns xb[maxiter & 1], even and odd.
    Measured on an MI355X, the largest error over all cases: float32 4.0e-6, complex64 2.5e-6, float64 1.7e-14,
    complex128 1.2e-14 (all four on `over`, ADMM)."""
    y, A, x0, mask1, mask2 = _problem(name, dt)
    for method, maxiter, rows in ref.shape_runs(name, _cplx(dt), mname):
        yc, xc, mc = ref.cut_rows(rows, y, x0, ref.pick_mask(mname, mask1, mask2))
        kw = dict(x=xc, tol=0.0, method=method, maxiter=maxiter, mask=mc)
        alpha = ref.ALPHA[method.replace('_pos', '')]
        it, x = _solve(yc, A, alpha, **kw)
        r = ref.solve(yc, A, alpha, **kw)
        e = ref.rel_err(x, r.x)
        print('%s %s %s %s maxiter %d: it %d, error %.2e' % (name, dt, mname, method, maxiter, it, e))
        assert it == r.it == maxiter - 1
        assert x.dtype == np.dtype(dt) and x.shape == xc.shape
        assert e < ref.LIMIT[dt], (method, e)


STOP_CASES = [('k33', dt, method, masked) for dt in ref.DTYPES for method in ('parallel_cd', 'admm')
              for masked in (False, True)] + \
             [('k130', 'float64', method, masked) for method in ('parallel_cd', 'admm') for masked in (False, True)]


@pytest.mark.parametrize('name,dt,method,masked', STOP_CASES,
                         ids=['%s-%s-%s-%s' % (c[0], c[1], c[2], 'mask2d' if c[3] else 'nomask') for c in STOP_CASES])
def test_stop_bookkeeping(name, dt, method, masked):
    """The reference stops at i*: maxiter = i* runs out just before the check that is met, i* + 1 meets it on the very
    last iteration, i* + 5 meets it with iterations to spare, and tol = 1e3 is met at iteration 0.  `it` equals the
    reference's in every dtype; at a met test parallel_cd returns the full update, not the committed iterate (the
    host test keeps the two more than 100 limits apart)."""
    y, A, x0, mask1, mask2 = _problem(name, dt)
    mask = mask2 if masked else None
    tol = ref.STOP_TOL[(name, _cplx(dt), method, masked)]
    alpha = ref.ALPHA[method]
    i_star = ref.solve(y, A, alpha, tol=tol, method=method, maxiter=400, mask=mask).it
    assert 0 < i_star < 399
    for t, maxiter, it_want in ref.stop_runs(i_star):
        kw = dict(tol=tol if t is None else t, method=method, maxiter=maxiter, mask=mask)
        it, x = _solve(y, A, alpha, **kw)
        r = ref.solve(y, A, alpha, **kw)
        e = ref.rel_err(x, r.x)
        print('%s %s %s masked %d tol %g maxiter %d: it %d (reference %d), error %.2e'
              % (name, dt, method, masked, kw['tol'], maxiter, it, r.it, e))
        assert r.it == it_want
        if method == 'parallel_cd' and it_want < maxiter - 1:
            assert np.array_equal(r.x, r.full)
        assert it == it_want
        assert x.dtype == np.dtype(dt) and e < ref.LIMIT[dt], e


@pytest.mark.parametrize('rho', ref.RHOS)
@pytest.mark.parametrize('dt', ref.DTYPES)
def test_admm_rho(dt, rho):
    """rho = 0.1, 1, 10 on `over` (K > F: the unpivoted Gauss-Jordan on A A^H + rho I rests on rho alone) and `k130`,
    without a mask, and on 16 rows of `k130` with a 2-D mask; 15 iterations from x0.  Double: 1e-9.  Single: 4 x the
    error of the reference run in single-precision arithmetic (Gram matrix, stored inverse and iterates in single)
    against the double reference, and 2e-4 at the least.  That error, measured on the CPU
    (test_lasso_extra_ref_host.py), is 1.1e-5 at most (`over`, float32, rho = 0.1; k130: 1.9e-6 at most; masked:
    7.8e-7), so the limit is 2e-4 in every case."""
    single = dt in ('float32', 'complex64')
    for name, mname in ref.RHO_CASES:
        y, A, x0, mask1, mask2 = _problem(name, dt)
        rows = ref.MASKED_ADMM_ROWS if mname == 'mask2d' else None
        yc, xc, mc = ref.cut_rows(rows, y, x0, ref.pick_mask(mname, mask1, mask2))
        kw = dict(x=xc, tol=0.0, method='admm', maxiter=ref.RHO_ITER, mask=mc, rho=rho)
        r = ref.solve(yc, A, 0.05, **kw)
        limit = ref.LIMIT[dt]
        if single:
            e1 = ref.rel_err(ref.solve(yc, A, 0.05, dtype=dt, **kw).x, r.x)
            limit = max(limit, 4.0 * e1)
        it, x = _solve(yc, A, 0.05, **kw)
        e = ref.rel_err(x, r.x)
        print('%s %s %s rho %g: error %.2e, limit %.2e' % (name, mname, dt, rho, e, limit))
        assert it == r.it == ref.RHO_ITER - 1 and x.dtype == np.dtype(dt)
        assert e < limit, (name, mname, e, limit)


@pytest.mark.parametrize('dt', ['float32', 'complex128'])
def test_fallback_is_coordinate_descent(dt):
    """130 nearly parallel atoms: p <= 1, so parallel_cd is plain coordinate descent on the same Gram matrix -- the
    bytes of method='cd' without a mask and with a 1-D mask -- and with a 2-D mask the reference's TypeError."""
    cplx = _cplx(dt)
    N, F, K = 50, 70, 130
    A = ref.parallel_atoms(K, F, cplx, dt)
    rng = np.random.RandomState(4)
    y = (rng.randn(N, F) + (1j * rng.randn(N, F) if cplx else 0.0)).astype(dt)
    mask1 = _problem('k33', dt)[3]
    mask2 = (rng.uniform(size=(N, F)) > 0.3).astype(mask1.dtype)
    methods = ['parallel_cd'] + ([] if cplx else ['parallel_cd_pos'])
    for mask in (None, mask1):
        assert ref.pcd_width(A, mask, dt)[1] <= 1
        for method in methods:
            kw = dict(tol=1e-3, maxiter=12, mask=mask)
            it, x = _solve(y, A, 0.01, method=method, **kw)
            itc, xc = _solve(y, A, 0.01, method=method.replace('parallel_cd', 'cd'), **kw)
            assert it == itc and x.tobytes() == xc.tobytes()
            assert np.count_nonzero(x) > 0
    with pytest.raises(TypeError):
        _solve(y, A, 0.01, method='parallel_cd', tol=1e-3, maxiter=12, mask=mask2)


@pytest.mark.parametrize('dt', ['float32', 'complex128'])
def test_batch_layout_and_repeat(dt):
    """y [5, 40, F] with a mask [5, 40, F] is the flattened [200, F] call; a call repeated gives the same bytes; an
    empty batch returns an empty [0, K]."""
    y, A, x0, mask1, mask2 = _problem('k33', dt)
    N, F, K = ref.SHAPES['k33']
    for method in ('parallel_cd', 'admm'):
        kw = dict(tol=0.0, method=method, maxiter=11)
        it, x = _solve(y, A, ref.ALPHA[method], x=x0, mask=mask2, **kw)
        it3, x3 = _solve(y.reshape(5, 40, F), A, ref.ALPHA[method], x=x0.reshape(5, 40, K),
                         mask=mask2.reshape(5, 40, F), **kw)
        assert it3 == it and x3.shape == (5, 40, K) and x3.tobytes() == x.tobytes()
        it2, x2 = _solve(y, A, ref.ALPHA[method], x=x0, mask=mask2, **kw)
        assert it2 == it and x2.tobytes() == x.tobytes()
        ite, xe = _solve(y[:0], A, ref.ALPHA[method], **kw)
        assert xe.shape == (0, K) and xe.dtype == np.dtype(dt)
        ite, xe = _solve(y[:0].reshape(0, 4, F), A, ref.ALPHA[method], mask=mask2[:0].reshape(0, 4, F), **kw)
        assert xe.shape == (0, 4, K)


@pytest.mark.parametrize('dt', ref.DTYPES)
def test_inverse_beyond_256_rows(dt):
    """linalg.inv at n = 257 and 300: inv_batched_kernel's pivot search and row loops (`+= 256`) make a second pass.
    Batch (a) random, (b) diagonally dominant with its rows reversed -- the pivot of column k is found in row
    n - 1 - k, for n = 300 the first 44 in rows >= 256 -- (c) A A^H + I.  Against np.linalg.inv in double with the
    limits of test_linalg_inv_matches_numpy (2e-4 / 1e-10 of max(1, max|inverse|)); for (b) in single also the
    residual max|inv(X) X - I| against 4 x that of the double inverse rounded to single (measured on the CPU:
    5.6e-8 .. 5.8e-8, so the limit is about 2.3e-7; on an MI355X the kernel's residual equals it to three digits)."""
    from decomp_amd.math_utils import linalg
    single = dt in ('float32', 'complex64')
    tol = 2e-4 if single else 1e-10
    for n in (257, 300):
        X = ref.inverse_batches(n, dt)
        Xd = X.astype(np.complex128 if _cplx(dt) else np.float64)
        keep = X.copy()
        got = linalg.inv(X)
        want = np.linalg.inv(Xd)
        assert np.array_equal(X, keep)
        assert got.dtype == np.dtype(dt) and got.shape == X.shape
        for b, tag in enumerate('abc'):
            e = float(np.max(np.abs(got[b] - want[b]))) / max(1.0, float(np.max(np.abs(want[b]))))
            print('inv n = %d %s (%s): error %.2e' % (n, dt, tag, e))
            assert e <= tol, (n, tag, e)
        if single:
            eye = np.eye(n)
            res = float(np.max(np.abs(got[1].astype(Xd.dtype).dot(Xd[1]) - eye)))
            res_ref = float(np.max(np.abs(want[1].astype(dt).astype(Xd.dtype).dot(Xd[1]) - eye)))
            print('inv n = %d %s (b): residual %.2e, of the rounded double inverse %.2e' % (n, dt, res, res_ref))
            assert res <= 4.0 * res_ref
