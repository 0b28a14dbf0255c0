"""GPU: approximate K-SVD (decomp_amd.ksvd, dcp_ksvd_sweep_*, dcp_ksvd_step_*) against the NumPy reference of
ksvd_ref.py.

The sweep is smooth (no discrete decisions), so it is compared value by value, in all four dtypes, against the
double sweep on the same single-exact inputs.  The bounds are not fixed in advance: 4 x the error the NumPy sweep in
the working dtype shows against double (the factor covers the other summation order of the chunked reduction), floor
64 eps; D relative to 1, X relative to max|x_ref| (ksvd_ref.sweep_bounds).  The loop contains the greedy coder, so
end to end the OBJECTIVE is compared (a row whose OMP margin is below omp_ref.DELTA may choose another atom, which
changes every later D but the objective only at second order); D and X only over iterations in which every row's
margin in the double reference stays above DELTA."""
import ctypes
import os
import re

import numpy as np
import pytest

import ksvd_ref
import omp_ref

pytestmark = pytest.mark.gpu

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
DTYPES = ['float32', 'float64', 'complex64', 'complex128']
ERR_INVALID = -1


def _constant(name):
    text = open(os.path.join(ROOT, 'decomp_amd', 'csrc', 'ksvd.hpp')).read()
    return int(re.search(r'constexpr int %s = (\d+);' % name, text).group(1))


C = _constant('kKsvdChunk')            # support rows per pass-1 partial
LDS_BYTES = _constant('kKsvdLdsBytes')   # a pass-2 row longer than this is read twice instead of kept in LDS


def _precision(dt):
    dt = np.dtype(dt)
    return 'single' if dt.itemsize == (8 if dt.kind == 'c' else 4) else 'double'


def _sweep(y, x, D, row_nnz_max=None, expect_rc=0):
    """dcp_ksvd_sweep_* on host arrays of one dtype: (x, D, maxdiff)."""
    import torch
    from decomp_amd import _arrays, _hip
    yt = torch.from_numpy(np.ascontiguousarray(y)).cuda()
    xt = torch.from_numpy(np.ascontiguousarray(x)).cuda()
    Dt = torch.from_numpy(np.ascontiguousarray(D)).cuda()
    N, F = y.shape
    K = D.shape[0]
    lib, h = _arrays.lib_handle(yt)
    md = ctypes.c_double(-1.0)
    name = 'dcp_ksvd_sweep_' + _arrays.suffix(yt)
    rc = getattr(lib, name)(h, _arrays.ptr(yt), _arrays.ptr(xt), _arrays.ptr(Dt), N, F, K,
                            K if row_nnz_max is None else row_nnz_max, ctypes.byref(md))
    if expect_rc != 0:
        assert rc == expect_rc, rc
        return xt.cpu().numpy(), Dt.cpu().numpy(), lib.dcp_last_error_string(h).decode()
    _hip.check(h, rc, name)
    return xt.cpu().numpy(), Dt.cpu().numpy(), md.value


def _step(y, D, s, coef_tol=-1.0):
    """dcp_ksvd_step_* on host arrays: (x, D, maxdiff, it).  x starts as NaN: the coder writes all of it."""
    import torch
    from decomp_amd import _arrays, _hip
    yt = torch.from_numpy(np.ascontiguousarray(y)).cuda()
    Dt = torch.from_numpy(np.ascontiguousarray(D)).cuda()
    N, F = y.shape
    K = D.shape[0]
    xt = torch.full((N, K), float('nan'), dtype=yt.dtype, device=yt.device)
    lib, h = _arrays.lib_handle(yt)
    md, it = ctypes.c_double(-1.0), ctypes.c_int(-1)
    name = 'dcp_ksvd_step_' + _arrays.suffix(yt)
    rc = getattr(lib, name)(h, _arrays.ptr(yt), _arrays.ptr(xt), _arrays.ptr(Dt), N, F, K, int(s), float(coef_tol),
                            ctypes.byref(md), ctypes.byref(it))
    _hip.check(h, rc, name)
    return xt.cpu().numpy(), Dt.cpu().numpy(), md.value, it.value


def _normalised_on_gpu(D):
    import torch
    from decomp_amd import _arrays
    Dt = torch.from_numpy(np.ascontiguousarray(D)).cuda()
    return _arrays.l2_normalize_(Dt, strict=True).cpu().numpy()


def _rel_resid(y, x, D):
    return float(np.sqrt(ksvd_ref.objective(y, x, D)))


# ---- 1 and 3: the sweep against the double reference, and monotone ------------------------------------------------
def _cases_for(dt):
    return [c for c in sorted(ksvd_ref.CASES) if ksvd_ref.CASES[c][5] == (np.dtype(dt).kind == 'c')]


SWEEP_PARAMS = [(dt, c, st) for dt in DTYPES for c in _cases_for(dt) for st in ('planted', 'random')]


@pytest.mark.parametrize('dt,case,start', SWEEP_PARAMS)
def test_sweep_parity_and_monotone(dt, case, start):
    dt = np.dtype(dt)
    prec = _precision(dt)
    y, x, D = ksvd_ref.sweep_inputs(case, start)
    S = ksvd_ref.CASES[case][4]
    xr, Dr = ksvd_ref.sweep_reference(case, start, 'double')
    b_d, b_x, b_r = ksvd_ref.sweep_bounds(case, start, prec)
    xg, Dg, md = _sweep(y.astype(dt), x.astype(dt), D.astype(dt), row_nnz_max=S)
    assert xg.dtype == dt and Dg.dtype == dt
    err_d = float(np.max(np.abs(Dg - Dr)))
    err_x = float(np.max(np.abs(xg - xr))) / float(np.max(np.abs(xr)))
    r_before, r_ref, r_gpu = _rel_resid(y, x, D), _rel_resid(y, xr, Dr), _rel_resid(y, xg, Dg)
    md_ref = float(np.max(np.abs(Dr - D)))
    print('case %d %s %s: D error %.3g (bound %.3g); x error %.3g (bound %.3g); |y - xD|/|y| %.6g -> %.6g '
          '(reference %.6g, difference %.3g, bound %.3g); maxdiff %.6g (reference %.6g)'
          % (case, start, dt.name, err_d, b_d, err_x, b_x, r_before, r_gpu, r_ref, abs(r_gpu - r_ref), b_r, md,
             md_ref))
    assert np.all(np.isfinite(xg)) and np.all(np.isfinite(Dg))
    assert np.array_equal(xg == 0, xr == 0) or np.all((xg != 0) <= (x != 0))
    assert err_d <= b_d
    assert err_x <= b_x
    assert abs(r_gpu - r_ref) <= b_r                     # the maintained residual, through |Y - X D| on the host
    assert r_gpu <= r_before + b_r                       # monotone, up to rounding
    assert r_gpu < r_before
    assert abs(md - md_ref) <= b_d
    assert abs(md - float(np.max(np.abs(Dg - D.astype(dt))))) <= 4 * float(np.finfo(dt).eps)


# ---- 2: shapes where the kernels can go wrong -----------------------------------------------------------------------
def _random(rng, cplx, *shape):
    return rng.randn(*shape) + 1j * rng.randn(*shape) if cplx else rng.randn(*shape)


def _hand_built(seed, N, F, sizes, cplx, fill=0.1):
    """y [N, F], D [K, F] random, x [N, K] with column q holding sizes[q] non-zeros (None: about fill * N) in random
    rows; all single-exact, in double."""
    rng = np.random.RandomState(seed)
    K = len(sizes)
    y, D = omp_ref.single_exact(_random(rng, cplx, N, F), ksvd_ref.normalise(_random(rng, cplx, K, F)))
    x = np.zeros((N, K), dtype=y.dtype)
    for q, sz in enumerate(sizes):
        n = int(rng.binomial(N, fill)) if sz is None else min(sz, N)
        rows = rng.choice(N, n, replace=False)
        x[rows, q] = (1 + rng.rand(n)) * rng.choice([-1, 1], n) * (np.exp(2j * np.pi * rng.rand(n)) if cplx else 1)
    x = omp_ref.single_exact(x, x)[0]
    return y, x, D


def _check_hand_built(dt, y, x, D, tag):
    dt = np.dtype(dt)
    eps = float(np.finfo(dt).eps)
    xr, Dr, _ = ksvd_ref.sweep(y, x, D)
    xw, Dw, _ = ksvd_ref.sweep(y.astype(dt), x.astype(dt), D.astype(dt))
    xmax = max(float(np.max(np.abs(xr))), 1e-300)
    b_d = max(4 * float(np.max(np.abs(Dw - Dr))), 64 * eps)
    b_x = max(4 * float(np.max(np.abs(xw - xr))) / xmax, 64 * eps)
    xg, Dg, md = _sweep(y.astype(dt), x.astype(dt), D.astype(dt))
    err_d = float(np.max(np.abs(Dg - Dr)))
    err_x = float(np.max(np.abs(xg - xr))) / xmax
    print('%s %s: D error %.3g (bound %.3g); x error %.3g (bound %.3g)' % (tag, dt.name, err_d, b_d, err_x, b_x))
    assert np.all(np.isfinite(xg)) and np.all(np.isfinite(Dg))
    assert np.all((xg != 0) <= (x != 0))
    for k in range(D.shape[0]):
        if not np.any(x[:, k] != 0):
            assert np.array_equal(Dg[k], D[k].astype(dt)), 'atom %d is used by no row but changed' % k
    assert err_d <= b_d
    assert err_x <= b_x
    assert abs(md - float(np.max(np.abs(Dr - D)))) <= b_d
    return xg, Dg


# the vector-load tail and more than one pass per row; 260 and 1028 keep 16-byte rows in every dtype
ROW_LENGTHS = [1, 3, 50, 257, 260, 1025, 1028]
SUPPORTS = [0, 1, C, C + 1, 2000]       # 2000 = N: a dense column, many chunks


@pytest.mark.parametrize('dt', DTYPES)
@pytest.mark.parametrize('F', ROW_LENGTHS)
def test_row_lengths(dt, F):
    """N = 300, K = 6; the first column C + 1 rows (two chunks), the last one row."""
    y, x, D = _hand_built(40 + F, 300, F, [C + 1, None, None, 0, None, 1], np.dtype(dt).kind == 'c')
    _check_hand_built(dt, y, x, D, 'F = %d' % F)


@pytest.mark.parametrize('dt', DTYPES)
@pytest.mark.parametrize('rot', range(len(SUPPORTS)))
def test_support_sizes_first_middle_last(dt, rot):
    """N = 2000, F = 50, K = 7: the first, middle and last column take three consecutive entries of SUPPORTS; over
    the five rotations each size sits in each of the three places."""
    sz = [SUPPORTS[(rot + q) % len(SUPPORTS)] for q in range(3)]
    y, x, D = _hand_built(60 + rot, 2000, 50, [sz[0], None, None, sz[1], None, None, sz[2]],
                          np.dtype(dt).kind == 'c', fill=0.05)
    _check_hand_built(dt, y, x, D, 'supports %s' % sz)


@pytest.mark.parametrize('dt', DTYPES)
def test_one_row_and_one_atom(dt):
    cplx = np.dtype(dt).kind == 'c'
    y, x, D = _hand_built(71, 1, 20, [1, 0, 1], cplx)
    _check_hand_built(dt, y, x, D, 'N = 1')
    y, x, D = _hand_built(72, 150, 20, [C + 3], cplx)
    _check_hand_built(dt, y, x, D, 'K = 1')
    y, x, D = _hand_built(73, 1, 1, [1], cplx)
    _check_hand_built(dt, y, x, D, 'N = F = K = 1')


@pytest.mark.parametrize('dt', DTYPES)
def test_zero_u_keeps_the_atom(dt):
    """K = 1, Y = 0 and exactly representable products: u = 0, d is kept bit for bit, g' = 0."""
    dt = np.dtype(dt)
    d = np.full((1, 4), 0.5, dtype=dt)
    x = np.array([[1.0], [2.0], [0.0], [-3.0], [4.0]], dtype=dt)
    xg, Dg, md = _sweep(np.zeros((5, 4), dtype=dt), x, d)
    assert np.array_equal(Dg, d) and md == 0.0
    assert np.all(xg == 0)


@pytest.mark.parametrize('dt', DTYPES)
def test_row_beyond_row_nnz_max_is_refused_untouched(dt):
    y, x, D = _hand_built(81, 200, 24, [None] * 5, np.dtype(dt).kind == 'c', fill=0.2)
    x = x.copy()
    x[np.count_nonzero(x, axis=1) > 3, 3:] = 0     # every other row: at most 3
    x[131, :] = 0
    x[131, :4] = 1.5                               # one row with 4 non-zeros
    worst = int(np.count_nonzero(x, axis=1).max())
    assert worst == 4
    xg, Dg, msg = _sweep(y.astype(dt), x.astype(dt), D.astype(dt), row_nnz_max=3, expect_rc=ERR_INVALID)
    assert np.array_equal(xg, x.astype(dt)) and np.array_equal(Dg, D.astype(dt))
    assert 'row_nnz_max' in msg
    for bad in (0, 6, -1):
        _sweep(y.astype(dt), x.astype(dt), D.astype(dt), row_nnz_max=bad, expect_rc=ERR_INVALID)
    _check_hand_built(dt, y, x, D, 'row_nnz_max = K')
    xa, Da, _ = _sweep(y.astype(dt), x.astype(dt), D.astype(dt), row_nnz_max=4)      # exactly at the bound
    xb, Db, _ = _sweep(y.astype(dt), x.astype(dt), D.astype(dt), row_nnz_max=5)
    assert np.array_equal(xa, xb) and np.array_equal(Da, Db)


def test_row_longer_than_the_lds_slice():
    """complex128 rows of just over kKsvdLdsBytes: pass 2 reads the row twice instead of keeping it in LDS."""
    F = LDS_BYTES // 16 + 3
    y, x, D = _hand_built(91, 40, F, [7, 0, None], True, fill=0.3)
    _check_hand_built('complex128', y, x, D, 'F = %d' % F)


# ---- 4: composition and reproducibility, bitwise ------------------------------------------------------------------
@pytest.mark.parametrize('dt', DTYPES)
@pytest.mark.parametrize('coef_tol', [None, 'median'])
def test_step_is_omp_then_sweep(dt, coef_tol):
    from decomp_amd import omp
    dt = np.dtype(dt)
    case = _cases_for(dt)[0]
    S = ksvd_ref.CASES[case][4]
    y, _, D0 = ksvd_ref.case_problem(case)
    y, D = y.astype(dt), _normalised_on_gpu(D0.astype(dt))
    tol = None if coef_tol is None else 0.15 * float(np.median(np.sum(np.abs(y) ** 2, axis=1)))
    it_o, x_o = omp.solve(y, D, n_nonzero_coefs=S, tol=tol)
    xs, Ds, md_s = _sweep(y, x_o, D, row_nnz_max=S)
    xt, Dt, md_t, it_t = _step(y, D, S, coef_tol=-1.0 if tol is None else tol)
    assert it_t == it_o
    assert np.array_equal(xs, xt) and np.array_equal(Ds, Dt) and md_s == md_t
    xt2, Dt2, md_t2, it_t2 = _step(y, D, S, coef_tol=-1.0 if tol is None else tol)
    assert np.array_equal(xt, xt2) and np.array_equal(Dt, Dt2) and md_t == md_t2 and it_t == it_t2
    if tol is not None:
        assert len(set(np.count_nonzero(x_o, axis=1).tolist())) >= 2       # rows stopped at different steps


@pytest.mark.parametrize('dt', DTYPES)
def test_solve_is_the_loop_over_the_step(dt):
    from decomp_amd import dictionary_learning, ksvd
    dt = np.dtype(dt)
    case = _cases_for(dt)[0]
    S = ksvd_ref.CASES[case][4]
    y, _, D0 = ksvd_ref.case_problem(case)
    y, D0 = y.astype(dt), D0.astype(dt)
    D = _normalised_on_gpu(D0)
    states, mds = [], []
    for _ in range(5):
        x, D, md, _ = _step(y, D, S)
        states.append((D, x))
        mds.append(md)
    print('maxdiff per iteration', mds)
    # maxiter exhausted
    it, Dm, xm = ksvd.solve(y, D0, S, tol=0.0, maxiter=6)
    assert isinstance(Dm, np.ndarray) and isinstance(xm, np.ndarray)
    assert it == 6 and np.array_equal(Dm, states[4][0]) and np.array_equal(xm, states[4][1])
    it, Dm, xm = ksvd.solve(y, D0, S, tol=0.0, maxiter=3)
    assert it == 3 and np.array_equal(Dm, states[1][0]) and np.array_equal(xm, states[1][1])
    # the stop rule: tol between two consecutive maxdiff values, the later one below every earlier one
    j = max(i for i in range(1, 5) if mds[i] < min(mds[:i]))
    tol = 0.5 * (mds[j] + min(mds[:j]))
    it, Ds, xs = ksvd.solve(y, D0, S, tol=tol, maxiter=1000)
    assert it == j + 1 and np.array_equal(Ds, states[j][0]) and np.array_equal(xs, states[j][1])
    # two runs, and the dictionary_learning front end
    it2, Ds2, xs2 = ksvd.solve(y, D0, S, tol=tol, maxiter=1000)
    assert it2 == it and np.array_equal(Ds2, Ds) and np.array_equal(xs2, xs)
    it3, Ds3, xs3 = dictionary_learning.solve(y, D0, 0, tol=tol, minibatch=None, maxiter=1000, method='ksvd',
                                              lasso_method='omp', lasso_iter=S, lasso_tol=None)
    assert it3 == it and np.array_equal(Ds3, Ds) and np.array_equal(xs3, xs)
    ctol = 0.15 * float(np.median(np.sum(np.abs(y) ** 2, axis=1)))
    a = ksvd.solve(y, D0, S, tol=0.0, maxiter=3, coef_tol=ctol)
    b = dictionary_learning.solve(y, D0, 0.0, tol=0.0, maxiter=3, method='ksvd', lasso_method='omp', lasso_iter=S,
                                  lasso_tol=ctol)
    assert a[0] == b[0] == 3 and np.array_equal(a[1], b[1]) and np.array_equal(a[2], b[2])
    assert not np.array_equal(a[2], states[1][1])                       # the residual stop took effect


def test_torch_tensors_stay_on_the_device():
    import torch
    from decomp_amd import ksvd
    y, _, D0 = ksvd_ref.case_problem(1)
    yt, Dt = torch.from_numpy(y.astype(np.float32)).cuda(), torch.from_numpy(D0.astype(np.float32)).cuda()
    D_in = Dt.clone()
    it, D, x = ksvd.solve(yt, Dt, 3, tol=0.0, maxiter=3)
    assert it == 3 and D.is_cuda and x.is_cuda and torch.equal(Dt, D_in)        # the caller's D is not written
    itn, Dn, xn = ksvd.solve(y.astype(np.float32), D0.astype(np.float32), 3, tol=0.0, maxiter=3)
    assert np.array_equal(D.cpu().numpy(), Dn) and np.array_equal(x.cpu().numpy(), xn)
    it, D1, x1 = ksvd.solve(yt, Dt, 3, maxiter=1)                                # no iteration: D normalised, x = 0
    assert it == 1 and not bool(x1.any())


# ---- 5: end to end against the reference loop -------------------------------------------------------------------
@pytest.mark.parametrize('case', sorted(ksvd_ref.CASES))
@pytest.mark.parametrize('precision', ['single', 'double'])
def test_end_to_end(case, precision):
    """ITERATIONS iterations from the perturbed start.

    The objective: <= the double reference loop's x (1 + m), m = 4 x the relative gap of the NumPy loop in the
    working dtype to the double loop, floor 1e-3.  Recovery: per planted atom, the best |<a, d>| >= the double
    reference's - m.  D and X (bounds: 4 x the NumPy working-dtype loop against the double loop, floor 64 eps): over
    all iterations when every row's margin in the double reference stays >= DELTA[precision] throughout, else after
    the first iteration alone when that one's margins allow it, else not at all."""
    from decomp_amd import ksvd
    seed, N, F, K, S, cplx = ksvd_ref.CASES[case]
    dt = omp_ref.precision_dtype(cplx, precision)
    eps = float(np.finfo(dt).eps)
    y, A, D0 = ksvd_ref.case_problem(case)
    n = ksvd_ref.ITERATIONS
    ref = ksvd_ref.loop_reference(case, 'double')
    work = ksvd_ref.loop_reference(case, precision)
    obj_ref = ksvd_ref.objective(y, ref[-1][1], ref[-1][0])
    obj_work = ksvd_ref.objective(y, work[-1][1], work[-1][0])
    m = max(4 * abs(obj_work - obj_ref) / obj_ref, 1e-3)
    it, D, x = ksvd.solve(y.astype(dt), D0.astype(dt), S, tol=0.0, maxiter=n + 1)
    assert it == n + 1 and D.dtype == dt and x.dtype == dt
    obj = ksvd_ref.objective(y, x, D)
    rec, rec_ref = ksvd_ref.recovery(A, D), ksvd_ref.recovery(A, ref[-1][0])
    margins = [mg for _, _, _, mg in ref]
    print('case %d %s: objective %.6g (reference %.6g, NumPy %s loop %.6g, start %.6g), m %.3g; recovery min %.6f '
          '(reference %.6f), worst shortfall %.3g; margins %s'
          % (case, np.dtype(dt).name, obj, obj_ref, precision, obj_work, ksvd_ref.objective(y, ref[0][1], ref[0][0]),
             m, rec.min(), rec_ref.min(), float(np.max(rec_ref - rec)), ['%.2g' % v for v in margins]))
    assert np.all(np.isfinite(D)) and np.all(np.isfinite(x))
    assert np.all(np.count_nonzero(x, axis=1) <= S)
    assert np.allclose(np.linalg.norm(D[np.any(x != 0, axis=0)].astype(y.dtype), axis=1), 1.0, atol=64 * eps)
    assert obj <= obj_ref * (1 + m)
    assert np.all(rec >= rec_ref - m)

    delta = omp_ref.DELTA[precision]
    if min(margins) >= delta:
        upto, got = n, (D, x)
    elif margins[0] >= delta:
        upto = 1
        got = ksvd.solve(y.astype(dt), D0.astype(dt), S, tol=0.0, maxiter=2)[1:]
        print('  a margin below %.0e after the first iteration: D and X are compared after iteration 1 only' % delta)
    else:
        print('  a margin below %.0e in the first iteration: D and X are not compared' % delta)
        return
    Dr, xr = ref[upto - 1][0], ref[upto - 1][1]
    Dw, xw = work[upto - 1][0], work[upto - 1][1]
    xmax = float(np.max(np.abs(xr)))
    b_d = max(4 * float(np.max(np.abs(Dw - Dr))), 64 * eps)
    b_x = max(4 * float(np.max(np.abs(xw - xr))) / xmax, 64 * eps)
    err_d = float(np.max(np.abs(got[0] - Dr)))
    err_x = float(np.max(np.abs(got[1] - xr))) / xmax
    print('  after %d iteration(s): D error %.3g (bound %.3g); x error %.3g (bound %.3g)'
          % (upto, err_d, b_d, err_x, b_x))
    assert np.array_equal(got[1] != 0, xr != 0)
    assert err_d <= b_d
    assert err_x <= b_x
