"""GPU: masked approximate K-SVD (decomp_amd.ksvd.solve(mask=...), dcp_ksvd_mask_sweep_*, dcp_ksvd_mask_step_*)
against the NumPy reference of ksvd_mask_ref.py.

The sweep has no discrete decision, so it is compared value by value, in all four dtypes, against the double sweep on
the same single-exact inputs.  The bounds are not fixed in advance: 4 x the error the NumPy sweep in the working dtype
shows against double (the factor covers the other summation order of the chunked reduction), floor 64 eps; D relative
to 1, X relative to max|x_ref| (ksvd_mask_ref.bounds_against).  The loop contains the greedy coder, so end to end the
weighted OBJECTIVE is compared; D and X only over iterations in which every row's margin in the double reference stays
above omp_ref.DELTA."""
import ctypes
import os
import re

import numpy as np
import pytest

import ksvd_mask_ref as mr
import ksvd_ref
import omp_ref

pytestmark = pytest.mark.gpu

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
DTYPES = ['float32', 'float64', 'complex64', 'complex128']
ERR_INVALID = -1


def _constant(name):
    text = open(os.path.join(ROOT, 'decomp_amd', 'csrc', 'ksvd.hpp')).read()
    return int(re.search(r'constexpr int %s = (\d+);' % name, text).group(1))


C = _constant('kKsvdChunk')              # support rows per pass-1 partial
LDS_BYTES = _constant('kKsvdLdsBytes')   # a pass-2 row longer than this is read twice instead of kept in LDS


def _precision(dt):
    dt = np.dtype(dt)
    return 'single' if dt.itemsize == (8 if dt.kind == 'c' else 4) else 'double'


def _real(dt):
    return np.zeros(1, dtype=dt).real.dtype


def _sweep(y, m, x, D, row_nnz_max=None, expect_rc=0, mask_ndim=None, null_mask=False, mask_offset=0):
    """dcp_ksvd_mask_sweep_* on host arrays (y, x, D of one dtype, m cast to its real dtype): (x, D, maxdiff).
    mask_offset: the mask starts that many elements into its allocation."""
    import torch
    from decomp_amd import _arrays, _hip
    yt = torch.from_numpy(np.ascontiguousarray(y)).cuda()
    mt = torch.from_numpy(np.ascontiguousarray(np.asarray(m).astype(_real(y.dtype)))).cuda()
    if mask_offset:
        whole = torch.zeros(mt.numel() + mask_offset, dtype=mt.dtype, device=mt.device)
        whole[mask_offset:] = mt.reshape(-1)
        mt = whole[mask_offset:].view(mt.shape)
        assert mt.is_contiguous() and mt.data_ptr() == whole.data_ptr() + mask_offset * mt.element_size()
    xt = torch.from_numpy(np.ascontiguousarray(x)).cuda()
    Dt = torch.from_numpy(np.ascontiguousarray(D)).cuda()
    N, F = y.shape
    K = D.shape[0]
    lib, h = _arrays.lib_handle(yt)
    md = ctypes.c_double(-1.0)
    name = 'dcp_ksvd_mask_sweep_' + _arrays.suffix(yt)
    rc = getattr(lib, name)(h, _arrays.ptr(yt), _arrays.ptr(None if null_mask else mt),
                            mt.dim() if mask_ndim is None else mask_ndim, _arrays.ptr(xt), _arrays.ptr(Dt), N, F, K,
                            K if row_nnz_max is None else row_nnz_max, ctypes.byref(md))
    if expect_rc != 0:
        assert rc == expect_rc, rc
        return xt.cpu().numpy(), Dt.cpu().numpy(), lib.dcp_last_error_string(h).decode()
    _hip.check(h, rc, name)
    return xt.cpu().numpy(), Dt.cpu().numpy(), md.value


def _unmasked_sweep(y, x, D, row_nnz_max):
    import torch
    from decomp_amd import _arrays, _hip
    yt, xt, Dt = (torch.from_numpy(np.ascontiguousarray(a)).cuda() for a in (y, x, D))
    lib, h = _arrays.lib_handle(yt)
    md = ctypes.c_double(-1.0)
    name = 'dcp_ksvd_sweep_' + _arrays.suffix(yt)
    _hip.check(h, getattr(lib, name)(h, _arrays.ptr(yt), _arrays.ptr(xt), _arrays.ptr(Dt), y.shape[0], y.shape[1],
                                     D.shape[0], row_nnz_max, ctypes.byref(md)), name)
    return xt.cpu().numpy(), Dt.cpu().numpy(), md.value


def _step(y, m, D, s, coef_tol=-1.0, rows_per_pass=0):
    """dcp_ksvd_mask_step_* on host arrays: (x, D, maxdiff, it).  x starts as NaN: the coder writes all of it."""
    import torch
    from decomp_amd import _arrays, _hip
    yt = torch.from_numpy(np.ascontiguousarray(y)).cuda()
    mt = torch.from_numpy(np.ascontiguousarray(np.asarray(m).astype(_real(y.dtype)))).cuda()
    Dt = torch.from_numpy(np.ascontiguousarray(D)).cuda()
    N, F = y.shape
    K = D.shape[0]
    xt = torch.full((N, K), float('nan'), dtype=yt.dtype, device=yt.device)
    lib, h = _arrays.lib_handle(yt)
    md, it = ctypes.c_double(-1.0), ctypes.c_int(-1)
    name = 'dcp_ksvd_mask_step_' + _arrays.suffix(yt)
    rc = getattr(lib, name)(h, _arrays.ptr(yt), _arrays.ptr(mt), mt.dim(), _arrays.ptr(xt), _arrays.ptr(Dt), N, F, K,
                            int(s), float(coef_tol), int(rows_per_pass), ctypes.byref(md), ctypes.byref(it))
    _hip.check(h, rc, name)
    return xt.cpu().numpy(), Dt.cpu().numpy(), md.value, it.value


def _omp_mask(y, m, A, s, rows_per_pass=0):
    """dcp_omp_mask_* on host arrays: x."""
    import torch
    from decomp_amd import _arrays, _hip
    yt = torch.from_numpy(np.ascontiguousarray(y)).cuda()
    mt = torch.from_numpy(np.ascontiguousarray(np.asarray(m).astype(_real(y.dtype)))).cuda()
    At = torch.from_numpy(np.ascontiguousarray(A)).cuda()
    xt = torch.full((y.shape[0], A.shape[0]), float('nan'), dtype=yt.dtype, device=yt.device)
    lib, h = _arrays.lib_handle(yt)
    it = ctypes.c_int(-1)
    name = 'dcp_omp_mask_' + _arrays.suffix(yt)
    _hip.check(h, getattr(lib, name)(h, _arrays.ptr(yt), _arrays.ptr(mt), mt.dim(), _arrays.ptr(At), _arrays.ptr(xt),
                                     y.shape[0], y.shape[1], A.shape[0], int(s), -1.0, int(rows_per_pass),
                                     ctypes.byref(it)), name)
    return xt.cpu().numpy()


def _normalised_on_gpu(D):
    import torch
    from decomp_amd import _arrays
    Dt = torch.from_numpy(np.ascontiguousarray(D)).cuda()
    return _arrays.l2_normalize_(Dt, strict=True).cpu().numpy()


def _cases_for(dt):
    return [c for c in sorted(mr.CASES) if mr.CASES[c][5] == (np.dtype(dt).kind == 'c')]


# ---- 1: the sweep against the double reference, and monotone -------------------------------------------------------
SWEEP_PARAMS = [(dt, c, kind, st) for dt in DTYPES for c in _cases_for(dt) for kind in mr.KINDS
                for st in ('planted', 'random')]


@pytest.mark.parametrize('dt,case,kind,start', SWEEP_PARAMS)
def test_sweep_parity_and_monotone(dt, case, kind, start):
    dt = np.dtype(dt)
    prec = _precision(dt)
    y, x, D, m = mr.sweep_inputs(case, kind, start)
    S = mr.CASES[case][4]
    xr, Dr = mr.sweep_reference(case, kind, start, 'double')
    b_d, b_x, b_r = mr.sweep_bounds(case, kind, start, prec)
    xg, Dg, md = _sweep(y.astype(dt), m, x.astype(dt), D.astype(dt), row_nnz_max=S)
    assert xg.dtype == dt and Dg.dtype == dt
    err_d = float(np.max(np.abs(Dg - Dr)))
    err_x = float(np.max(np.abs(xg - xr))) / float(np.max(np.abs(xr)))
    r_before, r_ref, r_gpu = mr.rel_resid(y, x, D, m), mr.rel_resid(y, xr, Dr, m), mr.rel_resid(y, xg, Dg, m)
    md_ref = float(np.max(np.abs(Dr - D)))
    print('case %d %s %s %s: D error %.3g (bound %.3g); x error %.3g (bound %.3g); weighted |y - xD|/|y| %.6g -> %.6g '
          '(reference %.6g, difference %.3g, bound %.3g); maxdiff %.6g (reference %.6g)'
          % (case, kind, start, dt.name, err_d, b_d, err_x, b_x, r_before, r_gpu, r_ref, abs(r_gpu - r_ref), b_r, md,
             md_ref))
    assert np.all(np.isfinite(xg)) and np.all(np.isfinite(Dg))
    assert np.all((xg != 0) <= (x != 0))
    assert err_d <= b_d
    assert err_x <= b_x
    assert abs(r_gpu - r_ref) <= b_r                     # the maintained residual, through the objective on the host
    assert r_gpu < r_before                              # the weighted objective strictly decreases
    assert abs(md - md_ref) <= b_d
    assert abs(md - float(np.max(np.abs(Dg - D.astype(dt))))) <= 4 * float(np.finfo(dt).eps)


# ---- 2: shapes where the kernels can go wrong -----------------------------------------------------------------------
def _random(rng, cplx, *shape):
    return rng.randn(*shape) + 1j * rng.randn(*shape) if cplx else rng.randn(*shape)


def _hand_built(seed, N, F, sizes, cplx, fill=0.1):
    """y [N, F], D [K, F] random, x [N, K] with column q holding sizes[q] non-zeros (None: about fill * N) in random
    rows, m [N, F] weights in [0.25, 1) with 30 % zeros; all single-exact, in double."""
    rng = np.random.RandomState(seed)
    K = len(sizes)
    y, D = omp_ref.single_exact(_random(rng, cplx, N, F), ksvd_ref.normalise(_random(rng, cplx, K, F)))
    x = np.zeros((N, K), dtype=y.dtype)
    for q, sz in enumerate(sizes):
        n = int(rng.binomial(N, fill)) if sz is None else min(sz, N)
        rows = rng.choice(N, n, replace=False)
        x[rows, q] = (1 + rng.rand(n)) * rng.choice([-1, 1], n) * (np.exp(2j * np.pi * rng.rand(n)) if cplx else 1)
    x = omp_ref.single_exact(x, x)[0]
    m = np.where(rng.rand(N, F) < mr.KEEP, 0.25 + 0.75 * rng.rand(N, F), 0).astype(np.float32).astype(np.float64)
    return y, x, D, m


def _check_hand_built(dt, y, x, D, m, tag, **kw):
    dt = np.dtype(dt)
    eps = float(np.finfo(dt).eps)
    xr, Dr, _ = mr.sweep(y, x, D, m)
    xw, Dw, _ = mr.sweep(y.astype(dt), x.astype(dt), D.astype(dt), m)
    b_d, b_x, b_r = mr.bounds_against(y, m, xr, Dr, xw, Dw, eps)
    xg, Dg, md = _sweep(y.astype(dt), m, x.astype(dt), D.astype(dt), **kw)
    xmax = max(float(np.max(np.abs(xr))), 1e-300)
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


SUPPORTS = [1, C - 1, C, C + 1, 2 * C + 1]
# 37: the scalar path, and float32 mask rows that do not start on 16 bytes; 64: the vector path in every dtype;
# 257: two finish tiles, the second with one column (scalar path)
ROW_LENGTHS = [37, 64, 257]


@pytest.mark.parametrize('dt', DTYPES)
@pytest.mark.parametrize('F', ROW_LENGTHS)
def test_support_sizes_row_lengths_and_degenerate_masks(dt, F):
    """N = 300, K = 7: supports of 1, C - 1, C, C + 1 and 2 C + 1 rows, an unused atom and a sparse one.  Column 3 is
    hidden in every support row of atom 2 (u_3 = d_3), one support row of atom 3 is hidden entirely (g' = 0)."""
    cplx = np.dtype(dt).kind == 'c'
    y, x, D, m = _hand_built(140 + F, 300, F, SUPPORTS + [0, None], cplx)
    assert [int(np.count_nonzero(x[:, k])) for k in range(6)] == SUPPORTS + [0]
    m[np.flatnonzero(x[:, 2]), 3] = 0.0
    hidden_row = int(np.flatnonzero(x[:, 3])[5])
    m[hidden_row, :] = 0.0
    xg, Dg = _check_hand_built(dt, y, x, D, m, 'F = %d' % F)
    assert np.all(xg[hidden_row] == 0)


def test_row_longer_than_the_lds_slice():
    """complex128 rows of F 16 > kKsvdLdsBytes bytes: pass 2 reads the row a second time instead of keeping it."""
    F = 4100
    assert F * 16 > LDS_BYTES
    y, x, D, m = _hand_built(191, 40, F, [7, 0, None], True, fill=0.3)
    _check_hand_built('complex128', y, x, D, m, 'F = %d' % F)


@pytest.mark.parametrize('dt', DTYPES)
def test_one_row_and_one_atom(dt):
    cplx = np.dtype(dt).kind == 'c'
    y, x, D, m = _hand_built(171, 1, 20, [1, 0, 1], cplx)
    m[0, 0] = 0.5
    _check_hand_built(dt, y, x, D, m, 'N = 1')
    y, x, D, m = _hand_built(173, 1, 1, [1], cplx)
    _check_hand_built(dt, y, x, D, np.ones((1, 1)), 'N = F = K = 1')


@pytest.mark.parametrize('ndim', [1, 2])
def test_mask_base_pointer_off_16_bytes(ndim):
    """float64, F = 64: the row length allows the 16-byte path, but the mask starts 8 bytes off a 16-byte boundary,
    so its two reals per access are not aligned and the sweep takes the scalar path."""
    y, x, D, m = _hand_built(197, 300, 64, [C + 1, 0, None, 1], False)
    if ndim == 1:
        m = m[0].copy()
    _check_hand_built('float64', y, x, D, m, 'mask off 16 bytes, mask_ndim %d' % ndim, mask_offset=1)


# ---- 3: identities ----------------------------------------------------------------------------------------------
@pytest.mark.parametrize('dt', DTYPES)
def test_all_ones_mask_is_the_unmasked_sweep_within_the_bounds(dt):
    """Not bitwise: the division by c reorders the rounding."""
    dt = np.dtype(dt)
    case = _cases_for(dt)[0]
    S = mr.CASES[case][4]
    y, x, D = ksvd_ref.sweep_inputs(case, 'planted')
    b_d, b_x, _ = ksvd_ref.sweep_bounds(case, 'planted', _precision(dt))
    xr, Dr = ksvd_ref.sweep_reference(case, 'planted', 'double')
    xu, Du, mdu = _unmasked_sweep(y.astype(dt), x.astype(dt), D.astype(dt), S)
    for ones in (np.ones(y.shape), np.ones(y.shape[1])):
        xg, Dg, md = _sweep(y.astype(dt), ones, x.astype(dt), D.astype(dt), row_nnz_max=S)
        xmax = float(np.max(np.abs(xr)))
        print('%s mask_ndim %d: against the unmasked sweep D %.3g, x %.3g; against the double reference D %.3g '
              '(bound %.3g), x %.3g (bound %.3g)'
              % (dt.name, ones.ndim, np.max(np.abs(Dg - Du)), np.max(np.abs(xg - xu)) / xmax,
                 np.max(np.abs(Dg - Dr)), b_d, np.max(np.abs(xg - xr)) / xmax, b_x))
        assert float(np.max(np.abs(Dg - Dr))) <= b_d and float(np.max(np.abs(xg - xr))) / xmax <= b_x
        assert float(np.max(np.abs(Dg - Du))) <= b_d and float(np.max(np.abs(xg - xu))) / xmax <= b_x
        assert abs(md - mdu) <= b_d


@pytest.mark.parametrize('dt', DTYPES)
@pytest.mark.parametrize('F', [37, 64])
def test_one_dimensional_mask_is_its_broadcast_and_runs_repeat(dt, F):
    dt = np.dtype(dt)
    y, x, D, m = _hand_built(240 + F, 300, F, [C + 1, None, None, 0, None, 1], dt.kind == 'c')
    m1 = m[0].copy()
    y, x, D = y.astype(dt), x.astype(dt), D.astype(dt)
    a = _sweep(y, m1, x, D)
    b = _sweep(y, np.ascontiguousarray(np.broadcast_to(m1, y.shape)), x, D)
    assert np.array_equal(a[0], b[0]) and np.array_equal(a[1], b[1]) and a[2] == b[2]
    c = _sweep(y, m, x, D)
    d = _sweep(y, m, x, D)
    assert np.array_equal(c[0], d[0]) and np.array_equal(c[1], d[1]) and c[2] == d[2]
    assert not np.array_equal(a[1], c[1])


@pytest.mark.parametrize('dt', DTYPES)
def test_y_at_hidden_entries_does_not_influence_the_result(dt):
    dt = np.dtype(dt)
    case = _cases_for(dt)[0]
    S = mr.CASES[case][4]
    y, x, D, m = mr.sweep_inputs(case, 'weights', 'planted')
    rng = np.random.RandomState(17)
    y2 = np.where(m > 0, y, y + 100.0 * rng.randn(*y.shape))
    a = _sweep(y.astype(dt), m, x.astype(dt), D.astype(dt), row_nnz_max=S)
    b = _sweep(y2.astype(dt), m, x.astype(dt), D.astype(dt), row_nnz_max=S)
    assert np.array_equal(a[0], b[0]) and np.array_equal(a[1], b[1]) and a[2] == b[2]
    # and through the coder
    Dn = _normalised_on_gpu(D.astype(dt))
    a = _step(y.astype(dt), m, Dn, S)
    b = _step(y2.astype(dt), m, Dn, S)
    assert np.array_equal(a[0], b[0]) and np.array_equal(a[1], b[1]) and a[2:] == b[2:]


# ---- 4: the step entry ------------------------------------------------------------------------------------------
STEP_PARAMS = [(dt, c, kind) for dt in ('float64', 'complex128') for c in _cases_for(dt) for kind in mr.KINDS]


def _check_step(dt, y, D0, m, S, ref_x, ref_D, ref_md, ref_steps, margin, tag, rows_per_pass=0):
    """A step in double precision from the normalised D0 against the reference iteration (ref_*).  The bounds: 4 x
    what the NumPy iteration in the working dtype shows against double, floor 64 eps.  The working dtype is double, so
    the NumPy iteration is the reference itself and the bounds are the floor."""
    assert _precision(dt) == 'double'
    b_d = b_x = 64 * float(np.finfo(dt).eps)
    xg, Dg, md, it = _step(y.astype(dt), m, _normalised_on_gpu(D0.astype(dt)), S, rows_per_pass=rows_per_pass)
    xmax = float(np.max(np.abs(ref_x)))
    err_d, err_x = float(np.max(np.abs(Dg - ref_D))), float(np.max(np.abs(xg - ref_x))) / xmax
    print('%s: smallest margin %.3g; D error %.3g (bound %.3g); x error %.3g (bound %.3g); it %d (reference %d)'
          % (tag, margin, err_d, b_d, err_x, b_x, it, ref_steps))
    assert margin >= omp_ref.DELTA['double']                # every row is compared
    assert it == ref_steps
    assert np.array_equal(xg != 0, ref_x != 0)
    assert err_d <= b_d and err_x <= b_x
    assert abs(md - ref_md) <= b_d
    return xg, Dg, md, it


@pytest.mark.parametrize('dt,case,kind', STEP_PARAMS)
def test_step_is_the_reference_iteration(dt, case, kind):
    dt = np.dtype(dt)
    S = mr.CASES[case][4]
    y, _, D0 = ksvd_ref.case_problem(case)
    m = mr.case_mask(case, kind)
    Dr, xr, md_ref, margin, steps = mr.loop_reference(case, kind, 'double')[0]
    got = _check_step(dt, y, D0, m, S, xr, Dr, md_ref, steps, margin, 'case %d %s %s' % (case, kind, dt.name))
    # the composition: the masked coder, then the sweep entry; two runs
    yd, Dn = y.astype(dt), _normalised_on_gpu(D0.astype(dt))
    from decomp_amd import omp
    it_o, x_o = omp.solve(yd, Dn, n_nonzero_coefs=S, mask=m)
    xs, Ds, md_s = _sweep(yd, m, x_o, Dn, row_nnz_max=S)
    assert it_o == got[3] and np.array_equal(xs, got[0]) and np.array_equal(Ds, got[1]) and md_s == got[2]
    one = _step(yd, m, Dn, S, rows_per_pass=y.shape[0])
    assert np.array_equal(got[0], one[0]) and np.array_equal(got[1], one[1]) and got[2:] == one[2:]
    # passes of 100 rows against one pass: bitwise.  The coder (unchanged) promises that only while the products of
    # every pass take the same GEMM tile.  Case 1 has 509 rows: the last pass has 9, and a 9 x 40 float64 product runs
    # on the generic core, not on the matrix core as the 509 x 40 one; measured on an MI355X, dcp_omp_mask_f64 itself
    # then differs by one unit in the last place (4.4e-16) in rows 500 .. 508 and in no other row.  There the rows
    # of the full passes are compared bitwise and the whole result within the bounds of the step.
    p = _step(yd, m, Dn, S, rows_per_pass=100)
    x_p = _omp_mask(yd, m, Dn, S, rows_per_pass=100)
    full = y.shape[0] // 100 * 100
    assert np.array_equal(x_p[:full], x_o[:full])
    coder_is_pass_invariant = np.array_equal(x_p, x_o)
    assert coder_is_pass_invariant or (case == 1 and dt == np.float64), 'the coder depends on rows_per_pass'
    xs_p, Ds_p, md_p = _sweep(yd, m, x_p, Dn, row_nnz_max=S)
    assert np.array_equal(xs_p, p[0]) and np.array_equal(Ds_p, p[1]) and md_p == p[2] and p[3] == got[3]
    if coder_is_pass_invariant:
        assert np.array_equal(got[0], p[0]) and np.array_equal(got[1], p[1]) and got[2:] == p[2:]
    else:
        print('  rows_per_pass = 100: the coder differs in rows %s by %.3g; the step by D %.3g, x %.3g'
              % (np.flatnonzero(np.any(x_p != x_o, axis=1)), np.max(np.abs(x_p - x_o)),
                 np.max(np.abs(p[1] - got[1])), np.max(np.abs(p[0] - got[0]))))
        _check_step(dt, y, D0, m, S, xr, Dr, md_ref, steps, margin, 'in passes of 100', rows_per_pass=100)


@pytest.mark.parametrize('dt', ['float64', 'complex128'])
def test_step_with_a_one_dimensional_mask(dt):
    """mask_ndim = 1: the coder in Gram form on sqrt(m) y, sqrt(m) D, the sweep with a mask row stride of 0."""
    dt = np.dtype(dt)
    case = _cases_for(dt)[0]
    S = mr.CASES[case][4]
    y, _, D0 = ksvd_ref.case_problem(case)
    m1 = mr.case_mask(case, 'weights')[0].copy()
    assert np.count_nonzero(m1 == 0) >= 3
    log = []
    mr.solve(y, D0, m1, S, tol=0.0, maxiter=2, log=log)
    Dr, xr, md_ref, margin, steps = log[0]
    got = _check_step(dt, y, D0, m1, S, xr, Dr, md_ref, steps, margin, 'case %d 1-D %s' % (case, dt.name))
    from decomp_amd import omp
    Dn = _normalised_on_gpu(D0.astype(dt))
    it_o, x_o = omp.solve(y.astype(dt), Dn, n_nonzero_coefs=S, mask=m1)
    xs, Ds, md_s = _sweep(y.astype(dt), m1, x_o, Dn, row_nnz_max=S)
    assert it_o == got[3] and np.array_equal(xs, got[0]) and np.array_equal(Ds, got[1]) and md_s == got[2]
    # the hidden channels of every used atom keep their direction: u_f = d_f there
    hidden = m1 == 0
    used = np.any(got[0] != 0, axis=0)
    ratio = got[1][used][:, hidden] / Dn[used][:, hidden]
    assert np.max(np.abs(ratio - ratio[:, :1])) <= 64 * float(np.finfo(dt).eps) * np.max(np.abs(ratio))


# ---- 5: end to end against the reference loop -------------------------------------------------------------------
@pytest.mark.parametrize('case', sorted(mr.CASES))
@pytest.mark.parametrize('precision', ['single', 'double'])
def test_end_to_end(case, precision):
    """ITERATIONS iterations from the perturbed start with the `weights` mask.

    The weighted objective: <= the double reference loop's x (1 + m), m = 4 x the relative gap of the NumPy loop in
    the working dtype to the double loop, floor 1e-3.  Recovery: per planted atom, the best |<a, d>| >= the double
    reference's - m.  D and X: over all iterations when every row's margin in the double reference stays >=
    DELTA[precision] throughout, else after the first iteration alone when that one's margins allow it, else not at
    all.  Their bounds: 4 x what the NumPy loop in the working dtype shows against the double loop, floor 64 eps (in
    double precision the NumPy loop is the reference itself, so the floor)."""
    from decomp_amd import ksvd
    seed, N, F, K, S, cplx = mr.CASES[case]
    dt = omp_ref.precision_dtype(cplx, precision)
    eps = float(np.finfo(dt).eps)
    y, A, D0 = ksvd_ref.case_problem(case)
    w = mr.case_mask(case, 'weights')
    n = mr.ITERATIONS
    ref = mr.loop_reference(case, 'weights', 'double')
    work = mr.loop_reference(case, 'weights', precision)
    obj_ref = mr.objective(y, ref[-1][1], ref[-1][0], w)
    obj_work = mr.objective(y, work[-1][1], work[-1][0], w)
    m = max(4 * abs(obj_work - obj_ref) / obj_ref, 1e-3)
    it, D, x = ksvd.solve(y.astype(dt), D0.astype(dt), S, tol=0.0, maxiter=n + 1, mask=w)
    assert it == n + 1 and D.dtype == dt and x.dtype == dt
    obj = mr.objective(y, x, D, w)
    rec, rec_ref = ksvd_ref.recovery(A, D), ksvd_ref.recovery(A, ref[-1][0])
    margins = [e[3] for e in ref]
    print('case %d %s: weighted objective %.6g (reference %.6g, NumPy %s loop %.6g, after iteration 1 %.6g), m %.3g; '
          'recovery min %.6f (reference %.6f), worst shortfall %.3g; margins %s'
          % (case, np.dtype(dt).name, obj, obj_ref, precision, obj_work, mr.objective(y, ref[0][1], ref[0][0], w),
             m, rec.min(), rec_ref.min(), float(np.max(rec_ref - rec)), ['%.2g' % v for v in margins]))
    assert np.all(np.isfinite(D)) and np.all(np.isfinite(x))
    assert np.all(np.count_nonzero(x, axis=1) <= S)
    norms = np.linalg.norm(D[np.any(x != 0, axis=0)].astype(y.dtype), axis=1)
    assert float(np.max(np.abs(norms - 1.0))) <= 64 * eps
    assert obj <= obj_ref * (1 + m)
    assert np.all(rec >= rec_ref - m)

    delta = omp_ref.DELTA[precision]
    if min(margins) >= delta:
        upto, got = n, (D, x)
        print('  every margin >= %.0e: D and X are compared after all %d iterations' % (delta, n))
    elif margins[0] >= delta:
        upto = 1
        got = ksvd.solve(y.astype(dt), D0.astype(dt), S, tol=0.0, maxiter=2, mask=w)[1:]
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


def test_solve_front_end():
    """torch CUDA inputs return torch; a 1-D mask; mask=None is the unmasked loop bit for bit; maxiter = 1; a row
    without observed samples gets x = 0 and x @ D fills the holes."""
    import torch
    from decomp_amd import _arrays, _hip, ksvd
    y, _, D0 = ksvd_ref.case_problem(1)
    w = mr.case_mask(1, 'weights').copy()
    w[11, :] = 0.0
    y32, D32, w32 = y.astype(np.float32), D0.astype(np.float32), w.astype(np.float32)
    yt, Dt, wt = (torch.from_numpy(a).cuda() for a in (y32, D32, w32))
    D_in = Dt.clone()
    it, D, x = ksvd.solve(yt, Dt, 3, tol=0.0, maxiter=3, mask=wt)
    assert it == 3 and D.is_cuda and x.is_cuda and torch.equal(Dt, D_in)        # the caller's D is not written
    itn, Dn, xn = ksvd.solve(y32, D32, 3, tol=0.0, maxiter=3, mask=w)           # a float64 mask is cast
    assert isinstance(Dn, np.ndarray) and isinstance(xn, np.ndarray)
    assert np.array_equal(D.cpu().numpy(), Dn) and np.array_equal(x.cpu().numpy(), xn)
    assert np.all(xn[11] == 0) and np.all(np.isfinite(xn @ Dn))
    # the holes (of rows that have observed samples) are filled as well as the double reference loop fills them
    hidden = (w == 0) & (np.arange(y.shape[0]) != 11)[:, None]
    _, Dref, xref = mr.solve(y, D0, w, 3, tol=0.0, maxiter=3)
    miss = np.linalg.norm((xn.astype(np.float64) @ Dn.astype(np.float64) - y)[hidden]) / np.linalg.norm(y[hidden])
    miss_ref = np.linalg.norm((xref @ Dref - y)[hidden]) / np.linalg.norm(y[hidden])
    print('relative error at the hidden entries %.4g (double reference %.4g)' % (miss, miss_ref))
    assert miss_ref < 0.5 and miss <= 1.1 * miss_ref
    # the two steps by hand
    Dh = _normalised_on_gpu(D32)
    for _ in range(2):
        xh, Dh, _, _ = _step(y32, w32, Dh, 3)
    assert np.array_equal(Dh, Dn) and np.array_equal(xh, xn)
    # a 1-D mask goes to the step entry as mask_ndim = 1 (its coder is the Gram form, so only the sweeps of a 1-D mask
    # and of its broadcast are bitwise equal, not the loops)
    m1 = w32[0].copy()
    a = ksvd.solve(y32, D32, 3, tol=0.0, maxiter=3, mask=m1)
    Dh = _normalised_on_gpu(D32)
    for _ in range(2):
        xh, Dh, _, _ = _step(y32, m1, Dh, 3)
    assert a[0] == 3 and np.array_equal(a[1], Dh) and np.array_equal(a[2], xh)
    assert np.all(np.count_nonzero(a[2], axis=1) <= 3)
    # maxiter = 1: no iteration
    it, D1, x1 = ksvd.solve(yt, Dt, 3, maxiter=1, mask=wt)
    assert it == 1 and not bool(x1.any())
    assert torch.equal(D1, _arrays.l2_normalize_(Dt.clone(), strict=True))
    # mask=None: the unmasked entry, as before
    u = ksvd.solve(y32, D32, 3, tol=0.0, maxiter=3, mask=None)
    v = ksvd.solve(y32, D32, 3, tol=0.0, maxiter=3)
    Dh = torch.from_numpy(_normalised_on_gpu(D32)).cuda()
    xh = torch.zeros((y32.shape[0], D32.shape[0]), dtype=torch.float32, device='cuda')
    lib, h = _arrays.lib_handle(yt)
    md, oit = ctypes.c_double(0), ctypes.c_int(0)
    for _ in range(2):
        _hip.check(h, lib.dcp_ksvd_step_f32(h, _arrays.ptr(yt), _arrays.ptr(xh), _arrays.ptr(Dh), y32.shape[0],
                                            y32.shape[1], D32.shape[0], 3, -1.0, ctypes.byref(md), ctypes.byref(oit)),
                   'dcp_ksvd_step_f32')
    for got in (u, v):
        assert got[0] == 3 and np.array_equal(got[1], Dh.cpu().numpy()) and np.array_equal(got[2], xh.cpu().numpy())
    assert not np.array_equal(u[1], Dn)


# ---- 6: ABI errors ----------------------------------------------------------------------------------------------
@pytest.mark.parametrize('dt', DTYPES)
def test_abi_errors_leave_x_and_d_untouched(dt):
    dt = np.dtype(dt)
    y, x, D, m = _hand_built(181, 200, 24, [None] * 5, dt.kind == 'c', fill=0.2)
    x = x.copy()
    x[np.count_nonzero(x, axis=1) > 3, 3:] = 0     # every other row: at most 3
    x[131, :] = 0
    x[131, :4] = 1.5                               # one row with 4 non-zeros
    assert int(np.count_nonzero(x, axis=1).max()) == 4
    y, x, D = y.astype(dt), x.astype(dt), D.astype(dt)

    def refused(what, **kw):
        xg, Dg, msg = _sweep(y, m, x, D, expect_rc=ERR_INVALID, **kw)
        assert np.array_equal(xg, x) and np.array_equal(Dg, D), what
        assert msg, what
        return msg
    assert 'row_nnz_max' in refused('a row beyond row_nnz_max', row_nnz_max=3)
    for bad in (0, 6, -1):
        assert 'row_nnz_max' in refused('row_nnz_max outside [1, K]', row_nnz_max=bad)
    for bad in (0, 3, -1):
        assert 'mask_ndim' in refused('mask_ndim', mask_ndim=bad)
    assert 'null' in refused('a null mask', null_mask=True)
    xa, Da, _ = _sweep(y, m, x, D, row_nnz_max=4)      # exactly at the bound
    xb, Db, _ = _sweep(y, m, x, D, row_nnz_max=5)
    assert np.array_equal(xa, xb) and np.array_equal(Da, Db) and not np.array_equal(Da, D)


def test_step_abi_errors():
    import torch
    from decomp_amd import _arrays
    y, x, D, m = _hand_built(182, 50, 24, [None] * 5, False)
    yt, Dt, mt = (torch.from_numpy(a.astype(np.float32)).cuda() for a in (y, D, m))
    xt = torch.zeros((50, 5), dtype=torch.float32, device='cuda')
    lib, h = _arrays.lib_handle(yt)
    md, it = ctypes.c_double(-1.0), ctypes.c_int(-1)

    def call(M=mt, ndim=2, s=3, tol=-1.0, rpp=0):
        rc = lib.dcp_ksvd_mask_step_f32(h, _arrays.ptr(yt), _arrays.ptr(M), ndim, _arrays.ptr(xt), _arrays.ptr(Dt), 50,
                                        24, 5, s, tol, rpp, ctypes.byref(md), ctypes.byref(it))
        return rc, lib.dcp_last_error_string(h).decode()
    D_in = Dt.clone()
    for kw, word in ((dict(ndim=0), 'mask_ndim'), (dict(ndim=3), 'mask_ndim'), (dict(M=None), 'null'),
                     (dict(s=0), 'n_nonzero'), (dict(s=6), 'n_nonzero'), (dict(s=65), 'n_nonzero'),
                     (dict(tol=float('nan')), 'NaN'), (dict(rpp=-1), 'rows_per_pass')):
        rc, msg = call(**kw)
        assert rc == ERR_INVALID and msg, kw
        print(kw, '->', msg)
        assert word.lower() in msg.lower() or kw.get('s') is not None, (kw, msg)
        assert torch.equal(Dt, D_in) and not bool(xt.any())
    rc, msg = call()
    assert rc == 0 and it.value == 3 and not torch.equal(Dt, D_in)
