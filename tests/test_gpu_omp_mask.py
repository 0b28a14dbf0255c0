"""GPU: decomp_amd.omp.solve(mask=...) and dcp_omp_mask_* against the NumPy references of omp_mask_ref.py --
supports, coefficients, per-row properties in the weighted inner product, the residual stop, the row passes, the
1-D route, the degenerate rows and the sizes at which the step kernel takes another path, in all four dtypes.

Rows whose reference selection margin is below delta (1e-4 single, 1e-8 double), and in tol runs rows whose
residual margin is below 1e-4, are left out of the SUPPORT comparison (at most 10 % per run, asserted; the shares
are computed on the CPU in test_omp_mask_ref_host.py); the properties are checked on every row.  The bounds are
4 x what the working-dtype restatement shows on the CPU against the double reference, floor 64 eps
(omp_mask_ref.Analysis.bounds)."""
import ctypes

import numpy as np
import pytest

import omp_mask_ref as mr
import omp_ref

pytestmark = pytest.mark.gpu

DTYPES = ['float32', 'float64', 'complex64', 'complex128']
TABLE = [(c, 'double', k, t) for c in mr.CASES for k in mr.KINDS for t in (False, True)] + \
        [(c, 'single', k, t) for c in sorted(mr.SINGLE_RUNS) for (k, t) in mr.SINGLE_RUNS[c]]
STEP_K = [64, 65, 130, 256, 257, 520]     # the lane stride (64) and the scoring chunk (256) of the step kernel


def _precision(dt):
    dt = np.dtype(dt)
    return 'single' if dt.itemsize == (8 if dt.kind == 'c' else 4) else 'double'


def _random(rng, cplx, *shape):
    return rng.randn(*shape) + 1j * rng.randn(*shape) if cplx else rng.randn(*shape)


def _abi(y, m, A, s, tol=-1.0, rows_per_pass=0, mask_ndim=None, expect_rc=0, null_mask=False):
    """dcp_omp_mask_* on host arrays: (it, x).  x starts as NaN: the library writes all of it."""
    import torch
    from decomp_amd import _arrays, _hip
    yt = torch.from_numpy(np.ascontiguousarray(y)).cuda()
    At = torch.from_numpy(np.ascontiguousarray(A)).cuda()
    mt = torch.from_numpy(np.ascontiguousarray(m).astype(y.real.dtype)).cuda()
    x = torch.full((y.shape[0], A.shape[0]), float('nan'), dtype=yt.dtype, device=yt.device)
    lib, h = _arrays.lib_handle(yt)
    it = ctypes.c_int(-1)
    name = 'dcp_omp_mask_' + _arrays.suffix(yt)
    rc = getattr(lib, name)(h, _arrays.ptr(yt), None if null_mask else _arrays.ptr(mt),
                            m.ndim if mask_ndim is None else mask_ndim, _arrays.ptr(At), _arrays.ptr(x), y.shape[0],
                            y.shape[1], A.shape[0], int(s), float(tol), int(rows_per_pass), ctypes.byref(it))
    if expect_rc != 0:
        assert rc == expect_rc, rc
        return lib.dcp_last_error_string(h).decode(), None
    _hip.check(h, rc, name)
    return it.value, x.cpu().numpy()


def _check_against(an, precision, it, x, tag):
    """Supports, coefficients, step counts and the per-row properties of a GPU result against an Analysis."""
    dt = an.dtype(precision)
    assert x.dtype == dt and x.shape == an.x.shape
    keep = an.keep(precision)
    left_out = an.left_out(precision)
    b_coef, b_orth, b_res = an.bounds(precision)
    nnz = np.count_nonzero(x, axis=1)
    xd = x.astype(an.x.dtype)
    err = float(np.max(np.abs(xd - an.x)[keep], initial=0.0)) / float(np.max(np.abs(an.x)))
    res, orth = mr.row_metrics(x, an.y, an.A, an.m)
    res_ref, _ = mr.row_metrics(an.x, an.y, an.A, an.m)
    same = np.array_equal((x != 0)[keep], (an.x != 0)[keep])
    print('%s %s: left out %.2f %%; coefficient error %.3g (bound %.3g); orthogonality %.3g (bound %.3g); '
          'residual excess %.3g (bound %.3g); steps %s; it %d'
          % (tag, np.dtype(dt).name, 100 * left_out, err, b_coef, float(orth.max()), b_orth,
             float(np.max(res - res_ref)), b_res, sorted(set(nnz.tolist())), it))
    assert left_out <= omp_ref.MAX_LEFT_OUT
    assert np.all(np.isfinite(x))
    assert np.all(nnz <= an.s)
    assert it == int(nnz.max())
    assert same, 'supports differ on %d compared rows' % int(np.sum(np.any((x != 0) != (an.x != 0), axis=1) & keep))
    assert np.array_equal(nnz[keep], an.steps[keep])
    assert err <= b_coef
    assert float(orth.max()) <= b_orth
    assert float(np.max(res - res_ref)) <= b_res


@pytest.mark.parametrize('case,precision,kind,with_tol', TABLE)
def test_table_cases(case, precision, kind, with_tol):
    from decomp_amd import omp
    an = mr.case_analysis(case, kind, with_tol)
    dt = an.dtype(precision)
    if with_tol:
        assert len(set(an.steps.tolist())) >= 2
        it, x = omp.solve(an.y.astype(dt), an.A.astype(dt), tol=an.tol, mask=an.m.astype(an.rdtype(precision)))
    else:
        it, x = omp.solve(an.y.astype(dt), an.A.astype(dt), n_nonzero_coefs=an.s,
                          mask=an.m.astype(an.rdtype(precision)))
    assert isinstance(x, np.ndarray)
    _check_against(an, precision, it, x, 'case %d %s%s' % (case, kind, ' tol' if with_tol else ''))


@pytest.mark.parametrize('kind', mr.KINDS)
def test_row_passes_are_bitwise_equal(kind):
    """Case 12 in passes of 100, 100 and 57 rows, in one pass, and again: the same bits."""
    an = mr.case_analysis(12, kind, False)
    y, A, m = an.y.astype(np.float32), an.A.astype(np.float32), an.m.astype(np.float32)
    assert y.shape[0] == 257
    it_p, x_p = _abi(y, m, A, an.s, rows_per_pass=100)
    it_0, x_0 = _abi(y, m, A, an.s, rows_per_pass=0)
    it_r, x_r = _abi(y, m, A, an.s, rows_per_pass=100)
    assert it_p == it_0 == it_r
    assert np.array_equal(x_p, x_0)
    assert np.array_equal(x_p, x_r)
    _check_against(an, 'single', it_p, x_p, 'case 12 %s in passes' % kind)
    tol = mr.case_tol(12, kind)
    it_p, x_p = _abi(y, m, A, 24, tol=tol, rows_per_pass=100)
    it_0, x_0 = _abi(y, m, A, 24, tol=tol, rows_per_pass=0)
    assert it_p == it_0 and np.array_equal(x_p, x_0)


@pytest.mark.parametrize('dt', DTYPES)
def test_one_dimensional_mask(dt):
    """One mask for all rows: the Gram form on the scaled problem.  The weights are squares of binary fractions, so
    y sqrt(m) and A sqrt(m) round once and the scaled problem the reference sees is the one the library forms."""
    from decomp_amd import omp
    dt = np.dtype(dt)
    cplx = dt.kind == 'c'
    precision = _precision(dt)
    y, A = omp_ref.single_exact(*omp_ref.make_problem(77, 67, 24, 40, 4, cplx))
    m1 = np.random.RandomState(78).choice([0, .25, 1, 2.25, 4], 24)
    for tol in (None, 0.02 * float(np.median(np.sum(m1 * np.abs(y) ** 2, axis=1)))):
        an = mr.Analysis(y, A, m1, 4 if tol is None else 10, tol=tol, form='gram')
        it, x = omp.solve(y.astype(dt), A.astype(dt), n_nonzero_coefs=an.s, tol=tol, mask=m1)   # (a float64 mask: cast)
        _check_against(an, precision, it, x, '1-D mask tol %s' % tol)
        assert np.all(x[:, np.flatnonzero((np.abs(A) ** 2) @ m1 == 0)] == 0)


@pytest.mark.parametrize('precision', ['single', 'double'])
def test_all_ones_mask_agrees_with_the_unmasked_solve(precision):
    from decomp_amd import omp
    y, A = mr.case_problem(12)
    s = omp_ref.CASES[12][4]
    an = mr.Analysis(y, A, np.ones(y.shape), s)
    an_plain = omp_ref.case_analysis(12, False)
    dt = an.dtype(precision)
    it_m, x_m = omp.solve(y.astype(dt), A.astype(dt), n_nonzero_coefs=s, mask=np.ones(y.shape, dtype=an.rdtype(precision)))
    it_p, x_p = omp.solve(y.astype(dt), A.astype(dt), n_nonzero_coefs=s)
    keep = an.keep(precision) & an_plain.keep(precision)[:y.shape[0]]
    bound = an.bounds(precision)[0] + an_plain.bounds(precision)[0]
    err = float(np.max(np.abs(x_m - x_p)[keep])) / float(np.max(np.abs(an.x)))
    print('all-ones mask %s: compared %d of %d rows, difference %.3g (bound %.3g)'
          % (dt.__name__, keep.sum(), len(keep), err, bound))
    assert 1.0 - keep.mean() <= omp_ref.MAX_LEFT_OUT
    assert np.array_equal((x_m != 0)[keep], (x_p != 0)[keep])
    assert err <= bound
    _check_against(an, precision, it_m, x_m, 'all-ones mask')


@pytest.mark.parametrize('dt', DTYPES)
def test_full_support_is_weighted_least_squares(dt):
    """s = K = 12, F = 20 with exactly 5 channels hidden per row: no support ambiguity, x is the weighted
    least-squares solution."""
    from decomp_amd import omp
    dt = np.dtype(dt)
    cplx = dt.kind == 'c'
    precision = _precision(dt)
    rng = np.random.RandomState(21)
    N, F, K = 37, 20, 12
    y, A = omp_ref.single_exact(_random(rng, cplx, N, F), _random(rng, cplx, K, F))
    m = np.ones((N, F))
    for i in range(N):
        m[i, rng.choice(F, 5, replace=False)] = 0
    want = np.stack([np.linalg.lstsq((A * m[i]).T, y[i] * m[i], rcond=None)[0] for i in range(N)])
    an = mr.Analysis(y, A, m, K)
    assert np.max(np.abs(an.x - want)) <= 1e-12 * np.max(np.abs(want))
    xc = an.cpu(precision)[0]
    bound = max(4 * float(np.max(np.abs(xc - want))) / float(np.max(np.abs(want))), 64 * float(np.finfo(dt).eps))
    it, x = omp.solve(y.astype(dt), A.astype(dt), n_nonzero_coefs=K, mask=m)
    err = float(np.max(np.abs(x - want))) / float(np.max(np.abs(want)))
    print('full support %s: error %.3g (bound %.3g)' % (dt.name, err, bound))
    assert it == K and x.dtype == dt and np.all(x != 0)
    assert err <= bound


@pytest.mark.parametrize('dt', DTYPES)
def test_degenerate_rows(dt):
    dt = np.dtype(dt)
    cplx = dt.kind == 'c'
    rdt = np.zeros(1, dt).real.dtype
    eps = float(np.finfo(dt).eps)
    wide = np.complex128 if cplx else np.float64
    rng = np.random.RandomState(5)
    K, F, N = 6, 16, 4
    A = _random(rng, cplx, K, F)
    y = _random(rng, cplx, N, F)
    m = (rng.rand(N, F) < 0.8).astype(float)
    m[1] = 0                           # row 1: no weight at all
    A[4] = 0                           # row 2: atom 4 would win unmasked, and is entirely hidden in that row
    A[4, :3] = [5, -4, 3]
    y[2] = 3 * A[4] + 0.1 * y[2]
    m[2] = 1
    m[2, :3] = 0
    y, A, m = y.astype(dt), A.astype(dt), m.astype(rdt)
    for tol in (-1.0, 0.0):
        it, x = _abi(y, m, A, K, tol=tol)
        assert np.all(np.isfinite(x))
        assert np.all(x[1] == 0)
        assert x[2, 4] == 0 and np.count_nonzero(x[2]) == K - 1
        it_open, x_open = _abi(y, np.ones_like(m), A, 1)
        assert np.flatnonzero(x_open[2]).tolist() == [4] and it_open == 1
        # the neighbours of the empty row, without it: the same bits
        it_n, x_n = _abi(y[[0, 2, 3]], m[[0, 2, 3]], A, K, tol=tol)
        assert np.array_equal(x_n, x[[0, 2, 3]]) and it_n == it
        xr = mr.reference(y.astype(wide), A.astype(wide), m.astype(np.float64), K)[0]
        assert np.array_equal(x != 0, xr != 0)
        assert np.max(np.abs(x - xr)) <= 1e4 * eps * np.max(np.abs(xr))
    # rows without any weight only: no step at all
    it, x = _abi(y, np.zeros_like(m), A, K)
    assert it == 0 and np.all(x == 0)
    # two atoms equal on the observed channels, different on the hidden ones: K = s = 3, the twin fails the pivot test
    A3 = _random(rng, cplx, 3, F)
    A3[2] = A3[0]
    A3[2, :4] += 1.0
    m3 = np.ones((1, F))
    m3[0, :4] = 0
    y3 = _random(rng, cplx, 1, F)
    y3, A3, m3 = y3.astype(dt), A3.astype(dt), m3.astype(rdt)
    it, x3 = _abi(y3, m3, A3, 3)
    xr = mr.reference(y3.astype(wide), A3.astype(wide), m3.astype(np.float64), 3)[0]
    assert np.all(np.isfinite(x3)) and np.count_nonzero(x3) <= 2 and it == np.count_nonzero(x3)
    # the twins tie exactly on the observed channels (the hidden ones enter every sum as exact zeros): the library
    # takes the lower index; which one a BLAS-backed reference takes is not fixed, so the twins are folded together
    assert x3[0, 2] == 0 and x3[0, 0] != 0 and (xr[0, 0] == 0) != (xr[0, 2] == 0)

    def fold(v):
        return np.array([v[0, 0] + v[0, 2], v[0, 1]])
    assert np.array_equal(fold(x3) != 0, fold(xr) != 0)
    assert np.max(np.abs(fold(x3) - fold(xr))) <= 1e4 * eps * np.max(np.abs(xr))


@pytest.mark.parametrize('dt', DTYPES)
def test_sparsity_at_the_cap(dt):
    """s = 64 real / 32 complex, K = 70, F = 80, N = 67, 90 % observed: the properties only."""
    dt = np.dtype(dt)
    cplx = dt.kind == 'c'
    precision = _precision(dt)
    s = 32 if cplx else 64
    rng = np.random.RandomState(41)
    N, F, K = 67, 80, 70
    y, A = omp_ref.single_exact(_random(rng, cplx, N, F), _random(rng, cplx, K, F) * (0.5 + rng.rand(K, 1)))
    m = (rng.rand(N, F) < 0.9).astype(np.float64)
    an = mr.Analysis(y, A, m, s)
    it, x = _abi(y.astype(dt), m, A.astype(dt), s)
    nnz = np.count_nonzero(x, axis=1)
    orth = float(mr.row_metrics(x, y, A, m)[1].max())
    b_orth = an.bounds(precision)[1]
    print('s = %d %s: steps %s, orthogonality %.3g (bound %.3g)' % (s, dt.name, sorted(set(nnz.tolist())), orth, b_orth))
    assert np.all(np.isfinite(x)) and np.all(nnz <= s) and it == int(nnz.max())
    assert orth <= b_orth


def size_problem(K, cplx, N=67, F=33, S=4):
    """S - 1 random atoms per row and the LAST atom (the end of the last lane block) in every row."""
    y, A = omp_ref.make_problem(200 + K, N, F, K, S - 1, cplx)
    y, A = omp_ref.single_exact(y + 2.5 * A[K - 1], A)
    m = (np.random.RandomState(300 + K).rand(N, F) < 0.7).astype(np.float64)
    return y, A, m


@pytest.mark.parametrize('K', STEP_K)
@pytest.mark.parametrize('dt', ['float32', 'complex64'])
def test_step_kernel_k_boundaries(dt, K):
    """One K on each side of the lane stride and of the scoring chunk, F = 33 (odd), N = 67, s = 4.  On the CPU these
    inputs leave out at most 3 % of the rows."""
    dt = np.dtype(dt)
    y, A, m = size_problem(K, dt.kind == 'c')
    an = mr.Analysis(y, A, m, 4)
    it, x = _abi(y.astype(dt), m, A.astype(dt), 4)
    _check_against(an, 'single', it, x, 'K %d' % K)
    assert np.any(an.x[an.keep('single'), K - 1] != 0)      # the last atom of the last lane block is taken
    # one row alone: the rows are independent, bit for bit
    it1, x1 = _abi(y[:1].astype(dt), m[:1], A.astype(dt), 4)
    assert np.array_equal(x1[0], x[0]) and it1 == int(np.count_nonzero(x[0]))


def test_tensor_y_torch_in_torch_out():
    import torch
    from decomp_amd import omp
    an = mr.case_analysis(12, 'weights', False)
    y, A, m = an.y.astype(np.float32), an.A.astype(np.float32), an.m.astype(np.float32)
    F = y.shape[1]
    it, x = omp.solve(y[:15].reshape(3, 5, F), A, n_nonzero_coefs=an.s, mask=m[:15].reshape(3, 5, F))
    it_flat, x_flat = omp.solve(y[:15], A, n_nonzero_coefs=an.s, mask=m[:15])
    assert x.shape == (3, 5, A.shape[0]) and np.array_equal(x.reshape(15, -1), x_flat) and it == it_flat
    yt, At, mt = torch.from_numpy(y).cuda(), torch.from_numpy(A).cuda(), torch.from_numpy(m).cuda()
    runs = [omp.solve(yt, At, n_nonzero_coefs=an.s, mask=mt) for _ in range(2)]
    assert torch.is_tensor(runs[0][1]) and runs[0][1].is_cuda and runs[0][1].dtype == torch.float32
    assert runs[0][0] == runs[1][0] and torch.equal(runs[0][1], runs[1][1])
    assert np.array_equal(runs[0][1][:15].cpu().numpy(), x_flat)
    with pytest.raises(TypeError):
        omp.solve(yt, At, n_nonzero_coefs=2, mask=m)


def test_invalid_arguments_return_an_error():
    y = np.ones((3, 8), dtype=np.float32)
    A = np.eye(8, dtype=np.float32)
    m = np.ones((3, 8), dtype=np.float32)
    msg, _ = _abi(y, m, A, 2, mask_ndim=3, expect_rc=-1)
    assert 'mask_ndim' in msg
    msg, _ = _abi(y, m, A, 2, mask_ndim=0, expect_rc=-1)
    assert 'mask_ndim' in msg
    msg, _ = _abi(y, m, A, 2, rows_per_pass=-1, expect_rc=-1)
    assert 'rows_per_pass' in msg
    for s in (0, 9, 65):
        msg, _ = _abi(y, m, A, s, expect_rc=-1)
        assert '64' in msg and '32' in msg
    msg, _ = _abi(y.astype(np.complex64), m, np.ones((40, 8), dtype=np.complex64), 33, expect_rc=-1)
    assert '32' in msg
    msg, _ = _abi(y, m, A, 2, tol=float('nan'), expect_rc=-1)
    assert 'NaN' in msg
    msg, _ = _abi(y, m, A, 2, null_mask=True, expect_rc=-1)
    assert 'null' in msg
