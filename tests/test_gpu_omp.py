"""GPU: decomp_amd.omp.solve and the greedy kernel alone (dcp_omp_gram_*) against the NumPy references of
omp_ref.py -- supports, coefficients, per-row properties, the residual stop, every alpha0 tier and the
wave-boundary sizes, in all four dtypes.

Rows whose reference selection margin is below delta (1e-4 single, 1e-8 double), and in tol runs rows whose
residual margin is below 1e-4, are left out of the SUPPORT comparison (at most 10 % per case, asserted); the
properties are checked on every row.  The coefficient, orthogonality and residual bounds are not fixed in advance:
they are 4 x what omp_gram in the test dtype on the CPU shows against omp_lstsq in double, floor 64 eps
(omp_ref.Analysis.bounds)."""
import ctypes

import numpy as np
import pytest

import omp_ref

pytestmark = pytest.mark.gpu

CASE_PARAMS = [(c, p) for c in sorted(omp_ref.CASES)
               for p in (('single', 'double') if c in omp_ref.SINGLE_CASES else ('double',))]
DTYPES = ['float32', 'float64', 'complex64', 'complex128']


def _gram(alpha0, G, yn2, s, tol=-1.0, expect_rc=0):
    """dcp_omp_gram_* on host arrays: (it, x).  x starts as NaN: the kernel writes all of it."""
    import torch
    from decomp_amd import _arrays, _hip
    a = torch.from_numpy(np.ascontiguousarray(alpha0)).cuda()
    g = torch.from_numpy(np.ascontiguousarray(G)).cuda()
    yn = None if yn2 is None else torch.from_numpy(np.ascontiguousarray(yn2)).cuda()
    x = torch.full_like(a, float('nan'))
    lib, h = _arrays.lib_handle(a)
    it = ctypes.c_int(-1)
    name = 'dcp_omp_gram_' + _arrays.suffix(a)
    rc = getattr(lib, name)(h, _arrays.ptr(a), _arrays.ptr(g), _arrays.ptr(yn), _arrays.ptr(x), a.shape[0],
                            a.shape[1], int(s), float(tol), ctypes.byref(it))
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
    left_out = 1.0 - float(np.mean(keep))
    b_coef, b_orth, b_res = an.bounds(precision)
    nnz = np.count_nonzero(x, axis=1)
    xd = x.astype(an.x.dtype)
    err = float(np.max(np.abs(xd - an.x)[keep], initial=0.0)) / float(np.max(np.abs(an.x)))
    res, orth = omp_ref.row_metrics(x, an.y, an.A)
    res_ref, _ = omp_ref.row_metrics(an.x, an.y, an.A)
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


@pytest.mark.parametrize('case,precision', CASE_PARAMS)
def test_supports_coefficients_and_properties(case, precision):
    from decomp_amd import omp
    an = omp_ref.case_analysis(case, False)
    dt = an.dtype(precision)
    it, x = omp.solve(an.y.astype(dt), an.A.astype(dt), n_nonzero_coefs=an.s)
    assert isinstance(x, np.ndarray)
    _check_against(an, precision, it, x, 'case %d' % case)


@pytest.mark.parametrize('case,precision', CASE_PARAMS)
def test_residual_stop(case, precision):
    """tol = 0.02 median|y|^2 and no sparsity: rows stop at different steps."""
    from decomp_amd import omp
    an = omp_ref.case_analysis(case, True)
    dt = an.dtype(precision)
    assert len(set(an.steps.tolist())) >= 2
    it, x = omp.solve(an.y.astype(dt), an.A.astype(dt), tol=an.tol)
    _check_against(an, precision, it, x, 'case %d tol' % case)


def _random(rng, cplx, *shape):
    return rng.randn(*shape) + 1j * rng.randn(*shape) if cplx else rng.randn(*shape)


@pytest.mark.parametrize('dt', DTYPES)
def test_full_support_is_least_squares(dt):
    """s = K = 12, F = 20: no support ambiguity, x is the least-squares solution."""
    from decomp_amd import omp
    dt = np.dtype(dt)
    cplx = dt.kind == 'c'
    precision = 'single' if dt.itemsize == (8 if cplx else 4) else 'double'
    rng = np.random.RandomState(21)
    y, A = omp_ref.single_exact(_random(rng, cplx, 37, 20), _random(rng, cplx, 12, 20))
    want = np.linalg.lstsq(A.T, y.T, rcond=None)[0].T
    an = omp_ref.Analysis(y, A, 12)
    assert np.max(np.abs(an.x - want)) <= 1e-12 * np.max(np.abs(want))
    xc = an.cpu(precision)[0]
    bound = max(4 * float(np.max(np.abs(xc - want))) / float(np.max(np.abs(want))), 64 * float(np.finfo(dt).eps))
    it, x = omp.solve(y.astype(dt), A.astype(dt), n_nonzero_coefs=12)
    err = float(np.max(np.abs(x - want))) / float(np.max(np.abs(want)))
    print('full support %s: error %.3g (bound %.3g)' % (dt.name, err, bound))
    assert it == 12 and x.dtype == dt and np.all(x != 0)
    assert err <= bound


@pytest.mark.parametrize('dt', DTYPES)
def test_sparsity_at_the_cap(dt):
    """s = 64 real / 32 complex, K = 70, F = 80, N = 67 (the problem of test_gpu_omp_mask's test of this name, without
    the mask): the factor at its full size.  The reference takes s steps in every row; the properties only."""
    from decomp_amd import omp
    dt = np.dtype(dt)
    cplx = dt.kind == 'c'
    precision = 'single' if dt.itemsize == (8 if cplx else 4) else 'double'
    s = 32 if cplx else 64
    rng = np.random.RandomState(41)
    N, F, K = 67, 80, 70
    y, A = omp_ref.single_exact(_random(rng, cplx, N, F), _random(rng, cplx, K, F) * (0.5 + rng.rand(K, 1)))
    an = omp_ref.Analysis(y, A, s)
    assert np.all(an.steps == s)
    it, x = omp.solve(y.astype(dt), A.astype(dt), n_nonzero_coefs=s)
    nnz = np.count_nonzero(x, axis=1)
    orth = float(omp_ref.row_metrics(x, y, A)[1].max())
    b_orth = an.bounds(precision, np.ones(N, dtype=bool))[1]
    print('s = %d %s: steps %s, orthogonality %.3g (bound %.3g)' % (s, dt.name, sorted(set(nnz.tolist())), orth, b_orth))
    assert np.all(np.isfinite(x))
    assert np.all(nnz == s) and it == s
    assert orth <= b_orth


# ---- the greedy kernel alone ---------------------------------------------------------------------------------
@pytest.mark.parametrize('dt', DTYPES)
def test_duplicate_zero_atom_and_zero_row(dt):
    """Atoms 1 and 3 identical: the lower index is taken and the duplicate fails the dependence test without a NaN;
    atom 2 zero: never selected; row 1 zero: x = 0 and no step."""
    dt = np.dtype(dt)
    cplx = dt.kind == 'c'
    rng = np.random.RandomState(31)
    K, F, N = 6, 16, 5
    A = _random(rng, cplx, K, F).astype(dt)
    A[3] = A[1]
    A[2] = 0
    y = _random(rng, cplx, N, F).astype(dt)
    y[1] = 0
    alpha0, G = y @ A.conj().T, A @ A.conj().T
    G[3, :], G[:, 3], alpha0[:, 3] = G[1, :], G[:, 1], alpha0[:, 1]      # exact duplicates, whatever the BLAS does
    yn2 = np.sum(np.abs(y) ** 2, axis=1).astype(G.real.dtype)
    for tol in (-1.0, 0.0):
        it, x = _gram(alpha0, G, yn2 if tol >= 0 else None, K, tol=tol)
        assert np.all(np.isfinite(x))
        assert np.all(x[:, 2] == 0) and np.all(x[:, 3] == 0)
        assert np.all(x[1] == 0)
        live = [0, 2, 3, 4]
        assert np.all(x[live][:, [0, 1, 4, 5]] != 0)
        assert it == 4
        sup = [0, 1, 4, 5]
        want = np.linalg.lstsq(A[sup].astype(np.complex128 if cplx else np.float64).T,
                               y[live].astype(np.complex128 if cplx else np.float64).T, rcond=None)[0].T
        assert np.max(np.abs(x[live][:, sup] - want)) <= 1e4 * float(np.finfo(dt).eps) * np.max(np.abs(want))
    # a problem of zero rows only: no step at all
    it, x = _gram(np.zeros_like(alpha0), G, None, K)
    assert it == 0 and np.all(x == 0)
    # two atoms, both the same: one step, then the only candidate is the duplicate
    G2 = np.full((2, 2), 4.0, dtype=dt)
    it, x = _gram(np.array([[3.0, 3.0]], dtype=dt), G2, None, 2)
    assert it == 1 and x[0, 0] == dt.type(0.75) and x[0, 1] == 0
    # ... and with a correlation left on it, it reaches the dependence test: pivot 4 - |4 / 2|^2 = 0
    it, x = _gram(np.array([[3.0, 2.75]], dtype=dt), G2, None, 2)
    assert it == 1 and x[0, 0] == dt.type(0.75) and x[0, 1] == 0


@pytest.mark.parametrize('dt', DTYPES)
def test_exact_ties_go_to_the_lowest_index(dt):
    """G = I: the correlations are alpha0 itself.  Ties inside a lane's share, across lanes and across the
    butterfly's halves."""
    dt = np.dtype(dt)
    for K, tied in ((4, (1, 2)), (130, (5, 70)), (130, (3, 67)), (130, (40, 129)), (300, (255, 256)),
                    (130, tuple(range(130)))):
        alpha0 = np.ones((2, K), dtype=dt)
        alpha0[0, list(tied)] = 2
        alpha0[1, list(tied)] = -2
        if dt.kind == 'c':
            alpha0[1, list(tied)] = 2j          # the same magnitude, another phase
            alpha0[1, tied[0]] = 2
        it, x = _gram(alpha0, np.eye(K, dtype=dt), None, 1)
        assert it == 1
        assert np.array_equal(np.flatnonzero(x[0]), [tied[0]]) and np.array_equal(np.flatnonzero(x[1]), [tied[0]])
        assert x[0, tied[0]] == alpha0[0, tied[0]] and x[1, tied[0]] == alpha0[1, tied[0]]


@pytest.mark.parametrize('K', [1, 63, 64, 65])
@pytest.mark.parametrize('dt', DTYPES)
def test_wave_boundary_sizes(dt, K):
    """s in {1, cap (or K below it)}, K around the wave, N = 65 and N = 1."""
    dt = np.dtype(dt)
    cplx = dt.kind == 'c'
    precision = 'single' if dt.itemsize == (8 if cplx else 4) else 'double'
    cap = 32 if cplx else 64
    rng = np.random.RandomState(100 + K)
    N, F = 65, K + 7
    A = _random(rng, cplx, K, F) * (0.5 + rng.rand(K, 1))
    x0 = _random(rng, cplx, N, K) * (rng.rand(N, K) < 0.3)
    y, A = omp_ref.single_exact(x0 @ A + 0.05 * _random(rng, cplx, N, F), A)
    for s in sorted({1, min(cap, K)}):
        an = omp_ref.Analysis(y, A, s)
        alpha0, G, _ = an.products(precision)
        it, x = _gram(alpha0, G, None, s)
        # s = K: every atom is taken, in whatever order -- all rows are compared; else the rows with a margin
        keep = np.ones(N, dtype=bool) if s == K else an.keep(precision)
        b_coef = an.bounds(precision, keep)[0]
        err = float(np.max(np.abs(x - an.x)[keep], initial=0.0)) / float(np.max(np.abs(an.x)))
        print('K %d s %d %s: compared %d of %d rows, error %.3g (bound %.3g)' % (K, s, dt.name, keep.sum(), N, err, b_coef))
        assert np.all(np.isfinite(x)) and np.all(np.count_nonzero(x, axis=1) <= s)
        assert it == int(np.count_nonzero(x, axis=1).max())
        assert np.array_equal((x != 0)[keep], (an.x != 0)[keep])
        assert err <= b_coef
        assert float(omp_ref.row_metrics(x, y, A)[1].max()) <= an.bounds(precision, keep)[1]
        # one row alone: the rows are independent, bit for bit
        it1, x1 = _gram(alpha0[:1], G, None, s)
        assert np.array_equal(x1[0], x[0]) and it1 == int(np.count_nonzero(x[0]))


@pytest.mark.parametrize('K', [512, 513, 2048, 2049])
@pytest.mark.parametrize('dt', ['float32', 'complex128'])
def test_alpha0_tiers(dt, K):
    """The last K of the register tier, the first and last of the LDS tier, the first of the global tier."""
    dt = np.dtype(dt)
    cplx = dt.kind == 'c'
    precision = 'single' if dt == np.float32 else 'double'
    rng = np.random.RandomState(K)
    N, F, S = 9, 64, 4
    A = _random(rng, cplx, K, F) * (0.5 + rng.rand(K, 1))
    x0 = np.zeros((N, K))
    for i in range(N):
        x0[i, rng.choice(K, S, replace=False)] = (1 + rng.rand(S)) * rng.choice([-1, 1], S)
    x0[:, K - 1] = 2.5              # the last atom of the last pass is in every support
    y, A = omp_ref.single_exact(x0 @ A + 0.01 * _random(rng, cplx, N, F), A)
    tol = 0.02 * float(np.median(np.sum(np.abs(y) ** 2, axis=1)))
    for t in (None, tol):
        s = S + 1 if t is None else 10       # the atoms that are there; with tol: until the residual is small
        an = omp_ref.Analysis(y, A, s, tol=t)
        alpha0, G, yn2 = an.products(precision)
        it, x = _gram(alpha0, G, yn2, s, tol=-1.0 if t is None else t)
        keep = an.keep(precision)
        b_coef = an.bounds(precision)[0]
        err = float(np.max(np.abs(x - an.x)[keep], initial=0.0)) / float(np.max(np.abs(an.x)))
        print('K %d %s tol %s: compared %d of %d rows, error %.3g (bound %.3g), steps %s'
              % (K, dt.name, t, keep.sum(), N, err, b_coef, sorted(set(an.steps.tolist()))))
        nnz = np.count_nonzero(x, axis=1)
        assert np.all(np.isfinite(x)) and it == int(nnz.max())
        assert keep.sum() >= N // 2 and np.any(an.x[keep][:, K - 1] != 0)
        assert np.array_equal((x != 0)[keep], (an.x != 0)[keep])
        assert err <= b_coef


def test_invalid_arguments_return_an_error():
    a = np.ones((3, 8), dtype=np.float32)
    G = np.eye(8, dtype=np.float32)
    for s in (0, -1, 9, 65):
        msg, _ = _gram(a, G, None, s, expect_rc=-1)
        assert '64' in msg and '32' in msg
    msg, _ = _gram(a.astype(np.complex64), G.astype(np.complex64), None, 33, expect_rc=-1)
    assert '32' in msg
    msg, _ = _gram(a, G, None, 2, tol=0.5, expect_rc=-1)          # tol >= 0 needs ynorm2
    assert 'ynorm2' in msg
    msg, _ = _gram(a, G, None, 2, tol=float('nan'), expect_rc=-1)


# ---- the conventions of lasso.solve ------------------------------------------------------------------------------
def test_tensor_y_torch_in_torch_out_and_bitwise_repeatable():
    import torch
    from decomp_amd import omp
    an = omp_ref.case_analysis(12, False)
    y, A = an.y.astype(np.float32), an.A.astype(np.float32)
    it, x = omp.solve(y[:21].reshape(3, 7, -1), A, n_nonzero_coefs=an.s)
    it_flat, x_flat = omp.solve(y[:21], A, n_nonzero_coefs=an.s)
    assert x.shape == (3, 7, A.shape[0]) and np.array_equal(x.reshape(21, -1), x_flat) and it == it_flat
    yt, At = torch.from_numpy(y).cuda(), torch.from_numpy(A).cuda()
    runs = [omp.solve(yt, At, n_nonzero_coefs=an.s, tol=an.s * 1e-3) for _ in range(2)]
    assert torch.is_tensor(runs[0][1]) and runs[0][1].is_cuda and runs[0][1].dtype == torch.float32
    assert runs[0][0] == runs[1][0] and torch.equal(runs[0][1], runs[1][1])
    assert np.array_equal(runs[0][1][:21].cpu().numpy(), omp.solve(y[:21], A, n_nonzero_coefs=an.s, tol=an.s * 1e-3)[1])
    with pytest.raises(TypeError):
        omp.solve(yt, A, n_nonzero_coefs=2)
