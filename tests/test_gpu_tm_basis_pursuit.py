"""GPU: decomp_amd.template_matching.basis_pursuit with multichannel templates D [T, Ch, S] (dcp_tm_mc_lasso_*, the
proximal-gradient LASSO in Gram form) against the oracle, oracle.lasso.solve_fastpath on the dense operator
[T C, Ch N] in double (tm_basis_pursuit_ref.py): every geometry at which a piece of the step kernel can go wrong, in
four dtypes, three methods and their positive forms; the reference's own outputs (tests/golden); the stop bookkeeping;
the new entry at Ch = 1 against the one-channel solver, 'VALID' against the one-channel solver on the interleaved
problem; bit-for-bit reproducibility; the calling conventions; the refusal above the edge table's limit.

Limits (the project's own): relative max-norm error below 1e-10 in the double dtypes (test_lasso_multi_tile) and below
2e-4 in the single dtypes (test_solve_fixtures).  Every test prints the error it found."""
import numpy as np
import pytest

import tm_basis_pursuit_ref as ref
import tm_multichannel_ref as mc

pytestmark = pytest.mark.gpu

DTYPES = ['float32', 'float64', 'complex64', 'complex128']
LIMIT = {'float32': 2e-4, 'complex64': 2e-4, 'float64': 1e-10, 'complex128': 1e-10}


def _bp(*a, **k):
    from decomp_amd import template_matching as tm
    return tm.basis_pursuit(*a, **k)


def _methods(dtype):
    return ref.METHODS + (('ista_pos', 'acc_ista_pos', 'fista_pos') if np.dtype(dtype).kind == 'f' else ())


# ---- geometries against the oracle ---------------------------------------------------------------------------------------
@pytest.mark.parametrize('dtype', DTYPES)
@pytest.mark.parametrize('name', [n for n in sorted(ref.GEOMS) if n != 'no_lds'])
def test_geometries_against_the_oracle(name, dtype):
    cplx = np.dtype(dtype).kind == 'c'
    y, D, x0, alpha = ref.problem(name, cplx)
    stride, padding = ref.GEOMS[name][5:]
    yd, Dd, xd = y.astype(dtype), D.astype(dtype), x0.astype(dtype)
    for j, method in enumerate(_methods(dtype)):
        maxiter = 3 + j % 2
        if method.endswith('_pos'):
            it_ref, x_ref = ref.oracle(y, D, alpha, x0, 0.0, maxiter, method, stride, padding, A=ref.operator(name, cplx))
        else:
            it_ref, x_ref = ref.oracle_case(name, cplx, method, maxiter)
        it, x = _bp(yd, Dd, alpha, x=xd, tol=0.0, maxiter=maxiter, method=method, stride=stride, padding=padding)
        err = ref.rel_err(x, x_ref)
        print('%s %s %s maxiter %d: it %d, relative error %.3g' % (name, dtype, method, maxiter, it, err))
        assert x.dtype == np.dtype(dtype) and x.shape == x0.shape and it == it_ref == maxiter - 1
        assert err < LIMIT[dtype], (method, err)
        assert np.any(x_ref == 0) and np.any(x_ref != 0)              # the threshold acts, the code is not empty


@pytest.mark.parametrize('dtype', DTYPES)
def test_iterate_window_beyond_the_lds_budget(dtype):
    """2 dh + 1 = 5899 taps: the tile's window of the iterate does not fit the LDS budget in the 8- and 16-byte dtypes
    and the step reads the iterate from global memory, guarded (in float32 the same shape stays on the LDS path)."""
    from decomp_amd import _hip
    cplx = np.dtype(dtype).kind == 'c'
    B, T, Ch, S, N, stride, padding = ref.GEOMS['no_lds']
    nd = 2 * ((S - 1) // stride) + 1
    cpp = getattr(_hip.load(), 'dcp_tm_mc_channels_per_pass_' + {'float32': 'f32', 'float64': 'f64', 'complex64': 'c64',
                                                                 'complex128': 'c128'}[dtype])(nd, 1)
    assert (cpp == 0) == (dtype != 'float32')
    y, D, x0, alpha = ref.problem('no_lds', cplx)
    it_ref, x_ref = ref.oracle_case('no_lds', cplx, 'acc_ista', 3)
    it, x = _bp(y.astype(dtype), D.astype(dtype), alpha, x=x0.astype(dtype), tol=0.0, maxiter=3, stride=stride,
                padding=padding)
    err = ref.rel_err(x, x_ref)
    print('no_lds %s: relative error %.3g' % (dtype, err))
    assert it == it_ref and err < LIMIT[dtype]


# ---- the reference's own outputs -----------------------------------------------------------------------------------------
@pytest.mark.parametrize('case', ref.GOLDEN_CASES, ids=[c[0] for c in ref.GOLDEN_CASES])
def test_golden_vectors(case):
    tag, dtype, method, stride, padding, maxiter, tol = case
    gold = np.load(ref.GOLDEN)
    y, D, x0 = gold[tag + '_y'], gold[tag + '_D'], gold[tag + '_x0']
    it, x = _bp(y, D, float(gold[tag + '_alpha']), x=x0, tol=tol, maxiter=maxiter, method=method, stride=stride,
                padding=padding)
    err = ref.rel_err(x, gold[tag + '_x'].reshape(x0.shape))
    print('golden %s %s %s: it %d, relative error %.3g' % (tag, dtype, method, it, err))
    assert it == int(gold[tag + '_it']) and x.dtype == np.dtype(dtype)
    assert err < LIMIT[dtype]


# ---- stop bookkeeping ------------------------------------------------------------------------------------------------
@pytest.mark.parametrize('maxiter', ref.STOP_MAXITER)
@pytest.mark.parametrize('method', ref.METHODS)
def test_iteration_count_edges(method, maxiter):
    """The cases of test_structured_lasso_iteration_count_edges on a 3-channel problem, float64: exhaustion, a check on
    the very last iteration (11, 21), the test met on the last iteration (21 at tol 3e-3), an exit at iteration 20 with
    iteration 21 discarded (31 at tol 3e-3), an exit at iteration 0 (tol 1e3) -- count and codes against the oracle."""
    y, D, A, C = ref.stop_problem(method)
    B, T = y.shape[0], D.shape[0]
    stride, padding = ref.STOP_SHAPE[5:]
    for tol in ref.STOP_TOL:
        trace = []
        it_ref, x_ref = ref.oracle(y, D, ref.STOP_ALPHA, np.zeros((B, T, C)), tol, maxiter, method, stride, padding,
                                   trace=trace, A=A)
        stats = [float(np.max(t)) for t in trace]
        print(method, maxiter, tol, 'it', it_ref, 'stop statistics', stats)
        assert ref.stop_margin_ok(stats, tol), stats      # no stop decision may hang on rounding
        it, x = _bp(y, D, ref.STOP_ALPHA, tol=tol, maxiter=maxiter, method=method, stride=stride, padding=padding)
        err = float(np.max(np.abs(x - x_ref)))
        print('  it', it, 'max|x - x_oracle|', err)
        assert it == it_ref, (tol, it, it_ref)
        assert err <= 1e-10 * max(1.0, float(np.max(np.abs(x_ref)))), (tol, err)


# ---- against the existing solver -----------------------------------------------------------------------------------------
@pytest.mark.parametrize('dtype', DTYPES)
@pytest.mark.parametrize('geom', [(40, 5, 1, 'SAME'), (300, 33, 1, 'SAME'), (64, 8, 2, 'VALID')])
def test_one_channel_against_the_one_channel_solver(geom, dtype):
    """dcp_tm_mc_lasso_* at Ch = 1 against dcp_tm_lasso_*: the two forms re-associate the sums, so not bit for bit."""
    N, S, stride, padding = geom
    cplx = np.dtype(dtype).kind == 'c'
    y, D, x0, alpha = ref.make_problem(50 + N, 3, 3, 1, S, N, stride, padding, cplx)
    y, D, x0 = y.astype(dtype), D.astype(dtype), x0.astype(dtype)
    for method, maxiter, tol in (('acc_ista', 4, 0.0), ('fista', 12, 1e-3), ('ista', 11, 1e-3)):
        it1, x1 = _bp(y[:, 0], D[:, 0], alpha, x=x0, tol=tol, maxiter=maxiter, method=method, stride=stride,
                      padding=padding)
        it, x = _bp(y, D, alpha, x=x0, tol=tol, maxiter=maxiter, method=method, stride=stride, padding=padding)
        err = ref.rel_err(x, x1.astype(np.complex128 if cplx else np.float64))
        print('%s %s %s: it %d / %d, relative difference %.3g' % (geom, dtype, method, it, it1, err))
        assert it == it1 and err < LIMIT[dtype]


@pytest.mark.parametrize('dtype', DTYPES)
def test_valid_against_the_interleaved_one_channel_problem(dtype):
    """'VALID', Ch = 3, stride 2: the one-channel solver on the channel-interleaved signal with stride 2 Ch is the same
    problem (its n is N Ch too)."""
    cplx = np.dtype(dtype).kind == 'c'
    B, T, Ch, S, N, stride = 3, 2, 3, 7, 48, 2
    y, D, x0, alpha = ref.make_problem(77, B, T, Ch, S, N, stride, 'VALID', cplx)
    y, D, x0 = y.astype(dtype), D.astype(dtype), x0.astype(dtype)
    y1, D1 = mc.interleave(y, D)
    for method in ref.METHODS:
        it1, x1 = _bp(y1, D1, alpha, x=x0, tol=0.0, maxiter=4, method=method, stride=stride * Ch, padding='VALID')
        it, x = _bp(y, D, alpha, x=x0, tol=0.0, maxiter=4, method=method, stride=stride, padding='VALID')
        err = ref.rel_err(x, x1.astype(np.complex128 if cplx else np.float64))
        print('%s %s: relative difference %.3g' % (dtype, method, err))
        assert it == it1 and x.shape == x1.shape and err < LIMIT[dtype]


# ---- reproducibility ---------------------------------------------------------------------------------------------------
@pytest.mark.parametrize('dtype', DTYPES)
@pytest.mark.parametrize('name', ['tiles_same', 'templates', 'none_inside'])
def test_bits_are_reproducible_and_independent_of_the_batch(name, dtype):
    cplx = np.dtype(dtype).kind == 'c'
    y, D, x0, alpha = ref.problem(name, cplx)
    stride, padding = ref.GEOMS[name][5:]
    y, D, x0 = y.astype(dtype), D.astype(dtype), x0.astype(dtype)
    kw = dict(tol=0.0, maxiter=4, method='fista', stride=stride, padding=padding)
    _, xa = _bp(y, D, alpha, x=x0, **kw)
    _, xb = _bp(y, D, alpha, x=x0, **kw)
    assert np.array_equal(xa.view(np.uint8), xb.view(np.uint8))
    for b in range(y.shape[0]):
        _, xs = _bp(y[b], D, alpha, x=x0[b], **kw)
        assert np.array_equal(xs.view(np.uint8), xa[b].view(np.uint8)), b


# ---- calling conventions -------------------------------------------------------------------------------------------------
def test_calling_conventions():
    import torch
    y, D, x0, alpha = ref.problem('tile_s2_same', False)
    stride, padding = ref.GEOMS['tile_s2_same'][5:]
    kw = dict(tol=0.0, maxiter=3, stride=stride, padding=padding)
    it, x = _bp(y, D, alpha, x=x0, **kw)
    assert isinstance(x, np.ndarray)
    # torch in, torch out; the given x is not modified
    yt, Dt, xt = (torch.from_numpy(np.array(a)).cuda() for a in (y, D, x0))
    keep = xt.clone()
    it_t, x_t = _bp(yt, Dt, alpha, x=xt, **kw)
    assert isinstance(x_t, torch.Tensor) and x_t.is_cuda and it_t == it
    assert torch.equal(xt, keep) and x_t.data_ptr() != xt.data_ptr()
    assert np.array_equal(x_t.cpu().numpy(), x)
    xn = np.array(x0)
    _bp(y, D, alpha, x=xn, **kw)
    assert np.array_equal(xn, x0)
    # one signal: y [Ch, N] -> x [T, C]
    _, x1 = _bp(y[1], D, alpha, x=x0[1], **kw)
    assert x1.shape == x0.shape[1:] and np.array_equal(x1, x[1])
    # leading batch dimensions
    y4 = np.stack([y, y[::-1]], 0)
    x4 = np.stack([x0, x0[::-1]], 0)
    _, xo = _bp(y4, D, alpha, x=x4, **kw)
    assert xo.shape == x4.shape and np.array_equal(xo[0], x) and np.array_equal(xo[1], x[::-1])
    # x = None starts from zero
    _, xz = _bp(y, D, alpha, **kw)
    _, xz0 = _bp(y, D, alpha, x=np.zeros_like(x0), **kw)
    assert np.array_equal(xz, xz0)
    # an empty batch
    it_e, xe = _bp(y[:0], D, alpha, **kw)
    assert xe.shape == (0,) + x0.shape[1:] and it_e == 0


def test_table_limit_is_refused_before_anything_runs():
    """'SAME' with S = 1025, T = 16: 2048 atoms reach outside the signal and their table [ne, T, T, 2 dh + 1] would take
    4.3 GB in float32.  The entry fails with DCP_ERR_INVALID, naming the size (it checks the size before it lays out
    its workspace or launches anything); the error surfaces as the library's usual exception."""
    from decomp_amd import _hip
    T, S, N = 16, 1025, 1100
    y = np.zeros((1, 1, N), dtype=np.float32)
    D = np.ones((T, 1, S), dtype=np.float32)
    with pytest.raises(_hip.HipLibraryError, match=r'DCP_ERR_INVALID.*edge table.* %d bytes' % (2048 * T * T * 2049 * 4)):
        _bp(y, D, 0.1, maxiter=1)
    it, x = _bp(y, D, 0.1, maxiter=1, padding='VALID')               # no table: the same templates run
    assert x.shape == (1, T, N - S + 1) and not np.any(x)
