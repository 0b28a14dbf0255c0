"""GPU: decomp_amd.template_matching.pursuit and the raw entry dcp_tm_pursuit_* against the NumPy references of
tm_pursuit_ref.py -- supports, coefficients, step counts, per-signal properties, the residual stop, both tiers of the
greedy kernel and their boundary, exact values and exact ties, in all four dtypes.

Signals whose reference selection margin is below delta (1e-4 single, 1e-8 double), and in tol runs signals whose
residual margin is below 1e-4, are left out of the support and coefficient comparison (at most 10 % per case,
asserted); the properties are checked on every signal.  The coefficient and residual bounds are 4 x what mp_gram in
the test dtype on the CPU shows against mp_residual in double, floor 64 eps (tm_pursuit_ref.Analysis.bounds)."""
import ctypes

import numpy as np
import pytest

import tm_pursuit_ref as ref

pytestmark = pytest.mark.gpu

DTYPES = ['float32', 'float64', 'complex64', 'complex128']
REAL = ['float32', 'float64']
SFX = {'float32': 'f32', 'float64': 'f64', 'complex64': 'c64', 'complex128': 'c128'}


def _precision(dt):
    return 'single' if np.dtype(dt) in (np.dtype(np.float32), np.dtype(np.complex64)) else 'double'


def _lds_atoms(dt):
    from decomp_amd import _hip
    return getattr(_hip.load(), 'dcp_tm_pursuit_lds_atoms_' + SFX[np.dtype(dt).name])()


def _check_against(an, dt, it, x, solve, tag):
    """Supports, coefficients, step counts and the per-signal properties of a GPU result against an Analysis.
    solve(y) runs the same call on other signals: a signal alone must give its row of the batch bit for bit, and the
    `it` of that call is the signal's step count."""
    precision = _precision(dt)
    N, stride, padding = an.geom
    assert x.dtype == np.dtype(dt) and x.shape == an.x.shape
    B = x.shape[0]
    keep = an.keep(precision)
    left_out = 1.0 - float(np.mean(keep))
    b_coef, b_res = an.bounds(precision)
    nnz = np.count_nonzero(x.reshape(B, -1), axis=1)
    err = float(np.max(np.abs(x.astype(an.x.dtype) - an.x)[keep], initial=0.0)) / float(np.max(np.abs(an.x)))
    res = ref.residual_norm(x, an.y, an.D, N, stride, padding)
    print('%s %s: left out %.2f %%; coefficient error %.3g (bound %.3g); residual excess %.3g (bound %.3g); '
          'steps %s; it %d' % (tag, np.dtype(dt).name, 100 * left_out, err, b_coef, float(np.max(res - an.res)), b_res,
                               sorted(set(an.steps.tolist())), it))
    assert left_out <= ref.MAX_LEFT_OUT
    assert np.all(np.isfinite(x))
    assert np.array_equal((x != 0)[keep], (an.x != 0)[keep])
    steps = np.zeros(B, dtype=np.int64)
    for b in range(B):
        steps[b], xb = solve(an.y[b:b + 1].astype(dt))
        assert np.array_equal(xb[0], x[b]), 'signal %d alone differs from its row of the batch' % b
    assert np.array_equal(steps[keep], an.steps[keep])
    assert it == int(steps.max())
    assert np.all(nnz <= steps)
    assert err <= b_coef
    assert float(np.max(res - an.res)) <= b_res
    return nnz


def _run(an, dt, positive=False):
    """pursuit on the Analysis' problem in dtype dt, with its n / tol: (it, x, solve) for _check_against."""
    from decomp_amd import template_matching as tm
    N, stride, padding = an.geom
    D = an.D.astype(dt)

    def solve(y):
        return tm.pursuit(y, D, n_nonzero_coefs=an.n, tol=an.tol, stride=stride, padding=padding, positive=positive)
    it, x = solve(an.y.astype(dt))
    assert isinstance(x, np.ndarray)
    return it, x, solve


@pytest.mark.parametrize('dt', DTYPES)
@pytest.mark.parametrize('case', sorted(ref.CASES))
def test_supports_coefficients_and_properties(case, dt):
    nev = ref.CASES[case][-1]
    an = ref.case_analysis(case, np.dtype(dt).kind == 'c', False)
    nnz = _check_against(an, dt, *_run(an, dt), tag='case %d' % case)
    assert np.all(nnz <= nev)


@pytest.mark.parametrize('dt', DTYPES)
@pytest.mark.parametrize('case', sorted(ref.CASES))
def test_residual_stop(case, dt):
    """tol = 0.02 median|y|^2 and the step limit left at its default."""
    an = ref.case_analysis(case, np.dtype(dt).kind == 'c', True)
    assert an.n is None
    _check_against(an, dt, *_run(an, dt), tag='case %d tol' % case)


# ---- the tiers of the greedy kernel ---------------------------------------------------------------------------------
@pytest.mark.parametrize('where', ['below', 'at', 'above', 'at_T3', 'above_T3'])
@pytest.mark.parametrize('dt', DTYPES)
def test_tier_boundary(dt, where):
    """T C one flat index below, at and above the largest size whose correlations live in LDS (and, with three
    templates, at it and one coefficient per template above), events planted on the last atoms too."""
    L = _lds_atoms(dt)
    assert L == 144 * 1024 // np.dtype(dt).itemsize and L % 3 == 0
    T = 3 if where.endswith('T3') else 1
    K = {'below': L - 1, 'at': L, 'above': L + 1, 'at_T3': L, 'above_T3': L + 3}[where]
    S, stride, padding, nev, B = 3, 1, 'SAME', 5, 3
    C = K // T
    N = C - S + 1
    cplx = np.dtype(dt).kind == 'c'
    y, D, x0 = ref.make_problem(K % 1000, B, T, S, N, stride, padding, nev, cplx)
    assert x0.shape == (B, T, C) and T * C == K
    in_lds = K <= L
    assert in_lds == (where in ('below', 'at', 'at_T3'))
    # one more event on the last atom whose taps lie inside the signal, of the last template: the end of the image
    last = int(ref.inside_atoms(S, N, stride, padding)[-1])
    ev = np.zeros((B, T, C), dtype=D.dtype)
    ev[:, T - 1, last] = 3.0
    y = ref.single_exact(y + ref.predict(ev, D, N, stride, padding), D)[0]
    for kw in (dict(n=nev + 1), dict(tol=0.02 * float(np.median(np.sum(np.abs(y) ** 2, axis=1))))):
        an = ref.Analysis(y, D, (N, stride, padding), **kw)
        assert np.all(an.x[:, T - 1, last] != 0)
        _check_against(an, dt, *_run(an, dt), tag='T C = %d (%s tier)' % (K, 'LDS' if in_lds else 'global'))


# ---- directed cases -------------------------------------------------------------------------------------------------
@pytest.mark.parametrize('padding', ['VALID', 'SAME'])
@pytest.mark.parametrize('dt', DTYPES)
def test_dyadic_reselection_exact_values(dt, padding):
    """D = [[1, 1]], y = 2 atom(3) + 1.5 atom(4): atom 3 is taken, then atom 4, then atom 3 again."""
    from decomp_amd import template_matching as tm
    y = np.zeros((1, 10), dtype=dt)
    y[0, 3:5] += 2
    y[0, 4:6] += 1.5
    D = np.ones((1, 2), dtype=dt)
    c = 3 if padding == 'VALID' else 4
    for n, want in ((1, (2.75, 0.0)), (2, (2.75, 1.125)), (3, (2.1875, 1.125))):
        it, x = tm.pursuit(y, D, n_nonzero_coefs=n, padding=padding)
        assert it == n
        assert x[0, 0, c] == want[0] and x[0, 0, c + 1] == want[1]
        assert np.count_nonzero(x) == np.count_nonzero(want)


def _tie_sizes(dt):
    L = _lds_atoms(dt)
    # (K, tied): inside a segment, across lanes, across the segments of one wave's share and of two waves' shares,
    # across the 256-entry stride of the table scan, the last atoms of the LDS tier, across the tier boundary
    return [(4, (1, 2)), (130, (5, 70)), (130, (3, 67)), (300, (255, 256)), (1100, (1023, 1024)), (5000, (40, 4999)),
            (130, (63, 64)), (16500, (16383, 16384)), (L, (L - 2, L - 1)), (L + 1, (5, L)), (L + 1, (L - 1, L)),
            (130, tuple(range(130)))]


@pytest.mark.parametrize('dt', DTYPES)
def test_exact_ties_go_to_the_lowest_flat_index(dt):
    from decomp_amd import template_matching as tm
    dt = np.dtype(dt)
    D = np.ones((1, 1), dtype=dt)
    for K, tied in _tie_sizes(dt):
        y = np.ones((2, K), dtype=dt)
        y[0, list(tied)] = 2
        y[1, list(tied)] = -2
        if dt.kind == 'c':
            y[1, list(tied)] = 2j               # the same magnitude, another phase
            y[1, tied[0]] = 2
        it, x = tm.pursuit(y, D, n_nonzero_coefs=1)
        assert it == 1 and x.shape == (2, 1, K)
        for b in range(2):
            assert np.array_equal(np.flatnonzero(x[b]), [tied[0]]), (K, tied, b)
            assert x[b, 0, tied[0]] == y[b, tied[0]]


@pytest.mark.parametrize('dt', DTYPES)
def test_identical_templates_take_template_zero(dt):
    from decomp_amd import template_matching as tm
    rng = np.random.RandomState(5)
    d = rng.randn(1, 6).astype(dt)
    D = np.concatenate([d, d])
    y = rng.randn(9, 50).astype(dt)
    it, x = tm.pursuit(y, D, n_nonzero_coefs=4)
    assert it == 4 and np.all(x[:, 1] == 0) and np.all(np.count_nonzero(x[:, 0], axis=1) >= 1)


@pytest.mark.parametrize('dt', REAL)
def test_positive(dt):
    from decomp_amd import template_matching as tm
    B, T, S, N, stride, padding, nev = 16, 2, 7, 90, 1, 'SAME', 6
    y, D, x0 = ref.make_problem(41, B, T, S, N, stride, padding, nev, False)
    mixed = (x0.min(axis=(1, 2)) < 0) & (x0.max(axis=(1, 2)) > 0)
    assert mixed.sum() >= B // 2
    an = ref.Analysis(y, D, (N, stride, padding), n=nev, positive=True)
    it, x, solve = _run(an, dt, positive=True)
    _check_against(an, dt, it, x, solve, tag='positive')
    assert np.all(x >= 0) and np.all(an.x >= 0)
    # nothing correlates positively: no step
    yn = -np.abs(y).astype(dt)
    it, x = tm.pursuit(yn, np.abs(D).astype(dt), n_nonzero_coefs=nev, positive=True)
    assert it == 0 and np.all(x == 0)


@pytest.mark.parametrize('dt', DTYPES)
def test_degenerate_inputs(dt):
    from decomp_amd import template_matching as tm
    rng = np.random.RandomState(9)
    D = rng.randn(3, 5).astype(dt)
    D[1] = 0                                    # a zero template is never taken
    y = rng.randn(6, 40).astype(dt)
    y[2] = 0                                    # a zero signal: x = 0, no step
    for kw in (dict(n_nonzero_coefs=7), dict(tol=0.0, n_nonzero_coefs=7)):
        it, x = tm.pursuit(y, D, **kw)
        assert np.all(np.isfinite(x)) and np.all(x[:, 1] == 0) and np.all(x[2] == 0) and it == 7
        assert np.all(np.count_nonzero(x.reshape(6, -1), axis=1)[[0, 1, 3, 4, 5]] >= 1)
    it, x = tm.pursuit(np.zeros_like(y), D, n_nonzero_coefs=7)
    assert it == 0 and np.all(x == 0)
    it, x = tm.pursuit(np.zeros_like(y), D, tol=0.0)
    assert it == 0 and np.all(x == 0)
    # exact dyadic data, more steps allowed than there are events: the loop stops on a zero maximum
    y = np.zeros((2, 12), dtype=dt)
    y[0, 2:4] = 2
    y[0, 7:9] = -0.5
    y[1, 5:7] = 1
    it, x = tm.pursuit(y, np.ones((1, 2), dtype=dt), n_nonzero_coefs=11, padding='VALID')
    assert it == 2
    assert x[0, 0, 2] == 2 and x[0, 0, 7] == -0.5 and x[1, 0, 5] == 1 and np.count_nonzero(x) == 3
    # an empty batch
    it, x = tm.pursuit(y[:0], np.ones((1, 2), dtype=dt), n_nonzero_coefs=3, padding='VALID')
    assert it == 0 and x.shape == (0, 1, 11)


def test_reproducible_and_the_conventions_of_solve():
    import torch
    from decomp_amd import template_matching as tm
    B, T, S, N, stride, padding, nev = ref.CASES[2]
    y, D = ref.case_problem(2, False)
    y, D = y.astype(np.float32), D.astype(np.float32)
    C = ref.otm.geometry(S, N, stride, padding)[0]
    it, x = tm.pursuit(y[:21].reshape(3, 7, N), D, n_nonzero_coefs=nev, stride=stride, padding=padding)
    it_flat, x_flat = tm.pursuit(y[:21], D, n_nonzero_coefs=nev, stride=stride, padding=padding)
    assert x.shape == (3, 7, T, C) and np.array_equal(x.reshape(21, T, C), x_flat) and it == it_flat
    it1, x1 = tm.pursuit(y[5], D, n_nonzero_coefs=nev, stride=stride, padding=padding)
    assert x1.shape == (T, C) and np.array_equal(x1, x_flat[5])
    yt, Dt = torch.from_numpy(y).cuda(), torch.from_numpy(D).cuda()
    runs = [tm.pursuit(yt, Dt, n_nonzero_coefs=2 * nev, tol=1e-3, stride=stride, padding=padding) for _ in range(2)]
    assert torch.is_tensor(runs[0][1]) and runs[0][1].is_cuda and runs[0][1].dtype == torch.float32
    assert runs[0][0] == runs[1][0] and torch.equal(runs[0][1], runs[1][1])
    # a signal's result does not depend on the rest of the batch
    for b in (0, 13, B - 1):
        itb, xb = tm.pursuit(yt[b:b + 1], Dt, n_nonzero_coefs=2 * nev, tol=1e-3, stride=stride, padding=padding)
        assert torch.equal(xb[0], runs[0][1][b])
    assert np.array_equal(runs[0][1].cpu().numpy(),
                          tm.pursuit(y, D, n_nonzero_coefs=2 * nev, tol=1e-3, stride=stride, padding=padding)[1])
    pred = tm.predict(runs[0][1], Dt, N, stride, padding)
    assert float((yt - pred).norm()) < 0.5 * float(yt.norm())
    with pytest.raises(TypeError):
        tm.pursuit(yt, D, n_nonzero_coefs=2)


# ---- the raw entry ----------------------------------------------------------------------------------------------------
def _raw(y, D, B, T, S, N, stride, pad, n, tol=-1.0, positive=0, expect_rc=0, null=None):
    """dcp_tm_pursuit_* on host arrays: (it, x).  x starts as NaN: the entry writes all of it."""
    import torch
    from decomp_amd import _arrays, _hip
    from decomp_amd.template_matching import _coef_size
    yd = torch.from_numpy(np.ascontiguousarray(y)).cuda()
    Dd = torch.from_numpy(np.ascontiguousarray(D)).cuda()
    C = max(_coef_size(S, N, max(stride, 1), 'SAME' if pad else 'VALID'), 1) if S <= N else 1
    x = torch.full((max(B, 1), max(T, 1), C), float('nan'), dtype=yd.dtype, device='cuda')
    lib, h = _arrays.lib_handle(yd)
    it = ctypes.c_int(-1)
    name = 'dcp_tm_pursuit_' + _arrays.suffix(yd)
    ptrs = {'Y': _arrays.ptr(yd), 'D': _arrays.ptr(Dd), 'X': _arrays.ptr(x), 'it': ctypes.byref(it)}
    if null is not None:
        ptrs[null] = None
    rc = getattr(lib, name)(h, ptrs['Y'], ptrs['D'], ptrs['X'], B, T, S, N, stride, pad, n, float(tol), positive,
                            ptrs['it'])
    if expect_rc != 0:
        assert rc == expect_rc, rc
        return lib.dcp_last_error_string(h).decode(), None
    _hip.check(h, rc, name)
    return it.value, x.cpu().numpy()


@pytest.mark.parametrize('dt', DTYPES)
def test_raw_entry_writes_all_of_x(dt):
    B, T, S, N, stride, padding, nev = ref.CASES[2]
    an = ref.case_analysis(2, np.dtype(dt).kind == 'c', False)
    D = an.D.astype(dt)
    it, x = _raw(an.y.astype(dt), D, B, T, S, N, stride, 1, nev)
    assert np.all(np.isfinite(x))
    _check_against(an, dt, it, x, lambda y: _raw(y, D, y.shape[0], T, S, N, stride, 1, nev), tag='raw')


def test_raw_entry_invalid_arguments_return_an_error():
    y = np.ones((3, 20), dtype=np.float32)
    D = np.ones((2, 4), dtype=np.float32)
    ok = (3, 2, 4, 20, 1, 1)                    # C = 23, T C = 46
    for geom in ((0, 2, 4, 20, 1, 1), (3, 0, 4, 20, 1, 1), (3, 2, 0, 20, 1, 1), (3, 2, 21, 20, 1, 1),
                 (3, 2, 4, 20, 0, 1), (3, 2, 4, 20, -2, 0)):
        msg, _ = _raw(y, D, *geom, 2, expect_rc=-1)
        assert 'geometry' in msg
    for n in (0, -1, 47, 2 ** 40):
        msg, _ = _raw(y, D, *ok, n, expect_rc=-1)
        assert 'n_steps' in msg
    msg, _ = _raw(y, D, *ok, 2, tol=float('nan'), expect_rc=-1)
    assert 'NaN' in msg
    msg, _ = _raw(y.astype(np.complex64), D.astype(np.complex64), *ok, 2, positive=1, expect_rc=-1)
    assert 'real' in msg
    for null in ('Y', 'D', 'X', 'it'):
        msg, _ = _raw(y, D, *ok, 2, expect_rc=-1, null=null)
        assert 'null' in msg
    it, x = _raw(y, D, *ok, 46)                 # the largest n_steps is accepted
    assert np.all(np.isfinite(x))
