"""GPU: every dcp_tm_* kernel of decomp_amd.template_matching against the float64 oracle
(oracle/template_matching.py, itself pinned to the reference's fixtures in tests/test_oracle_golden.py), in
all four dtypes, past the 256-wide tiles of both LASSO passes, on both sides of their LDS budget and at the
geometry edges.

Rounding model for float32 / complex64 (unit roundoff u = 2^-24):
  * one pass (predict, the statistics): elementwise |err| <= gamma_n (|x| |A|) with n the number of taps per
    output, gamma_n = n u / (1 - n u), and a complex product counted as two real ones (gamma_{2n+4});
  * an iterated solve: the same oracle run in single precision on the same rounded inputs measures the
    rounding floor; the kernel must stay within FLOOR_MULT times that floor (never below u max|ref|).
Every single-precision bound is asserted to stay below 1e-3 relative.  Double precision is held to 1e-10.
"""
import numpy as np
import pytest

from oracle import template_matching as otm

pytestmark = pytest.mark.gpu

DTYPES = ['float32', 'float64', 'complex64', 'complex128']
U32 = 2.0 ** -24
FLOOR_MULT = 16.0
LDS_BYTES = 48 * 1024          # kTmLdsBytes of template_impl.hpp


def _single(dtype):
    return np.dtype(dtype) in (np.dtype(np.float32), np.dtype(np.complex64))


def _wide(dtype):
    return np.complex128 if np.dtype(dtype).kind == 'c' else np.float64


def _randn(rng, shape, dtype):
    a = rng.randn(*shape)
    if np.dtype(dtype).kind == 'c':
        a = a + 1j * rng.randn(*shape)
    return a.astype(dtype)


def _dev(a):
    import torch
    return torch.from_numpy(np.ascontiguousarray(a)).cuda()


def _gamma(n, dtype):
    n = 2 * n + 4 if np.dtype(dtype).kind == 'c' else n + 1
    g = n * U32 / (1.0 - n * U32)
    assert g < 1e-3, 'the single-precision bound must stay below 1e-3 relative'
    return g


def _check_pass(got, ref, absref, n, dtype, what):
    """got against the float64 ref elementwise: gamma_n |.| |.| in single precision, 1e-10 in double."""
    got = np.asarray(got).astype(_wide(dtype))
    err = np.abs(got - ref)
    if _single(dtype):
        bound = _gamma(n, dtype) * absref + 1e-30
    else:
        bound = 1e-10 * max(float(np.max(absref)), 1e-300) + 0 * absref
    bad = err > bound
    assert not np.any(bad), '%s: %d elements over the bound, worst err %.3e (bound %.3e)' % (
        what, int(bad.sum()), float(err[bad].max()), float(bound[bad][np.argmax(err[bad])]))


def _check_iterated(got, ref64, ref32, dtype, what, scale=None):
    """An iterated result: 1e-10 relative in double; FLOOR_MULT times the single-precision floor.  ``scale``
    (default max|ref64|) is what the error is relative to."""
    got = np.asarray(got).astype(_wide(dtype))
    if scale is None:
        scale = max(float(np.max(np.abs(ref64))), 1e-30)
    err = float(np.max(np.abs(got - ref64)))
    if not _single(dtype):
        assert err <= 1e-10 * scale, '%s: rel err %.3e' % (what, err / scale)
        return
    floor = float(np.max(np.abs(np.asarray(ref32).astype(_wide(dtype)) - ref64)))
    bound = FLOOR_MULT * max(floor, U32 * scale)
    assert bound < 1e-3 * scale, '%s: floor %.3e too high for a 1e-3 bound' % (what, floor / scale)
    assert err <= bound, '%s: err %.3e > %g x floor %.3e (rel %.3e)' % (what, err, FLOOR_MULT, floor, err / scale)


def _taps_per_output(T, S, s):
    return T * (-(-S // s))


# ---- the geometry set --------------------------------------------------------------------------------
# (B, T, S, N, stride, padding)
GEOMS = [
    (1, 1, 33, 255, 1, 'SAME'),      # residual tile ends one sample short
    (2, 2, 33, 256, 1, 'VALID'),     # exactly one residual tile
    (3, 2, 17, 257, 2, 'SAME'),      # one sample into the second tile
    (2, 3, 33, 3001, 3, 'SAME'),     # a dozen tiles, C = 1011
    (1, 2, 33, 288, 1, 'VALID'),     # C = 256: exactly one coefficient tile
    (2, 1, 33, 289, 1, 'VALID'),     # C = 257
    (2, 2, 1, 300, 1, 'SAME'),       # S = 1
    (2, 2, 300, 300, 1, 'VALID'),    # S = N: C = 1
    (2, 2, 16, 1000, 16, 'VALID'),   # stride = S
    (2, 2, 9, 1000, 20, 'SAME'),     # stride > S: taps never overlap (dh = 0)
    (1, 2, 40, 2000, 300, 'SAME'),   # large stride under SAME
]
GEOM_IDS = ['B%dT%dS%dN%ds%d%s' % (B, T, S, N, s, p[0]) for B, T, S, N, s, p in GEOMS]


def test_geometry_set_covers_the_edges():
    Cs = [otm.geometry(S, N, s, p)[0] for _, _, S, N, s, p in GEOMS]
    assert {255, 256, 257} <= {g[3] for g in GEOMS}
    assert 256 in Cs and 257 in Cs and 1 in Cs
    assert any(g[2] == 1 for g in GEOMS) and any(g[4] == g[2] for g in GEOMS)
    assert any(g[4] > g[2] for g in GEOMS) and any(g[0] == 1 for g in GEOMS) and any(g[1] == 1 for g in GEOMS)
    for B, T, S, N, s, p in GEOMS:
        assert T * otm.geometry(S, N, s, p)[0] * N < 1.5e7


# ---- pure copies: temp2mat, coef2mat ---------------------------------------------------------------------
@pytest.mark.parametrize('dtype', DTYPES)
def test_temp2mat_coef2mat_bitwise(dtype):
    from decomp_amd import template_matching as tm
    rng = np.random.RandomState(1)
    for B, T, S, N, s, p in GEOMS:
        C, _ = otm.geometry(S, N, s, p)
        if T * C * N > 4e6 or B * T * S * N > 4e6:
            continue
        D = _randn(rng, (T, S), dtype)
        x = _randn(rng, (B, T, C), dtype)
        np.testing.assert_array_equal(tm._temp2mat(D, N, s, p), otm.temp2mat(D, N, s, p))
        np.testing.assert_array_equal(tm._coef2mat(x, N, S, s, p), otm.coef2mat(x, N, S, s, p))


# ---- predict ---------------------------------------------------------------------------------------------
@pytest.mark.parametrize('dtype', DTYPES)
@pytest.mark.parametrize('geom', GEOMS, ids=GEOM_IDS)
def test_predict(dtype, geom):
    from decomp_amd import template_matching as tm
    B, T, S, N, s, p = geom
    rng = np.random.RandomState(S + N + s)
    C, _ = otm.geometry(S, N, s, p)
    D = _randn(rng, (T, S), dtype)
    x = _randn(rng, (B, T, C), dtype)
    got = tm.predict(x, D, N, stride=s, padding=p)
    W = _wide(dtype)
    ref = otm.predict(x.astype(W), D.astype(W), N, s, p)
    absref = otm.predict(np.abs(x).astype(np.float64), np.abs(D).astype(np.float64), N, s, p)
    _check_pass(got, ref, absref, _taps_per_output(T, S, s), dtype, 'predict')


# ---- LDS and global-memory paths of both LASSO passes ------------------------------------------------------
def residual_lds(S, s, itemsize):
    """tm_launch_residual: the template plus the coefficients that reach a 256-sample tile."""
    span = (255 + S - 1) // s + 2
    return (S + span) * itemsize <= LDS_BYTES


def step_lds(S, s, itemsize):
    """tm_launch_step: conj(D) plus the samples read by a 256-coefficient tile."""
    span = 255 * s + S
    return (S + span) * itemsize <= LDS_BYTES


def _last_fit(fits, lo):
    v = lo
    while fits(v + 1):
        v += 1
    return v


def _path_cases():
    cases = []
    for dtype in DTYPES:
        sz = np.dtype(dtype).itemsize
        S_r = _last_fit(lambda S: residual_lds(S, 1, sz), 1)
        s_c = _last_fit(lambda s: step_lds(33, s, sz), 1)
        for S, lds in ((S_r, True), (S_r + 1, False)):
            # residual pass at stride 1, VALID: C = 300 coefficients over two coefficient tiles
            cases.append((dtype, 'residual', lds, (2, 1, S, S + 299, 1, 'VALID')))
        for s, lds in ((s_c, True), (s_c + 1, False)):
            # correlation pass, S = 33: C = 261 coefficients (two tiles)
            cases.append((dtype, 'step', lds, (2, 2, 33, 260 * s, s, 'SAME')))
    return cases


PATHS = _path_cases()


def test_path_boundaries_match_the_issue_table():
    firsts = {}
    for dtype, which, lds, g in PATHS:
        if not lds:
            firsts[(dtype, which)] = g[2] if which == 'residual' else g[4]
    assert firsts[('float32', 'step')] == 48 and firsts[('float32', 'residual')] == 6017
    for dt in ('float64', 'complex64'):
        assert firsts[(dt, 'step')] == 24 and firsts[(dt, 'residual')] == 2945
    assert firsts[('complex128', 'step')] == 12 and firsts[('complex128', 'residual')] == 1409


def _lasso_problem(rng, geom, dtype, density=0.05):
    B, T, S, N, s, p = geom
    C, _ = otm.geometry(S, N, s, p)
    D = _randn(rng, (T, S), dtype)
    D = (D / np.linalg.norm(D, axis=1, keepdims=True) * rng.uniform(0.5, 2.0, (T, 1))).astype(dtype)
    xt = _randn(rng, (B, T, C), dtype) * (rng.uniform(size=(B, T, C)) < density)
    W = _wide(dtype)
    y = (otm.predict(xt.astype(W), D.astype(W), N, s, p) + 0.1 * _randn(rng, (B, N), W)).astype(dtype)
    x0 = (0.1 * _randn(rng, (B, T, C), dtype)).astype(dtype)
    return y, D, x0


def _alpha(N):
    """alpha such that alpha N (the reference scales alpha by the signal length) leaves part of the
    coefficients non-zero: a solution thresholded to zero would not test the operator."""
    return 0.3 / N


def _nonzero(x):
    frac = float(np.mean(x != 0))
    assert frac > 0.01, 'the oracle solution is %.3f non-zero: the case does not test the operator' % frac


def _run_lasso(y, D, x0, alpha, s, p, method, maxiter, tol):
    from decomp_amd import template_matching as tm
    xd = _dev(x0.copy())
    it = tm._lasso(_dev(y), _dev(D), xd, alpha, s, p, method, maxiter, tol)
    return it, xd.cpu().numpy()


def _oracle_lasso(y, D, x0, alpha, s, p, method, maxiter, tol, wide=True, trace=None):
    W = _wide(y.dtype) if wide else y.dtype
    return otm.lasso_step(y.astype(W), D.astype(W), x0.astype(W), alpha, s, p, method, maxiter, tol,
                          trace=trace)


@pytest.mark.parametrize('dtype,which,lds,geom', PATHS,
                         ids=['%s-%s-%s' % (c[0], c[1], 'lds' if c[2] else 'global') for c in PATHS])
def test_lds_and_global_paths(dtype, which, lds, geom):
    B, T, S, N, s, p = geom
    sz = np.dtype(dtype).itemsize
    # each case lands on the side of the budget it is meant to, for the pass it is meant for
    assert (residual_lds(S, s, sz) if which == 'residual' else step_lds(S, s, sz)) == lds
    assert otm.geometry(S, N, s, p)[0] > 256
    from decomp_amd import template_matching as tm
    rng = np.random.RandomState(S + s)
    y, D, x0 = _lasso_problem(rng, geom, dtype)
    W = _wide(dtype)
    got = tm.predict(x0, D, N, stride=s, padding=p)
    ref = otm.predict(x0.astype(W), D.astype(W), N, s, p)
    absref = otm.predict(np.abs(x0).astype(np.float64), np.abs(D).astype(np.float64), N, s, p)
    _check_pass(got, ref, absref, _taps_per_output(T, S, s), dtype, 'predict')
    for method in ('ista', 'acc_ista'):
        it, x = _run_lasso(y, D, x0, _alpha(N), s, p, method, 3, 0.0)
        it64, x64 = _oracle_lasso(y, D, x0, _alpha(N), s, p, method, 3, 0.0)
        _, x32 = _oracle_lasso(y, D, x0, _alpha(N), s, p, method, 3, 0.0, wide=False)
        assert it == it64 == 2
        _nonzero(x64)
        _check_iterated(x, x64, x32, dtype, method)


# ---- structured LASSO: methods, iteration counts, the lagged stop test --------------------------------------
LASSO_GEOM = (2, 2, 17, 300, 1, 'SAME')      # 2 residual tiles; C = 316: 2 coefficient tiles per template


def _methods(dtype):
    base = ['ista', 'acc_ista', 'fista']
    return base + ([m + '_pos' for m in base] if np.dtype(dtype).kind == 'f' else [])


LASSO_CASES = [(d, m) for d in DTYPES for m in _methods(d)]


@pytest.mark.parametrize('dtype,method', LASSO_CASES)
def test_structured_lasso_iterations(dtype, method):
    """tol = 0 from a non-zero warm start: the returned iterate after 1, 2, 10, 11, 12 and 21 iterations
    (acc_ista hands back the iterate before the last on exhaustion, ista / fista the last)."""
    rng = np.random.RandomState(len(method) + np.dtype(dtype).itemsize)
    y, D, x0 = _lasso_problem(rng, LASSO_GEOM, dtype)
    _, _, _, N, s, p = LASSO_GEOM
    a = _alpha(N)
    for maxiter in (1, 2, 10, 11, 12, 21):
        it, x = _run_lasso(y, D, x0, a, s, p, method, maxiter, 0.0)
        it64, x64 = _oracle_lasso(y, D, x0, a, s, p, method, maxiter, 0.0)
        _, x32 = _oracle_lasso(y, D, x0, a, s, p, method, maxiter, 0.0, wide=False)
        assert it == it64 == maxiter - 1
        _nonzero(x64)
        _check_iterated(x, x64, x32, dtype, '%s x%d' % (method, maxiter))


def _row_norms(D, N, s, p):
    A = otm.temp2mat(D.astype(_wide(D.dtype)), N, s, p).reshape(-1, N)
    return np.sqrt(np.sum(np.abs(A) ** 2, axis=-1))


@pytest.mark.parametrize('dtype,method', [(d, m) for d in DTYPES for m in ('ista', 'acc_ista', 'fista')])
@pytest.mark.parametrize('stop_at', [10, 20])
def test_structured_lasso_stop(dtype, method, stop_at):
    """tol > 0: the stop test of iteration 10 (or 20, the last of 21 iterations) fires; the flag is read one
    iteration late, so the same `it` and the iterate of the check iteration must come back."""
    rng = np.random.RandomState(13)
    y, D, x0 = _lasso_problem(rng, LASSO_GEOM, dtype)
    _, _, _, N, s, p = LASSO_GEOM
    rho = _row_norms(D, N, s, p)
    a = _alpha(N)
    free = []
    _oracle_lasso(y, D, x0, a, s, p, method, 21, 0.0, trace=free)
    u = [float(np.max(d / rho)) for d in free]           # max |dx| (unscaled) at iterations 0, 10, 20
    hi = min(u[:stop_at // 10])
    assert u[stop_at // 10] < 0.9 * hi, u
    tol = float(np.sqrt(u[stop_at // 10] * hi))
    maxiter = 30 if stop_at == 10 else 21
    trace = []
    it64, x64 = _oracle_lasso(y, D, x0, a, s, p, method, maxiter, tol, trace=trace)
    assert it64 == stop_at
    _nonzero(x64)
    for v in trace:                                      # |dx'| - tol rho at every check: no knife edge
        assert abs(float(np.max(v))) > 1e-2 * tol * float(rho.min())
    _, x32 = _oracle_lasso(y, D, x0, a, s, p, method, maxiter, tol, wide=False)
    it, x = _run_lasso(y, D, x0, a, s, p, method, maxiter, tol)
    assert it == stop_at
    _check_iterated(x, x64, x32, dtype, '%s stop %d' % (method, stop_at))


# The single ista step is sized by 1/L: these pin the Gershgorin prepare (Toeplitz and boundary columns).
GERSH = [
    (2, 2, 33, 40, 1, 'SAME'),       # only boundary columns, most of them truncated by the signal ends
    (2, 2, 9, 600, 1, 'SAME'),       # mostly Toeplitz columns
    (2, 3, 9, 1000, 20, 'SAME'),     # stride > S: dh = 0
    (2, 2, 7, 600, 3, 'VALID'),      # Toeplitz columns at a stride that divides nothing
]


def _toeplitz_cols(S, N, s, p):
    C, Q = otm.geometry(S, N, s, p)
    dh = (S - 1) // s
    a = max(-((-Q) // s), 0)
    b = min((N - S + Q) // s, C - 1)
    return a + dh, b - dh


@pytest.mark.parametrize('dtype', DTYPES)
@pytest.mark.parametrize('geom', GERSH, ids=['boundary', 'toeplitz', 'dh0', 'valid-s3'])
def test_gershgorin_single_ista_step(dtype, geom):
    B, T, S, N, s, p = geom
    C, _ = otm.geometry(S, N, s, p)
    lo, hi = _toeplitz_cols(S, N, s, p)
    if geom == GERSH[0]:
        assert lo > hi
    elif geom == GERSH[1]:
        assert hi - lo + 1 > 0.9 * C
    rng = np.random.RandomState(S + N)
    y, D, x0 = _lasso_problem(rng, geom, dtype, density=0.2)
    for method in (['ista', 'ista_pos'] if np.dtype(dtype).kind == 'f' else ['ista']):
        it, x = _run_lasso(y, D, x0, _alpha(N), s, p, method, 1, 0.0)
        it64, x64 = _oracle_lasso(y, D, x0, _alpha(N), s, p, method, 1, 0.0)
        _, x32 = _oracle_lasso(y, D, x0, _alpha(N), s, p, method, 1, 0.0, wide=False)
        assert it == it64 == 0
        _nonzero(x64)
        _check_iterated(x, x64, x32, dtype, method)


# ---- the D step -----------------------------------------------------------------------------------------------
def _dstep_call(y, x, D, XXt, yX, s, p, acc_it):
    from decomp_amd import template_matching as tm
    Dd, XXd, yXd = _dev(D.copy()), _dev(XXt.copy()), _dev(yX.copy())
    diff = tm._dstep(_dev(y), _dev(x), Dd, XXd, yXd, s, p, acc_it)
    return diff, Dd.cpu().numpy(), XXd.cpu().numpy(), yXd.cpu().numpy()


def _check_dstep(dtype, geom, y, x, D, XXt_in, yX_in, acc_it, got):
    """got = (maxdiff, D, XXt, yX) of one dstep call against the oracle's statistics, running sums and update."""
    B, T, S, N, s, p = geom
    W = _wide(dtype)
    diff, Dg, XXg, yXg = got
    XXt, yX = otm.statistics(y.astype(W), x.astype(W), S, s, p)
    aXX, ayX = otm.statistics(np.abs(y).astype(np.float64), np.abs(x).astype(np.float64), S, s, p)
    C, _ = otm.geometry(S, N, s, p)
    n = B * C + 2
    if acc_it:
        XXt, yX = otm.accumulate(XXt_in.astype(W), yX_in.astype(W), XXt, yX, acc_it)
        aXX, ayX = np.abs(XXt_in) + aXX / acc_it, np.abs(yX_in) + ayX / acc_it
    _check_pass(XXg, XXt, aXX, n, dtype, 'XXt')
    _check_pass(yXg, yX, ayX, n, dtype, 'yX')
    D64, d64 = otm.d_update(D.astype(W), XXt, yX)
    # the update from the statistics in single precision: the floor of the whole step
    XX32, yX32 = otm.statistics(y, x, S, s, p)
    if acc_it:
        XX32, yX32 = otm.accumulate(XXt_in, yX_in, XX32, yX32, acc_it)
    D32, d32 = otm.d_update(D, XX32, yX32)
    _check_iterated(Dg, D64, D32, dtype, 'D')
    # max|D - D_new| cancels down to the rounding of D where D is (near) a fixed point: relative to |D|
    _check_iterated(np.array([diff]), np.array([d64]), np.array([d32]), dtype, 'maxdiff',
                    scale=float(np.max(np.abs(D64))))
    return XXt, yX, D64


@pytest.mark.parametrize('dtype', DTYPES)
@pytest.mark.parametrize('geom', GEOMS, ids=GEOM_IDS)
def test_dstep(dtype, geom):
    B, T, S, N, s, p = geom
    rng = np.random.RandomState(7 * S + N)
    C, _ = otm.geometry(S, N, s, p)
    D = _randn(rng, (T, S), dtype)
    D = (D / np.linalg.norm(D, axis=1, keepdims=True)).astype(dtype)
    x = (_randn(rng, (B, T, C), dtype) * (rng.uniform(size=(B, T, C)) < 0.3)).astype(dtype)
    y = _randn(rng, (B, N), dtype)
    TS = T * S
    XXt0, yX0 = np.zeros((TS, TS), dtype), np.zeros(TS, dtype)
    got = _dstep_call(y, x, D, XXt0, yX0, s, p, 0)
    _check_dstep(dtype, geom, y, x, D, XXt0, yX0, 0, got)


DSEQ = [(3, 2, 33, 300, 1, 'SAME'), (2, 2, 16, 700, 4, 'VALID'), (2, 1, 120, 120, 1, 'VALID')]


@pytest.mark.parametrize('dtype', DTYPES)
@pytest.mark.parametrize('geom', DSEQ, ids=['same-s1', 'valid-s4', 'S=N'])
def test_dstep_running_sums(dtype, geom):
    """acc_it = 1, 2, 3 with a different (y, x) at each call, as solve_minibatch makes them: the running sums
    XXt_sum += XXt / it, yX_sum += yX / it and the update of D from them."""
    B, T, S, N, s, p = geom
    rng = np.random.RandomState(11 + S)
    C, _ = otm.geometry(S, N, s, p)
    D = _randn(rng, (T, S), dtype)
    D = (D / np.linalg.norm(D, axis=1, keepdims=True)).astype(dtype)
    XXt, yX = np.zeros((T * S, T * S), dtype), np.zeros(T * S, dtype)
    for acc_it in (1, 2, 3):
        x = (_randn(rng, (B, T, C), dtype) * (rng.uniform(size=(B, T, C)) < 0.3)).astype(dtype)
        y = _randn(rng, (B, N), dtype)
        got = _dstep_call(y, x, D, XXt, yX, s, p, acc_it)
        _check_dstep(dtype, geom, y, x, D, XXt, yX, acc_it, got)
        # continue from the kernel's own sums and D, as the loop does
        _, D, XXt, yX = got


# ---- minibatch windows ------------------------------------------------------------------------------------------
WINDOWS = [   # (B, T, S, N, w, stride, padding)
    (2, 3, 10, 100, 30, 1, 'SAME'),
    (3, 2, 17, 700, 300, 1, 'VALID'),
    (2, 2, 5, 400, 120, 2, 'VALID'),
]


def _window_draws(B, N, w, C, cw):
    """Hand-made draws: duplicated rows, overlapping and repeated starts, m > B, the first and the last valid
    start (start + w <= N and start + cw <= C)."""
    last = min(N - w, C - cw)
    assert last > 3
    rows = np.array([0, 1, 0, B - 1, 0, 1, B - 1, 0, 0], np.int64)
    starts = np.array([0, last, 1, last, 0, last - 1, 2, last // 2, last // 2 + 1], np.int64)
    assert rows.size > B and np.all((rows >= 0) & (rows < B))
    assert np.all(starts >= 0) and np.all(starts + w <= N) and np.all(starts + cw <= C)
    return rows, starts


@pytest.mark.parametrize('dtype', DTYPES)
@pytest.mark.parametrize('geom', WINDOWS, ids=['same-s1', 'valid-s1', 'valid-s2'])
def test_gather_scatter_windows_bitwise(dtype, geom):
    import torch
    from decomp_amd import template_matching as tm
    B, T, S, N, w, s, p = geom
    C, cw = otm.coef_size(S, N, s, p), otm.coef_size(S, w, s, p)
    rows, starts = _window_draws(B, N, w, C, cw)
    m = rows.size
    rng = np.random.RandomState(w)
    y = _randn(rng, (B, N), dtype)
    x = _randn(rng, (B, T, C), dtype)
    yd, xd, ib, inn = _dev(y), _dev(x), _dev(rows), _dev(starts)
    pc = 0 if p == 'VALID' else 1
    yw = torch.empty((m, w), dtype=yd.dtype, device=yd.device)
    xw = torch.empty((m, T, cw), dtype=yd.dtype, device=yd.device)
    tm._call(yd, 'gather_windows', yd, xd, ib, inn, m, B, T, S, N, w, s, pc, yw, xw)
    np.testing.assert_array_equal(yw.cpu().numpy(), otm.gather_windows(y, rows, starts, w))
    np.testing.assert_array_equal(xw.cpu().numpy(), otm.gather_windows(x, rows, starts, cw))
    # new values for every window, written back: the last window that covers an element wins
    vals = _randn(rng, (m, T, cw), dtype)
    tm._call(yd, 'scatter_windows', _dev(vals), xd, ib, inn, m, B, T, S, N, w, s, pc)
    ref = otm.scatter_windows(x.copy(), rows, starts, cw, vals)
    np.testing.assert_array_equal(xd.cpu().numpy(), ref)


# ---- end to end: tm.solve against oracle.template_matching.solve ----------------------------------------------------
E2E_GEOM = (2, 2, 17, 300, 1, 'SAME')     # C = 316: past one tile of each pass
ALPHA_E2E = 0.002


def _e2e_methods(dtype):
    return ['acc_ista', 'fista', 'cd'] + (['ista_pos'] if np.dtype(dtype).kind == 'f' else [])


def _e2e_problem(dtype, N, seed):
    rng = np.random.RandomState(seed)
    B, T, S = 2, 2, 17
    C, _ = otm.geometry(S, N, 1, 'SAME')
    Dt = _randn(rng, (T, S), _wide(dtype))
    xt = _randn(rng, (B, T, C), _wide(dtype)) * (rng.uniform(size=(B, T, C)) < 0.03)
    y = otm.predict(xt, Dt, N, 1, 'SAME') + 0.1 * _randn(rng, (B, N), _wide(dtype))
    D0 = Dt + 0.5 * _randn(rng, (T, S), _wide(dtype))
    return y.astype(dtype), D0.astype(dtype)


def _e2e_tol(trace):
    """A tol at which the outer loop stops at the latest new running minimum of the tol = 0 trace (from the
    second iteration on), halfway (geometrically) between it and the minimum before it; (0, maxiter) when
    the trace sets no new minimum."""
    js = [i for i in range(1, len(trace)) if trace[i] < min(trace[:i])]
    if not js:
        return 0.0, len(trace) + 1
    j = js[-1]
    return float(np.sqrt(trace[j] * min(trace[:j]))), j + 1


@pytest.mark.parametrize('dtype', DTYPES)
@pytest.mark.parametrize('loop', ['batch', 'minibatch'])
def test_solve_end_to_end(dtype, loop):
    from decomp_amd import template_matching as tm
    N = 300 if loop == 'batch' else 700
    mb, w, seed = (None, None, 5) if loop == 'batch' else (4, 300, 6)
    if mb:
        r = np.random.RandomState(seed)
        draws = [otm.minibatch_index((2, N - w), mb, r) for _ in range(3)]
        assert all(len(set(rows.tolist())) < mb for rows, _ in draws)       # m > B: duplicated rows
    for method in _e2e_methods(dtype):
        y, D0 = _e2e_problem(dtype, N, seed + len(method))
        liter = 3 if method == 'cd' else 10
        kw = dict(stride=1, padding='SAME', minibatch=mb, size_of_minibatch=w, maxiter=6, lasso_method=method,
                  lasso_iter=liter, lasso_tol=1e-5, random_seed=seed)
        W = _wide(dtype)
        free = []
        otm.solve(y.astype(W), D0.astype(W), ALPHA_E2E, tol=0.0, trace=free, **kw)
        tol, it_want = _e2e_tol(free)
        it64, D64, x64 = otm.solve(y.astype(W), D0.astype(W), ALPHA_E2E, tol=tol, **kw)
        assert it64 == it_want
        it, D, x = tm.solve(y.copy(), D0.copy(), ALPHA_E2E, tol=tol, **kw)
        assert D.dtype == y.dtype and x.dtype == y.dtype
        if _single(dtype):
            knife = any(abs(t - tol) < 1e-2 * tol for t in free[:it_want])
            if it != it64:
                assert knife, (method, it, it64)
                continue
        assert it == it64, (method, it, it64)
        _, D32, x32 = otm.solve(y.copy(), D0.copy(), ALPHA_E2E, tol=tol, **kw)
        _check_iterated(D, D64, D32, dtype, '%s D' % method)
        _check_iterated(x, x64, x32, dtype, '%s x' % method)
