"""GPU parity of the coordinate-descent LASSO kernels (lasso_impl.hpp: cd_gram_kernel at every register tier,
cd_gram_wide_kernel, cd_mask_kernel) through decomp_amd.lasso.solve, against the float64 restatement in cd_ref.py
(pinned to oracle.lasso.solve by test_cd_ref_host.py).

Every width runs in two regimes, asserted from the reference so that a case cannot degenerate: DENSE starts from
x = ones, where every coordinate moves in the first sweep (the kernel's ballot loop runs its 64 rounds per slot), and
SPARSE starts from x = 0 and runs to its stop.  The stop tolerance of a sparse run is half the largest step of the
reference's first sweep, so the test fails at sweep 0 and is met at a later check sweep with a margin that rounding
cannot cross: the iteration count is then required to be exact in every dtype.

Bounds.  double: 1e-9 max(1, max|x_ref|), the bound of test_gpu_lasso.py's float64 oracle comparisons.  single: the
reference is run a second time in float32 / complex64; with e32 = err(that run, the double run) the bound is
min(2e-4, max(1e-5, 8 e32)) -- 8x because the GPU forms y An^H, the Gram matrix and g in MFMA-tile and split-K
summation orders, each a rounding of the size the reference's own single-precision run has; 1e-5 is the README's
parity goal, 2e-4 the bound of the existing float32 LASSO tests.  Each case records e32, bound and the GPU's error
(pytest -rA / record_property)."""
import numpy as np
import pytest

import cd_ref

pytestmark = pytest.mark.gpu

SINGLE = ('float32', 'complex64')
REAL = ('float32', 'float64')
ALL_DT = ('float32', 'float64', 'complex64', 'complex128')

# The launch ladder (lasso_impl.hpp): MAXM = 1, 2, 4, 8, 16, 32 slots of 64 columns, then the memory-resident form.
# Both sides of every edge, a ragged and a full last slot in every tier, 2624 = 41 slots (not a multiple of 8).
TIERS = [(1, 63, 64), (65, 128), (129, 200, 256), (257, 500, 512), (513, 1000, 1024), (1025, 1500, 2048),
         (2049, 2112, 2500, 2624)]
# (N, F) per width: N never a multiple of 4 (a partial last workgroup), K < F and K > F both occur in every tier
GEOM = {1: (9, 5), 63: (37, 96), 64: (5, 40), 65: (9, 96), 128: (37, 100), 129: (5, 300), 200: (37, 96),
        256: (9, 300), 257: (37, 96), 500: (5, 600), 512: (9, 96), 513: (9, 96), 1000: (5, 1100), 1024: (5, 200),
        1025: (5, 1100), 1500: (9, 96), 2048: (5, 200), 2049: (5, 96), 2112: (5, 2200), 2500: (5, 200),
        2624: (9, 96)}
# thinned dtype x prox cross by position in the tier: every tier sees the four dtypes and _pos, every K sees float32
# and a double dtype
COMBOS = [[('float32', 'cd'), ('float64', 'cd'), ('complex64', 'cd'), ('float32', 'cd_pos')],
          [('float32', 'cd'), ('complex128', 'cd'), ('float64', 'cd_pos')],
          [('float32', 'cd'), ('float64', 'cd'), ('complex64', 'cd')],
          [('float32', 'cd'), ('complex128', 'cd'), ('float32', 'cd_pos')]]
SWEEP = [(K, dt, method) for tier in TIERS for i, K in enumerate(tier) for dt, method in COMBOS[i]]
# the folded 1-D mask: one width per tier, every dtype
MASKED_K = (63, 128, 200, 500, 1000, 1500, 2500)
MASKED = [(K, dt, method) for K in MASKED_K
          for dt, method in [(d, 'cd') for d in ALL_DT] + [('float64', 'cd_pos')]]


def _randn(rng, cplx, *s):
    return (rng.randn(*s) + 1j * rng.randn(*s)) if cplx else rng.randn(*s)


def _problem(dt, N, F, K, method, seed, noise=0.05):
    """y = x_t A + noise; every row of x_t has min(8, K / 16) (at least one) non-zeros of modulus 0.5 + |randn|,
    non-negative for _pos."""
    rng = np.random.RandomState(seed)
    cplx = dt.startswith('complex')
    A = _randn(rng, cplx, K, F).astype(dt)
    planted = max(1, min(8, K // 16))
    where = np.argsort(rng.uniform(size=(N, K)), axis=1) < planted
    xt = _randn(rng, cplx, N, K)
    xt = where * (xt + 0.5 * xt / np.abs(xt))
    if method.endswith('_pos'):
        xt = np.abs(xt)
    y = (xt @ A + noise * _randn(rng, cplx, N, F)).astype(dt)
    return y, A


def _channel_mask(dt, F, seed):
    m = (np.random.RandomState(seed).uniform(size=F) > 0.3).astype(np.float32 if dt in SINGLE else np.float64)
    m[0] = 1.0
    return m


def _bound(dt, ref, solve_single):
    """-> (e32, bound); solve_single() is the reference's run in the working precision (single dtypes only)."""
    if dt not in SINGLE:
        return None, 1e-9
    e32 = cd_ref.err(solve_single().x, ref.x)
    return e32, min(2e-4, max(1e-5, 8.0 * e32))


def _check(record_property, tag, x, ref_x, e32, bound):
    e = cd_ref.err(x, ref_x)
    print('%s e32=%s bound=%.3g gpu_err=%.3g' % (tag, 'n/a' if e32 is None else '%.3g' % e32, bound, e))
    record_property(tag, {'e32': e32, 'bound': bound, 'gpu_err': e})
    assert e <= bound, (tag, e, bound, e32)


def _decisive(ref, bound):
    """Every stop decision of the reference run is at least 10x the case's error bound away from zero (the bound is
    relative to max(1, max|x|) in the caller's units, the stop quantity is in the scaled ones: x' = x s)."""
    margin = 10.0 * bound * max(1.0, float(np.max(np.abs(ref.x)))) * float(np.max(ref.s))
    assert all(abs(q) >= margin for q in ref.stop), (ref.stop, margin)


def _half_first_step(ref_fn, **kw):
    """Half the largest step of the reference's first sweep from x = 0, in the caller's units: a tolerance the first
    check sweep misses by a factor two."""
    return 0.5 * float(np.max(np.abs(ref_fn(tol=0.0, maxiter=1, **kw).x)))


def _dense_case(record_property, K, dt, method, mask):
    from decomp_amd import lasso
    N, F = GEOM[K]
    y, A = _problem(dt, N, F, K, method, seed=K)
    x0 = np.ones((N, K), dt)
    kw = dict(x=x0, tol=0.0, method=method, maxiter=4, mask=mask)
    ref = cd_ref.solve(y, A, 0.02, **kw)
    assert ref.moved[0] >= 0.9 and ref.it == 3, ref.moved
    e32, bound = _bound(dt, ref, lambda: cd_ref.solve(y, A, 0.02, dtype=dt, **kw))
    it, x = lasso.solve(y.copy(), A.copy(), 0.02, x=x0.copy(), tol=0.0, method=method, maxiter=4,
                        mask=None if mask is None else mask.copy())
    assert it == 3 and x.dtype == y.dtype and x.shape == (N, K)     # tol = 0 never stops: |0| - 0 < 0 is false
    _check(record_property, 'dense K=%d %s %s' % (K, dt, method), x, ref.x, e32, bound)


def _sparse_alpha(K, F):
    """The threshold in units of the planted coefficients' scale: the interference of the other planted atoms on a
    coordinate has deviation ~ sqrt(8 / F) there, and the wider the dictionary the more coordinates compete."""
    if K == 1:
        return 0.01         # (every row's only coefficient has to survive the threshold)
    return 0.1 if K < F else 0.3


def _sparse_case(record_property, K, dt, method, mask):
    from decomp_amd import lasso
    N, F = GEOM[K]
    y, A = _problem(dt, N, F, K, method, seed=1000 + K)
    alpha = _sparse_alpha(K, F)
    tol = _half_first_step(cd_ref.solve, y=y, A=A, alpha=alpha, method=method, mask=mask)
    kw = dict(tol=tol, method=method, maxiter=40, mask=mask)
    ref = cd_ref.solve(y, A, alpha, **kw)
    share = np.count_nonzero(ref.x) / float(ref.x.size)
    assert 0.002 <= share <= max(0.10, 1.0 / K), share          # (one non-zero per row of a K < 10 problem is > 10 %)
    assert np.all(np.count_nonzero(ref.x, axis=-1) >= 1)
    assert ref.it in (10, 20), ref.it
    e32, bound = _bound(dt, ref, lambda: cd_ref.solve(y, A, alpha, dtype=dt, **kw))
    _decisive(ref, bound)
    it, x = lasso.solve(y.copy(), A.copy(), alpha, tol=tol, method=method, maxiter=40,
                        mask=None if mask is None else mask.copy())
    assert it == ref.it, (it, ref.it)
    _check(record_property, 'sparse K=%d %s %s' % (K, dt, method), x, ref.x, e32, bound)


@pytest.mark.parametrize('K,dt,method', SWEEP)
def test_tier_sweep_dense_start(record_property, K, dt, method):
    """x = ones: every coordinate moves in the first sweep, four sweeps, tol = 0."""
    _dense_case(record_property, K, dt, method, None)


@pytest.mark.parametrize('K,dt,method', SWEEP)
def test_tier_sweep_sparse_to_stop(record_property, K, dt, method):
    """x = 0, a sparse solution, run to its stop at a later check sweep: codes and the exact iteration count."""
    _sparse_case(record_property, K, dt, method, None)


@pytest.mark.parametrize('K,dt,method', MASKED)
def test_channel_mask_dense_start(record_property, K, dt, method):
    """A 0/1 channel mask that removes ~30 % of the channels (folded into y and A: the Gram form)."""
    _dense_case(record_property, K, dt, method, _channel_mask(dt, GEOM[K][1], K))


@pytest.mark.parametrize('K,dt,method', MASKED)
def test_channel_mask_sparse_to_stop(record_property, K, dt, method):
    _sparse_case(record_property, K, dt, method, _channel_mask(dt, GEOM[K][1], K))


@pytest.mark.parametrize('K', [1000, 2112])
@pytest.mark.parametrize('dt', ['float32', 'float64'])
def test_maxiter_edges_register_and_wide_form(record_property, K, dt):
    """maxiter = 1 (the check sweep alone), 10 (+ nine), 11 (a second check sweep that is the last one), 12: the
    launch bookkeeping of the ten-sweep rounds at a 16-slot and at a memory-resident width.  tol = 0, so the count
    is maxiter - 1 and the codes are the reference's after exactly maxiter sweeps."""
    from decomp_amd import lasso
    N, F, alpha = 5, 96, 0.02       # K >> F from x = ones: slow to settle, ~98 % of the coordinates move per sweep
    y, A = _problem(dt, N, F, K, 'cd', seed=2000 + K)
    x0 = np.ones((N, K), dt)
    kw = dict(x=x0, tol=0.0, maxiter=12, keep=(0, 9, 10, 11))
    ref = cd_ref.solve(y, A, alpha, **kw)
    ref32 = cd_ref.solve(y, A, alpha, dtype=dt, **kw) if dt in SINGLE else None
    # successive sweeps still differ by more than any bound used here, so one sweep too many or too few is seen
    assert min(cd_ref.err(ref.after[a], ref.after[b]) for a, b in ((0, 9), (9, 10), (10, 11))) > 10 * 2e-4
    for maxiter in (1, 10, 11, 12):
        want = ref.after[maxiter - 1]
        e32 = None if ref32 is None else cd_ref.err(ref32.after[maxiter - 1], want)
        bound = 1e-9 if e32 is None else min(2e-4, max(1e-5, 8.0 * e32))
        it, x = lasso.solve(y.copy(), A.copy(), alpha, x=x0.copy(), tol=0.0, method='cd', maxiter=maxiter)
        assert it == maxiter - 1
        _check(record_property, 'maxiter=%d K=%d %s' % (maxiter, K, dt), x, want, e32, bound)


@pytest.mark.parametrize('K', [200, 2112])
@pytest.mark.parametrize('dt', ['float32', 'float64'])
def test_tol_zero_never_stops_at_a_fixed_point(dt, K):
    """y = 0 from x = 0: every step of every sweep is a zero step, and with tol = 0 the reference still does not stop
    (|0| - 0 < 0 is false): the count is maxiter - 1.  With any tol > 0 the same problem stops at sweep 0."""
    from decomp_amd import lasso
    y, A = _problem(dt, 9, 96, K, 'cd', seed=K)
    y[:] = 0
    ref = cd_ref.solve(y, A, 0.1, tol=0.0, maxiter=25)
    assert ref.it == 24 and ref.moved == [0.0] * 25
    it, x = lasso.solve(y.copy(), A.copy(), 0.1, tol=0.0, method='cd', maxiter=25)
    assert it == 24 and not x.any()
    it, x = lasso.solve(y.copy(), A.copy(), 0.1, tol=1e-6, method='cd', maxiter=25)
    assert it == cd_ref.solve(y, A, 0.1, tol=1e-6, maxiter=25).it == 0 and not x.any()


# ---- many workgroups and the device-side `cond` ----------------------------------------------------------------
MANY_N, MANY_K, MANY_F = 4099, 200, 96          # 1025 workgroups, the last one with a single row


@pytest.mark.parametrize('dt', ['float32', 'float64'])
def test_many_blocks_ordinary_rows(record_property, dt):
    from decomp_amd import lasso
    y, A = _problem(dt, MANY_N, MANY_F, MANY_K, 'cd', seed=31)
    alpha = _sparse_alpha(MANY_K, MANY_F)
    tol = _half_first_step(cd_ref.solve, y=y, A=A, alpha=alpha)
    ref = cd_ref.solve(y, A, alpha, tol=tol, maxiter=40)
    assert ref.it in (10, 20) and np.all(np.count_nonzero(ref.x, axis=-1) >= 1)
    e32, bound = _bound(dt, ref, lambda: cd_ref.solve(y, A, alpha, tol=tol, maxiter=40, dtype=dt))
    _decisive(ref, bound)
    it, x = lasso.solve(y.copy(), A.copy(), alpha, tol=tol, method='cd', maxiter=40)
    assert it == ref.it
    _check(record_property, 'many blocks %s' % dt, x, ref.x, e32, bound)


@pytest.mark.parametrize('dt', ['float32', 'float64'])
@pytest.mark.parametrize('live', [MANY_N - 1, 1234])
def test_many_blocks_one_wave_raises_the_flag(record_property, dt, live):
    """Every row but one is y = 0: it meets the test at sweep 0 with x = 0.  The one live wave (in the one-row tail
    workgroup, or in the middle of the grid) alone must raise the flag, and the nine sweeps behind the check sweep
    must then run -- the live row's codes are the reference's after sweeps 0 .. 10."""
    from decomp_amd import lasso
    y, A = _problem(dt, MANY_N, MANY_F, MANY_K, 'cd', seed=32)
    keep = y[live].copy()
    y[:] = 0
    y[live] = keep
    alpha = _sparse_alpha(MANY_K, MANY_F)
    one = y[live:live + 1]                      # rows are independent: the reference of the live row alone
    tol = _half_first_step(cd_ref.solve, y=one, A=A, alpha=alpha)
    ref = cd_ref.solve(one, A, alpha, tol=tol, maxiter=40, keep=(0,))
    assert ref.it == 10 and np.count_nonzero(ref.x) >= 1
    e32, bound = _bound(dt, ref, lambda: cd_ref.solve(one, A, alpha, tol=tol, maxiter=40, dtype=dt))
    _decisive(ref, bound)
    assert cd_ref.err(ref.after[0], ref.x) > 10 * bound        # stopping after the check sweep would be seen
    it, x = lasso.solve(y.copy(), A.copy(), alpha, tol=tol, method='cd', maxiter=40)
    assert it == 10
    assert not np.delete(x, live, axis=0).any()
    _check(record_property, 'one live row %d %s' % (live, dt), x[live:live + 1], ref.x, e32, bound)


@pytest.mark.parametrize('dt', ['float32', 'float64'])
def test_many_blocks_all_rows_meet_the_test_at_sweep_0(record_property, dt):
    """A warm start near, not at, the fixed point and a loose tol: every row meets the test in sweep 0, so it == 0
    and the codes are the reference's after ONE sweep.  The reference's codes after ten sweeps differ from those by
    more than the bound (asserted from the reference), so a follow-up launch that ran anyway is caught."""
    from decomp_amd import lasso
    y, A = _problem(dt, MANY_N, MANY_F, MANY_K, 'cd', seed=33)
    alpha = _sparse_alpha(MANY_K, MANY_F)
    fixed = cd_ref.solve(y, A, alpha, tol=0.0, maxiter=30).x
    rng = np.random.RandomState(34)
    x0 = (fixed + 0.05 * rng.randn(*fixed.shape) * (fixed != 0)).astype(dt)
    tol = 1.0
    ref = cd_ref.solve(y, A, alpha, x=x0, tol=tol, maxiter=40)
    assert ref.it == 0 and ref.moved[0] > 0.0
    e32, bound = _bound(dt, ref, lambda: cd_ref.solve(y, A, alpha, x=x0, tol=tol, maxiter=40, dtype=dt))
    _decisive(ref, bound)
    ten = cd_ref.solve(y, A, alpha, x=x0, tol=0.0, maxiter=10)
    assert cd_ref.err(ten.x, ref.x) > 10 * bound
    it, x = lasso.solve(y.copy(), A.copy(), alpha, x=x0.copy(), tol=tol, method='cd', maxiter=40)
    assert it == 0
    _check(record_property, 'met at sweep 0 %s' % dt, x, ref.x, e32, bound)


# ---- register form against the memory-resident form ------------------------------------------------------------
@pytest.mark.parametrize('K', [1025, 2048])
@pytest.mark.parametrize('method', ['cd', 'cd_pos'])
def test_wide_form_equals_register_form_bitwise_over_the_knob_range(monkeypatch, K, method):
    """DCP_CD_REGISTER_LIMIT (a test knob, clamped to 1024 .. 2048) sends 1025 .. 2048 atoms to cd_gram_wide_kernel:
    at both ends of that range, with and without the positive prox, from a sparse and from a dense start, the wide
    form reproduces the 32-slot register form bit for bit in every dtype."""
    import decomp_amd as decomp
    for dt in (REAL if method == 'cd_pos' else ALL_DT):
        y, A = _problem(dt, 37, 96, K, method, seed=K + len(dt))
        runs = [dict(tol=1e-5, maxiter=21), dict(x=np.ones((37, K), dt), tol=0.0, maxiter=3)]
        for kw in runs:
            alpha = 0.05 if 'x' not in kw else 0.02
            monkeypatch.delenv('DCP_CD_REGISTER_LIMIT', raising=False)
            it_a, x_a = decomp.lasso.solve(y.copy(), A.copy(), alpha, method=method, **kw)
            monkeypatch.setenv('DCP_CD_REGISTER_LIMIT', '1024')
            it_b, x_b = decomp.lasso.solve(y.copy(), A.copy(), alpha, method=method, **kw)
            monkeypatch.delenv('DCP_CD_REGISTER_LIMIT', raising=False)
            assert it_a == it_b, (dt, kw['maxiter'])
            assert np.array_equal(x_a, x_b), (dt, kw['maxiter'])
            assert np.count_nonzero(x_a) > 0


# ---- the 2-D-mask kernel ------------------------------------------------------------------------------------------
MASK_N = 11
MASK2D = [(F, K, dt, method) for F in (255, 256, 257, 600, 1100) for K in (7, 40, 64)
          for dt, method in [(d, 'cd') for d in ALL_DT] + [(d, 'cd_pos') for d in REAL]]


def _mask2d(dt, F, seed):
    """~30 % zeros, row 0 fully observed, row 1 with a single observed channel (the last one: beyond the first 256
    whenever F is)."""
    m = (np.random.RandomState(seed).uniform(size=(MASK_N, F)) > 0.3).astype(np.float32 if dt in SINGLE else np.float64)
    m[0] = 1.0
    m[1] = 0.0
    m[1, F - 1] = 1.0
    return m


@pytest.mark.parametrize('F,K,dt,method', MASK2D)
def test_mask2d_kernel(record_property, F, K, dt, method):
    """cd_mask_kernel with F on both sides of its 256-thread stride: 12 sweeps with tol = 0, maxiter = 1 / 10 / 11
    (the last / check_last bookkeeping of the solver's launch loop) and a run whose stop fires at sweep 10.  The
    reference's x_k A_k term is unmasked (oracle/lasso.py QUIRK); with 30 % of the channels masked a sweep that masks
    it is far outside the bound."""
    from decomp_amd import lasso
    from oracle import lasso as olasso
    y, A = _problem(dt, MASK_N, F, K, method, seed=F + K)
    mask = _mask2d(dt, F, F * K)
    alpha = 0.1
    tag = 'mask2d F=%d K=%d %s %s' % (F, K, dt, method)

    def bound_for(ref_x, single_x):
        if dt not in SINGLE:
            return None, 1e-9
        e32 = cd_ref.err(single_x, ref_x)
        return e32, min(2e-4, max(1e-5, 8.0 * e32))

    keep = (0, 9, 10)
    ref = cd_ref.solve_masked(y, A, alpha, mask, tol=0.0, method=method, maxiter=12, keep=keep)
    ref32 = cd_ref.solve_masked(y, A, alpha, mask, tol=0.0, method=method, maxiter=12, keep=keep,
                                dtype=dt) if dt in SINGLE else None
    if dt not in SINGLE and K <= 40:        # the as-written sweep itself, where it is cheap
        ito, xo = olasso.solve(y.copy(), A.copy(), alpha, tol=0.0, method=method, maxiter=12, mask=mask.copy())
        assert ito == 11 and cd_ref.err(ref.x, xo) <= 1e-12
    assert np.count_nonzero(ref.x) > 0 and cd_ref.err(ref.after[0], ref.after[9]) > 10 * 2e-4
    for maxiter in (12, 1, 10, 11):
        want = ref.x if maxiter == 12 else ref.after[maxiter - 1]
        e32, bound = bound_for(want, None if ref32 is None else
                               (ref32.x if maxiter == 12 else ref32.after[maxiter - 1]))
        it, x = lasso.solve(y.copy(), A.copy(), alpha, tol=0.0, method=method, maxiter=maxiter, mask=mask.copy())
        assert it == maxiter - 1 and x.dtype == y.dtype
        _check(record_property, '%s maxiter=%d' % (tag, maxiter), x, want, e32, bound)

    tol = _half_first_step(cd_ref.solve_masked, y=y, A=A, alpha=alpha, mask=mask, method=method)
    stop = cd_ref.solve_masked(y, A, alpha, mask, tol=tol, method=method, maxiter=40)
    assert stop.it == 10
    e32, bound = bound_for(stop.x, None if dt not in SINGLE else
                           cd_ref.solve_masked(y, A, alpha, mask, tol=tol, method=method, maxiter=40, dtype=dt).x)
    _decisive(stop, bound)
    it, x = lasso.solve(y.copy(), A.copy(), alpha, tol=tol, method=method, maxiter=40, mask=mask.copy())
    assert it == 10
    _check(record_property, '%s stop' % tag, x, stop.x, e32, bound)
