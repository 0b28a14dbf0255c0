"""GPU: template learning with greedy codes -- the dictionary step on event lists (dcp_tm_dstep_events_*) against the
dense one (dcp_tm_dstep_*), bit for bit, and against the float64 oracle; template_matching.solve with lasso_method
'omp', 'mp', 'mp_pos' against the same loop written out with the public coders and the dense step, bit for bit; and
its result on the planted problems of tm_learn_ref against the NumPy loop.

Bounds against the oracle (those of test_gpu_template_kernels.py, restated): the statistics elementwise within
gamma_n sum|terms| in single precision (u = 2^-24, n = B C + 2 terms, a complex product counted as two real ones) and
1e-10 max sum|terms| in double; D and max|dD| within FLOOR_MULT times what the oracle's own update shows in single
precision against double (never below u), 1e-10 in double."""
import numpy as np
import pytest

import tm_learn_ref as ref
from oracle import template_matching as otm

pytestmark = pytest.mark.gpu

DTYPES = ['float32', 'float64', 'complex64', 'complex128']
U32 = 2.0 ** -24
FLOOR_MULT = 16.0


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


def _same_bits(a, b):
    a, b = np.ascontiguousarray(a), np.ascontiguousarray(b)
    return a.dtype == b.dtype and a.shape == b.shape and a.tobytes() == b.tobytes()


# ---- the oracle bounds ------------------------------------------------------------------------------------------------
def _gamma(n, dtype):
    n = 2 * n + 4 if np.dtype(dtype).kind == 'c' else n + 1
    g = n * U32 / (1.0 - n * U32)
    assert g < 1e-3, 'the single-precision bound must stay below 1e-3 relative'
    return g


def _check_pass(got, want, absref, n, dtype, what):
    got = np.asarray(got).astype(_wide(dtype))
    err = np.abs(got - want)
    if _single(dtype):
        bound = _gamma(n, dtype) * absref + 1e-30
    else:
        bound = 1e-10 * max(float(np.max(absref)), 1e-300) + 0 * absref
    bad = err > bound
    assert not np.any(bad), '%s: %d elements over the bound, worst err %.3e' % (what, int(bad.sum()),
                                                                                  float(err[bad].max()))


def _check_iterated(got, ref64, ref32, dtype, what, scale=None):
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
    assert err <= bound, '%s: err %.3e > %g x floor %.3e' % (what, err, FLOOR_MULT, floor)


def _check_oracle(dtype, geom, y, x, D, XXt_in, yX_in, acc_it, got):
    B, T, S, N, s, p = geom
    W = _wide(dtype)
    diff, Dg, XXg, yXg = got
    XXt, yX = otm.statistics(y.astype(W), x.astype(W), S, s, p)
    aXX, ayX = otm.statistics(np.abs(y).astype(np.float64), np.abs(x).astype(np.float64), S, s, p)
    n = B * otm.geometry(S, N, s, p)[0] + 2
    XX32, yX32 = otm.statistics(y, x, S, s, p)
    if acc_it:
        XXt, yX = otm.accumulate(XXt_in.astype(W), yX_in.astype(W), XXt, yX, acc_it)
        aXX, ayX = np.abs(XXt_in) + aXX / acc_it, np.abs(yX_in) + ayX / acc_it
        XX32, yX32 = otm.accumulate(XXt_in, yX_in, XX32, yX32, acc_it)
    _check_pass(XXg, XXt, aXX, n, dtype, 'XXt')
    _check_pass(yXg, yX, ayX, n, dtype, 'yX')
    D64, d64 = otm.d_update(D.astype(W), XXt, yX)
    D32, d32 = otm.d_update(D, XX32, yX32)
    _check_iterated(Dg, D64, D32, dtype, 'D')
    _check_iterated(np.array([diff]), np.array([d64]), np.array([d32]), dtype, 'maxdiff',
                    scale=float(np.max(np.abs(D64))))


# ---- geometry, restated from TmGeom ----------------------------------------------------------------------------------
# (B, T, S, N, stride, padding): each the smallest shape that reaches a distinct path of the event kernels
GEOMS = [
    (3, 2, 33, 300, 1, 'SAME'),      # the general case
    (2, 2, 16, 700, 4, 'VALID'),     # stride > 1
    (2, 2, 4, 100, 6, 'SAME'),       # stride > S: dh = 0
    (2, 1, 120, 120, 1, 'VALID'),    # C = 1
    (2, 3, 120, 400, 1, 'SAME'),     # T nd = 717 cells: three passes of the 256 threads
    (1, 2, 300, 900, 1, 'SAME'),     # S > 256: two passes in the yX kernel
    (2, 2, 12, 12, 2, 'SAME'),       # the core is empty for some lags: every term is an edge term there
]
GEOM_IDS = ['general', 'stride4', 'dh0', 'C1', 'cells717', 'S300', 'empty-core']


def _window(geom, k, d):
    B, T, S, N, s, p = geom
    C, Q = otm.geometry(S, N, s, p)
    return max(-((k - Q) // s), 0, -d), min((N - 1 + Q - k) // s, C - 1, C - 1 - d)


def _core(geom, d):
    """(cl, ch) of TmGeom::core before an empty core is re-labelled: the intersection of the windows of all taps."""
    S = geom[2]
    return _window(geom, 0, d)[0], _window(geom, S - 1, d)[1]


def _lags(geom):
    dh = (geom[2] - 1) // geom[4]
    return range(-dh, dh + 1)


def test_geometries_reach_their_paths():
    C = [otm.geometry(S, N, s, p)[0] for _, _, S, N, s, p in GEOMS]
    nd = [2 * ((S - 1) // s) + 1 for _, _, S, N, s, p in GEOMS]
    assert nd[2] == 1 and C[3] == 1 and GEOMS[4][1] * nd[4] == 717 and GEOMS[5][2] > 256
    assert C[0] > 256 and C[4] > 256 and C[5] > 256              # a list of more than 256 events is possible
    assert any(cl > ch for cl, ch in (_core(GEOMS[6], d) for d in _lags(GEOMS[6])))
    for g in GEOMS[:3] + GEOMS[4:6]:     # (with C = 1 only lag 0 has a core)
        assert all(cl <= ch for cl, ch in (_core(g, d) for d in _lags(g)))


# ---- hand-made codes ---------------------------------------------------------------------------------------------------
def _values(rng, n, dtype):
    """n non-zero values, magnitudes in [0.5, 1.5]."""
    v = (0.5 + rng.rand(n)) * rng.choice([-1.0, 1.0], n)
    if np.dtype(dtype).kind == 'c':
        v = v * np.exp(2j * np.pi * rng.rand(n))
    return v.astype(dtype)


def _put(x, b, t, cs, rng):
    cs = np.unique([c for c in cs if 0 <= c < x.shape[2]]).astype(np.int64)
    x[b, t, cs] = _values(rng, cs.size, x.dtype)


def _sparse(rng, shape, dtype, density):
    return (_randn(rng, shape, dtype) * (rng.uniform(size=shape) < density)).astype(dtype)


def _patterns(geom, dtype, rng):
    """[(name, x, the max_events to run)]"""
    B, T, S, N, s, p = geom
    C, _ = otm.geometry(S, N, s, p)
    shape = (B, T, C)
    out = []
    # rows with no event, one row with a single event
    x = np.zeros(shape, dtype)
    _put(x, B - 1, T - 1, [C // 2], rng)
    out.append(('one-event', x, [1, 3]))
    # events exactly at cl(d) and ch(d), one inside and one outside each; the partner rows are half full (with one
    # template the partners c + d are put into the row itself)
    lags = list(_lags(geom))
    if len(lags) > 9:
        lags = lags[:3] + lags[len(lags) // 2 - 1:len(lags) // 2 + 2] + lags[-3:]
    marks = []
    for d in lags:
        cl, ch = _core(geom, d)
        marks += [cl - 1, cl, cl + 1, ch - 1, ch, ch + 1]
        if T == 1:
            marks += [cl + d, ch + d]
    x = _sparse(rng, shape, dtype, 0.5)
    for b in range(B):
        x[b, b % T] = 0
        _put(x, b, b % T, marks, rng)
    n_marks = int(np.count_nonzero(x[0, 0]))
    out.append(('core-bounds', x, [1, n_marks, C]))
    # events in the head and tail edge regions of lag 0 only
    cl, ch = _core(geom, 0)
    x = np.zeros(shape, dtype)
    for b in range(B):
        for t in range(T):
            _put(x, b, t, list(range(0, cl)) + list(range(ch + 1, C)), rng)
    out.append(('edges-only', x, [2, C]))
    # the chunk boundaries of the compaction (64 lanes) and of the staging (256 events)
    x = np.zeros(shape, dtype)
    for b in range(B):
        for t in range(T):
            _put(x, b, t, [0, 63, 64, 255, 256, C - 1], rng)
    out.append(('chunk-bounds', x, [4, 6]))
    # a row with more than 256 events (every coefficient), listed and overflowing, among sparse rows
    x = _sparse(rng, shape, dtype, 0.05)
    x[0, 0] = _values(rng, C, dtype)
    out.append(('long-row', x, [C, 256, 8]))
    # -0.0 is a zero: no event
    x = _sparse(rng, shape, dtype, 0.1)
    flat = x.reshape(-1)
    idx = rng.choice(flat.size, max(flat.size // 10, 1), replace=False)
    flat[idx] = -0.0
    if np.dtype(dtype).kind == 'c':
        flat[idx[::2]] = complex(-0.0, 0.0)
        flat[idx[1::2]] = complex(0.0, -0.0)
    assert np.any(np.signbit(flat.real) & (flat == 0))
    nnz = int(np.count_nonzero(x.reshape(B * T, C), axis=1).max())
    out.append(('minus-zero', x, [max(nnz, 1), C]))
    # 30 % dense: every row overflows max_events = 1, none overflows max_events = C
    out.append(('dense30', _sparse(rng, shape, dtype, 0.3), [1, C]))
    return out


def _problem(geom, dtype, rng):
    B, T, S, N, s, p = geom
    D = _randn(rng, (T, S), dtype)
    D = (D / np.linalg.norm(D, axis=1, keepdims=True)).astype(dtype)
    return _randn(rng, (B, N), dtype), D


def _step(yd, xd, D, XXt, yX, s, p, acc_it, max_events=None):
    """One dictionary step from host copies of D and the sums: (maxdiff, D, XXt, yX) as NumPy."""
    from decomp_amd import template_matching as tm
    Dd, XXd, yXd = _dev(D.copy()), _dev(XXt.copy()), _dev(yX.copy())
    if max_events is None:
        diff = tm._dstep(yd, xd, Dd, XXd, yXd, s, p, acc_it)
    else:
        diff = tm._dstep_events(yd, xd, Dd, XXd, yXd, s, p, acc_it, max_events)
    return diff, Dd.cpu().numpy(), XXd.cpu().numpy(), yXd.cpu().numpy()


def _assert_same(a, b, what):
    bad = ['%s differs in %d elements (by up to %.3g)' % (name, int(np.sum(u != v)), float(np.max(np.abs(u - v))))
           for name, u, v in zip(('XXt', 'yX', 'D'), a[2:] + a[1:2], b[2:] + b[1:2]) if not _same_bits(u, v)]
    if a[0] != b[0]:
        bad.append('maxdiff %r != %r' % (a[0], b[0]))
    assert not bad, '%s: %s' % (what, '; '.join(bad))


@pytest.mark.parametrize('dtype', DTYPES)
@pytest.mark.parametrize('geom', GEOMS, ids=GEOM_IDS)
def test_event_step_equals_dense_step_bitwise(geom, dtype):
    """acc_it = 0 on every hand-made code: XXt, yX, D and maxdiff of the event step are the dense step's bits for every
    max_events, two calls give the same bits, and the result lies within the oracle's bounds."""
    B, T, S, N, s, p = geom
    rng = np.random.RandomState(S + N + s)
    y, D = _problem(geom, dtype, rng)
    yd = _dev(y)
    zXX, zyX = np.zeros((T * S, T * S), dtype), np.zeros(T * S, dtype)
    for name, x, caps in _patterns(geom, dtype, rng):
        xd = _dev(x)
        dense = _step(yd, xd, D, zXX, zyX, s, p, 0)
        assert np.all(np.isfinite(dense[2])) and np.isfinite(dense[0])
        for cap in caps:
            got = _step(yd, xd, D, zXX, zyX, s, p, 0, max_events=cap)
            _assert_same(got, dense, '%s, max_events %d' % (name, cap))
        again = _step(yd, xd, D, zXX, zyX, s, p, 0, max_events=caps[0])
        _assert_same(again, dense, '%s, second call' % name)
        _check_oracle(dtype, geom, y, x, D, zXX, zyX, 0, got)


@pytest.mark.parametrize('dtype', DTYPES)
@pytest.mark.parametrize('geom', GEOMS, ids=GEOM_IDS)
def test_event_step_running_sums_bitwise(geom, dtype):
    """acc_it = 1, 2, 3 with another (y, x) at each call, continued from the kernel's own sums and D as the minibatch
    loop does: the same bits as the dense step at every call, within the oracle's bounds."""
    B, T, S, N, s, p = geom
    C, _ = otm.geometry(S, N, s, p)
    rng = np.random.RandomState(11 + S)
    _, D = _problem(geom, dtype, rng)
    XXt, yX = np.zeros((T * S, T * S), dtype), np.zeros(T * S, dtype)
    for acc_it, (density, cap) in zip((1, 2, 3), ((0.02, 8), (0.3, 2), (0.05, C))):
        x = _sparse(rng, (B, T, C), dtype, density)
        y = _randn(rng, (B, N), dtype)
        yd, xd = _dev(y), _dev(x)
        dense = _step(yd, xd, D, XXt, yX, s, p, acc_it)
        got = _step(yd, xd, D, XXt, yX, s, p, acc_it, max_events=cap)
        _assert_same(got, dense, 'acc_it %d' % acc_it)
        _check_oracle(dtype, geom, y, x, D, XXt, yX, acc_it, got)
        _, D, XXt, yX = got


def test_event_step_rejects_bad_arguments():
    import ctypes
    import torch
    from decomp_amd import _arrays
    t = torch.zeros(64, device='cuda')
    lib, h = _arrays.lib_handle(t)
    p = _arrays.ptr(t)
    out = ctypes.c_double(0.0)
    fn = lib.dcp_tm_dstep_events_f32
    assert fn(h, p, p, p, p, p, 1, 1, 4, 8, 1, 1, 0, 0, ctypes.byref(out)) == -1          # max_events < 1
    assert fn(h, p, p, p, p, p, 1, 1, 4, 8, 1, 1, -1, 1, ctypes.byref(out)) == -1         # acc_it < 0
    assert fn(h, p, p, p, p, p, 1, 1, 9, 8, 1, 1, 0, 1, ctypes.byref(out)) == -1          # S > N
    assert fn(h, None, p, p, p, p, 1, 1, 4, 8, 1, 1, 0, 1, ctypes.byref(out)) == -1       # null pointer
    assert fn(h, p, p, p, p, p, 1, 1, 4, 8, 1, 1, 0, 1, None) == -1
    assert fn(None, p, p, p, p, p, 1, 1, 4, 8, 1, 1, 0, 1, ctypes.byref(out)) == -1       # no handle


# ---- solve = the coder and the dense step, composed --------------------------------------------------------------------
K = 3
COMPOSE = [(0, 'float32', 'omp'), (0, 'float32', 'mp'), (0, 'float32', 'mp_pos'), (0, 'float64', 'omp'),
           (2, 'complex64', 'omp'), (2, 'complex64', 'mp'), (2, 'complex128', 'mp')]
WINDOW = {0: (8, 60), 2: (8, 40)}          # problem -> (minibatch, size_of_minibatch)


def _coder(method, y, D, s, stride, padding):
    from decomp_amd import template_matching as tm
    if method == 'omp':
        return tm.orthogonal_pursuit(y, D, n_nonzero_coefs=s, stride=stride, padding=padding)[1]
    return tm.pursuit(y, D, n_nonzero_coefs=s, stride=stride, padding=padding, positive=(method == 'mp_pos'))[1]


def _composed(y, D0, method, s, stride, padding, window=None, seed=None):
    """K rounds of the public coder and tm._dstep on the device: (D, x) as NumPy."""
    import torch
    from decomp_amd import template_matching as tm
    from decomp_amd.utils import normalize
    yd = _dev(y)
    D = normalize.l2_strict(_dev(D0), axis=-1)
    B, N = y.shape
    T, S = D0.shape
    C = tm._coef_size(S, N, stride, padding)
    XXt = torch.zeros((T * S, T * S), dtype=D.dtype, device=D.device)
    yX = torch.zeros((T * S,), dtype=D.dtype, device=D.device)
    if window is None:
        for _ in range(K):
            x = _coder(method, yd, D, s, stride, padding).contiguous()
            tm._dstep(yd, x, D, XXt, yX, stride, padding, 0)
        return D.cpu().numpy(), x.cpu().numpy()
    m, w = window
    cw = tm._coef_size(S, w, stride, padding)
    pc = 0 if padding == 'VALID' else 1
    rng = np.random.RandomState(seed)
    x = torch.zeros((B, T, C), dtype=D.dtype, device=D.device)
    yw = torch.empty((m, w), dtype=D.dtype, device=D.device)
    xw = torch.empty((m, T, cw), dtype=D.dtype, device=D.device)
    for it in range(1, K + 1):
        rows, starts = tm._draw_windows(rng, B, N, w, m, C, cw)
        ib, inn = _dev(np.asarray(rows, np.int64)), _dev(np.asarray(starts, np.int64))
        tm._call(yd, 'gather_windows', yd, x, ib, inn, m, B, T, S, N, w, stride, pc, yw, xw)
        xq = _coder(method, yw, D, s, stride, padding).contiguous()
        tm._call(yd, 'scatter_windows', xq, x, ib, inn, m, B, T, S, N, w, stride, pc)
        tm._dstep(yw, xq, D, XXt, yX, stride, padding, it)
    return D.cpu().numpy(), x.cpu().numpy()


@pytest.mark.parametrize('loop', ['batch', 'minibatch'])
@pytest.mark.parametrize('problem,dtype,method', COMPOSE)
def test_solve_is_the_coder_and_the_dense_step(problem, dtype, method, loop):
    import torch
    from decomp_amd import template_matching as tm
    y, D0, (stride, padding), nev = ref.planted(problem)
    y, D0 = y.astype(dtype), D0.astype(dtype)
    window = WINDOW[problem] if loop == 'minibatch' else None
    kw = dict(stride=stride, padding=padding, tol=0, maxiter=K + 1, lasso_method=method, lasso_iter=nev,
              lasso_tol=None)
    if window:
        kw.update(minibatch=window[0], size_of_minibatch=window[1], random_seed=5)
    Dw, xw = _composed(y, D0, method, nev, stride, padding, window, 5)
    assert np.count_nonzero(xw) > 0 and np.all(np.isfinite(Dw))
    it, D, x = tm.solve(y.copy(), D0.copy(), 0, **kw)
    assert it == K + 1 and isinstance(D, np.ndarray) and isinstance(x, np.ndarray)
    assert _same_bits(D, Dw) and _same_bits(x, xw)
    # torch tensors stay on the device; an x passed in is not read by the coder (the batch loop overwrites all of it)
    x_in = None if window else torch.full(x.shape, 7.0, dtype=_dev(y).dtype, device='cuda')
    it, Dt, xt = tm.solve(_dev(y), _dev(D0), 0, x=x_in, **kw)
    assert it == K + 1 and torch.is_tensor(Dt) and Dt.is_cuda and xt.is_cuda
    assert _same_bits(Dt.cpu().numpy(), Dw) and _same_bits(xt.cpu().numpy(), xw)


@pytest.mark.parametrize('problem,dtype,method', [(0, 'float32', 'omp'), (2, 'complex64', 'mp')])
def test_solve_one_signal(problem, dtype, method):
    """y [N]: x comes back as [T, C], the bits of the batch of one."""
    from decomp_amd import template_matching as tm
    y, D0, (stride, padding), nev = ref.planted(problem)
    y, D0 = y[3].astype(dtype), D0.astype(dtype)
    Dw, xw = _composed(y[None], D0, method, nev, stride, padding)
    it, D, x = tm.solve(y, D0, 0, stride=stride, padding=padding, tol=0, maxiter=K + 1, lasso_method=method,
                        lasso_iter=nev, lasso_tol=None)
    assert it == K + 1 and x.shape == xw.shape[1:]
    assert _same_bits(D, Dw) and _same_bits(x, xw[0])


def test_solve_stops_on_tol():
    """The stop rule max|dD| < tol holds for the greedy loop: a tol above the first step's change stops at it = 1."""
    from decomp_amd import template_matching as tm
    y, D0, (stride, padding), nev = ref.planted(0)
    it, D, x = tm.solve(y.astype(np.float32), D0.astype(np.float32), 0, stride=stride, padding=padding, tol=10.0,
                        maxiter=5, lasso_method='omp', lasso_iter=nev, lasso_tol=None)
    assert it == 1 and np.count_nonzero(x) > 0


# ---- end to end on the planted problems ------------------------------------------------------------------------------------
@pytest.mark.parametrize('problem', [0, 1, 2])
def test_learns_the_planted_templates(problem):
    """solve(lasso_method='omp', maxiter=11, tol=0) in float32 / complex64: the templates it returns explain y as well
    as those of the NumPy loop (tm_learn_ref.coded_residual: the median |y - x * D| / |y| of a fresh 'omp' code on the
    returned D, coded and measured in double on the CPU).

    The yardstick is the gap between the single- and the double-precision runs of tm_learn_ref on the CPU (the values
    are in test_tm_learn_host.test_reference_loop_learns_the_planted_templates): the GPU's residual may exceed the
    double run's by at most twice that gap.  On these problems the CPU's single-precision trajectory meets no near
    tie and the gap is 1e-8 or less, which says nothing about a trajectory that does meet one: the kernels add in
    another order (and fuse multiply-adds), so a near tie between two atoms can fall the other way on the GPU.  One
    such choice alters the code of one signal in one iteration; D is a step along statistics summed over the B
    signals, so it moves by O(1 / B) of what one signal contributes, and the residual at noise level r moves by at
    most about r / B.  The floor of the allowance is therefore r64 / B: one signal's share.

    Observed on an MI355X (residual after 10 iterations; the double run's value in brackets):
      problem 0  float32    0.04886670  (0.04886670)
      problem 1  float32    0.04887592  (0.04887592)
      problem 2  complex64  0.08043642  (0.08043644)"""
    from decomp_amd import template_matching as tm
    seed, B, T, S, N, stride, padding, nev, cplx = ref.PLANTED[problem]
    y, D0, _, _ = ref.planted(problem)
    dt = ref.precision_dtype(cplx, 'single')
    start, r64 = ref.planted_run(problem, 'double')
    _, r32 = ref.planted_run(problem, 'single')
    it, D, x = tm.solve(y.astype(dt), D0.astype(dt), 0, stride=stride, padding=padding, tol=0, maxiter=11,
                        lasso_method='omp', lasso_iter=nev, lasso_tol=None)
    assert it == 11 and D.dtype == dt and np.all(np.isfinite(D))
    assert np.count_nonzero(x.reshape(B, -1), axis=1).max() <= nev
    got = ref.coded_residual(y, D, stride, padding, nev)
    allow = max(2 * abs(r32 - r64), r64 / B)
    print('problem %d: start %.6f, double %.8f, single %.8f, GPU %.8f (allowance %.2e)' % (problem, start, r64, r32,
                                                                                           got, allow))
    assert got <= r64 + allow
