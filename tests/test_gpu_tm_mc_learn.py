"""GPU: learning multichannel templates D [T, Ch, S] -- the dictionary step dcp_tm_mc_dstep_events_* against the
one-channel step dcp_tm_dstep_events_* channel by channel, bit for bit (XXt is that of any one channel, yX[:, ch] that
of channel ch; at Ch = 1 D and max|dD| too), and its D and max|dD| against tm_mc_learn_ref.d_update in double;
dcp_tm_mc_gather_windows_* against NumPy slicing; template_matching.solve with a 3-D D against the same loop written
out with the public multichannel coders and the step, bit for bit, against the 2-D solve at Ch = 1, and on the planted
problems of tm_mc_learn_ref against the NumPy loop.

Bounds against the oracle (those of test_gpu_tm_learn.py, restated): D and max|dD| within FLOOR_MULT times what the
reference's own update shows in single precision against double (never below u = 2^-24), 1e-10 in double."""
import ctypes

import numpy as np
import pytest

import tm_learn_ref
import tm_mc_learn_ref as ref
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


def _check_update(dtype, geom, y, x, D, XXt_in, yX_in, acc_it, got):
    """D and maxdiff of a step against tm_mc_learn_ref.d_update on the reference's own statistics, in double."""
    B, T, Ch, S, N, s, p = geom
    W = _wide(dtype)
    diff, Dg = got[0], got[1]
    XXt, yX = ref.statistics(y.astype(W), x.astype(W), S, s, p)
    if acc_it:
        XXt, yX = otm.accumulate(XXt_in.astype(W), yX_in.astype(W), XXt, yX, acc_it)
    D64, d64 = ref.d_update(D.astype(W), XXt, yX)
    D32, d32 = None, 0.0
    if _single(dtype):
        XX32, yX32 = ref.statistics(y, x, S, s, p)
        if acc_it:
            XX32, yX32 = otm.accumulate(XXt_in, yX_in, XX32, yX32, acc_it)
        D32, d32 = ref.d_update(D, XX32, yX32)
    _check_iterated(Dg, D64, D32, dtype, 'D')
    _check_iterated(np.array([diff]), np.array([d64]), np.array([d32]), dtype, 'maxdiff',
                    scale=float(np.max(np.abs(D64))))


# ---- geometry ---------------------------------------------------------------------------------------------------------
# (B, T, Ch, S, N, stride, padding): each the smallest shape that reaches a distinct path of the step
GEOMS = [
    (3, 2, 3, 33, 300, 1, 'SAME'),      # the general case
    (2, 2, 5, 60, 200, 1, 'SAME'),      # Ch S = 300 cells: two cell blocks
    (2, 2, 2, 16, 700, 4, 'VALID'),     # stride > 1
    (2, 1, 3, 120, 120, 1, 'VALID'),    # C = 1
    (1, 2, 2, 300, 900, 1, 'SAME'),     # S > 256: a channel spans two cell blocks
    (2, 2, 1, 33, 300, 1, 'SAME'),      # Ch = 1
]
GEOM_IDS = ['general', 'cells300', 'stride4', 'C1', 'S300', 'Ch1']


def _C(geom):
    return otm.geometry(geom[3], geom[4], geom[5], geom[6])[0]


def test_geometries_reach_their_paths():
    C = [_C(g) for g in GEOMS]
    assert GEOMS[1][2] * GEOMS[1][3] == 300 and C[3] == 1 and GEOMS[4][3] > 256 and GEOMS[5][2] == 1
    assert C[0] > 256 and C[1] > 256 and C[4] > 256              # a list of more than 256 events is possible
    assert all(g[2] * g[3] > 256 for g in (GEOMS[1], GEOMS[3], GEOMS[4]))      # more than one cell block


# ---- hand-made codes (the pattern ideas of test_gpu_tm_learn.py) ---------------------------------------------------------
def _values(rng, n, dtype):
    """n non-zero values, magnitudes in [0.5, 1.5]."""
    v = (0.5 + rng.rand(n)) * rng.choice([-1.0, 1.0], n)
    if np.dtype(dtype).kind == 'c':
        v = v * np.exp(2j * np.pi * rng.rand(n))
    return v.astype(dtype)


def _sparse(rng, shape, dtype, density):
    return (_randn(rng, shape, dtype) * (rng.uniform(size=shape) < density)).astype(dtype)


def _patterns(geom, dtype, rng):
    """[(name, x, the max_events to run)]"""
    B, T, Ch, S, N, s, p = geom
    C = _C(geom)
    shape = (B, T, C)
    out = []
    # rows with no event, one row with a single event
    x = np.zeros(shape, dtype)
    x[B - 1, T - 1, C // 2] = _values(rng, 1, dtype)[0]
    out.append(('one-event', x, [1, 3]))
    # events at the first and last coefficients only: the taps that leave the signal ('SAME') are clipped per tap
    x = np.zeros(shape, dtype)
    edge = np.unique(np.r_[0:min(C, S + 1), max(0, C - S - 1):C])
    x[:, :, edge] = _values(rng, B * T * edge.size, dtype).reshape(B, T, -1)
    out.append(('edges-only', x, [2, C]))
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
    B, T, Ch, S, N, s, p = geom
    D = _randn(rng, (T, Ch, S), dtype)
    D = (D / np.linalg.norm(D.reshape(T, -1), axis=1)[:, None, None]).astype(dtype)
    return _randn(rng, (B, Ch, N), dtype), D


def _mc_step(yd, xd, D, XXt, yX, s, p, acc_it, max_events):
    """One multichannel step from host copies of D and the sums: (maxdiff, D, XXt, yX) as NumPy."""
    from decomp_amd import template_matching as tm
    Dd, XXd, yXd = _dev(D.copy()), _dev(XXt.copy()), _dev(yX.copy())
    diff = tm._mc_dstep_events(yd, xd, Dd, XXd, yXd, s, p, acc_it, max_events)
    return diff, Dd.cpu().numpy(), XXd.cpu().numpy(), yXd.cpu().numpy()


def _one_step(y, xd, D, XXt, yX, s, p, acc_it, max_events):
    """The one-channel step on channel data y [B, N], D [T, S], yX [T S]: (maxdiff, D, XXt, yX) as NumPy."""
    from decomp_amd import template_matching as tm
    Dd, XXd, yXd = _dev(D.copy()), _dev(XXt.copy()), _dev(yX.copy())
    diff = tm._dstep_events(_dev(y), xd, Dd, XXd, yXd, s, p, acc_it, max_events)
    return diff, Dd.cpu().numpy(), XXd.cpu().numpy(), yXd.cpu().numpy()


def _assert_same(a, b, what):
    bad = ['%s differs in %d elements (by up to %.3g)' % (name, int(np.sum(u != v)), float(np.max(np.abs(u - v))))
           for name, u, v in zip(('XXt', 'yX', 'D'), a[2:] + a[1:2], b[2:] + b[1:2]) if not _same_bits(u, v)]
    if a[0] != b[0]:
        bad.append('maxdiff %r != %r' % (a[0], b[0]))
    assert not bad, '%s: %s' % (what, '; '.join(bad))


def _assert_channels(geom, got, y, xd, D, XXt_in, yX_in, acc_it, cap, what):
    """XXt is the one-channel step's on (y[:, 0], x); yX[:, ch] is the one-channel step's on (y[:, ch], x), for every
    channel; at Ch = 1, D and maxdiff are that step's too."""
    B, T, Ch, S, N, s, p = geom
    yX3, yXin3 = got[3].reshape(T, Ch, S), yX_in.reshape(T, Ch, S)
    for ch in range(Ch):
        one = _one_step(y[:, ch], xd, D[:, ch], XXt_in, yXin3[:, ch].reshape(-1), s, p, acc_it, cap)
        assert _same_bits(yX3[:, ch].reshape(-1), one[3]), '%s: yX of channel %d differs' % (what, ch)
        if ch == 0:
            assert _same_bits(got[2], one[2]), '%s: XXt differs' % what
        if Ch == 1:
            assert _same_bits(got[1][:, 0], one[1]) and got[0] == one[0], '%s: D or maxdiff differs at Ch = 1' % what


@pytest.mark.parametrize('dtype', DTYPES)
@pytest.mark.parametrize('geom', GEOMS, ids=GEOM_IDS)
def test_mc_step_equals_the_one_channel_step_per_channel_bitwise(geom, dtype):
    """acc_it = 0 on every hand-made code: XXt and yX are the one-channel event step's bits channel by channel (D and
    maxdiff too at Ch = 1), the result is the same for every max_events and on a second call, and D and maxdiff lie
    within the oracle's bounds."""
    B, T, Ch, S, N, s, p = geom
    rng = np.random.RandomState(S + N + s + Ch)
    y, D = _problem(geom, dtype, rng)
    yd = _dev(y)
    zXX, zyX = np.zeros((T * S, T * S), dtype), np.zeros(T * Ch * S, dtype)
    for name, x, caps in _patterns(geom, dtype, rng):
        xd = _dev(x)
        first = _mc_step(yd, xd, D, zXX, zyX, s, p, 0, caps[0])
        assert np.all(np.isfinite(first[2])) and np.all(np.isfinite(first[3])) and np.isfinite(first[0])
        for cap in caps[1:]:
            _assert_same(_mc_step(yd, xd, D, zXX, zyX, s, p, 0, cap), first, '%s, max_events %d' % (name, cap))
        _assert_same(_mc_step(yd, xd, D, zXX, zyX, s, p, 0, caps[0]), first, '%s, second call' % name)
        _assert_channels(geom, first, y, xd, D, zXX, zyX, 0, caps[-1], name)
        if name in ('long-row', 'dense30'):
            _check_update(dtype, geom, y, x, D, zXX, zyX, 0, first)


@pytest.mark.parametrize('dtype', DTYPES)
@pytest.mark.parametrize('geom', GEOMS, ids=GEOM_IDS)
def test_mc_step_running_sums_bitwise(geom, dtype):
    """acc_it = 1, 2, 3 with another (y, x) at each call, continued from the kernel's own sums and D as the minibatch
    loop does: channel by channel the one-channel step's bits at every call, within the oracle's bounds."""
    B, T, Ch, S, N, s, p = geom
    C = _C(geom)
    rng = np.random.RandomState(11 + S + Ch)
    _, D = _problem(geom, dtype, rng)
    XXt, yX = np.zeros((T * S, T * S), dtype), np.zeros(T * Ch * S, dtype)
    for acc_it, (density, cap) in zip((1, 2, 3), ((0.02, 8), (0.3, 2), (0.05, C))):
        x = _sparse(rng, (B, T, C), dtype, density)
        y = _randn(rng, (B, Ch, N), dtype)
        yd, xd = _dev(y), _dev(x)
        got = _mc_step(yd, xd, D, XXt, yX, s, p, acc_it, cap)
        _assert_channels(geom, got, y, xd, D, XXt, yX, acc_it, cap, 'acc_it %d' % acc_it)
        _check_update(dtype, geom, y, x, D, XXt, yX, acc_it, got)
        _, D, XXt, yX = got


def test_mc_step_rejects_bad_arguments():
    import torch
    from decomp_amd import _arrays
    t = torch.zeros(64, device='cuda')
    lib, h = _arrays.lib_handle(t)
    p = _arrays.ptr(t)
    out = ctypes.c_double(0.0)
    fn = lib.dcp_tm_mc_dstep_events_f32
    #          Y  X  D  XXt yX B  T  Ch S  N  stride padding acc_it max_events
    assert fn(h, p, p, p, p, p, 1, 1, 2, 4, 8, 1, 1, 0, 0, ctypes.byref(out)) == -1          # max_events < 1
    assert fn(h, p, p, p, p, p, 1, 1, 2, 4, 8, 1, 1, -1, 1, ctypes.byref(out)) == -1         # acc_it < 0
    assert fn(h, p, p, p, p, p, 1, 1, 2, 9, 8, 1, 1, 0, 1, ctypes.byref(out)) == -1          # S > N
    assert fn(h, p, p, p, p, p, 1, 1, 0, 4, 8, 1, 1, 0, 1, ctypes.byref(out)) == -1          # Ch < 1
    assert fn(h, p, p, p, p, p, 1, 1, 2, 4, 8, 0, 1, 0, 1, ctypes.byref(out)) == -1          # stride < 1
    assert fn(h, None, p, p, p, p, 1, 1, 2, 4, 8, 1, 1, 0, 1, ctypes.byref(out)) == -1       # null pointer
    assert fn(h, p, p, p, p, p, 1, 1, 2, 4, 8, 1, 1, 0, 1, None) == -1
    assert fn(None, p, p, p, p, p, 1, 1, 2, 4, 8, 1, 1, 0, 1, ctypes.byref(out)) == -1       # no handle
    gw = lib.dcp_tm_mc_gather_windows_f32
    #          Y  X  ib in m  B  T  Ch S  N  w  stride padding Yw Xw
    assert gw(h, p, p, p, p, 1, 1, 1, 0, 4, 8, 6, 1, 1, p, p) == -1                           # Ch < 1
    assert gw(h, p, p, p, p, 1, 1, 1, 2, 4, 8, 9, 1, 1, p, p) == -1                           # w > N
    assert gw(h, p, p, p, p, 1, 1, 1, 2, 4, 8, 3, 1, 1, p, p) == -1                           # w < S
    assert gw(h, p, p, None, p, 1, 1, 1, 2, 4, 8, 6, 1, 1, p, p) == -1                        # null pointer


@pytest.mark.parametrize('dtype', DTYPES)
@pytest.mark.parametrize('geom', [(5, 2, 3, 7, 90, 1, 'SAME'), (4, 3, 1, 6, 301, 2, 'VALID')], ids=['same', 'stride2-Ch1'])
def test_mc_gather_windows_is_numpy_slicing(geom, dtype):
    import torch
    from decomp_amd import template_matching as tm
    B, T, Ch, S, N, s, p = geom
    C = _C(geom)
    w, m = 40, 9
    cw = otm.geometry(S, w, s, p)[0]
    rng = np.random.RandomState(3)
    y, x = _randn(rng, (B, Ch, N), dtype), _randn(rng, (B, T, C), dtype)
    rows = rng.randint(0, B, m)
    starts = rng.randint(0, min(N - w, C - cw) + 1, m)
    rows[1], starts[1] = rows[0], starts[0]                                    # a window drawn twice
    ib, inn = _dev(rows.astype(np.int64)), _dev(starts.astype(np.int64))
    yw = torch.full((m, Ch, w), 7, dtype=_dev(y).dtype, device='cuda')
    xw = torch.full((m, T, cw), 7, dtype=yw.dtype, device='cuda')
    tm._call(yw, 'mc_gather_windows', _dev(y), _dev(x), ib, inn, m, B, T, Ch, S, N, w, s, 0 if p == 'VALID' else 1, yw,
             xw)
    np.testing.assert_array_equal(yw.cpu().numpy(), otm.gather_windows(y, rows, starts, w))
    np.testing.assert_array_equal(xw.cpu().numpy(), otm.gather_windows(x, rows, starts, cw))


# ---- solve = the multichannel coder and the step, composed ------------------------------------------------------------------
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
    """K rounds of the public coder on the 3-D D and tm._mc_dstep_events on the device: (D, x) as NumPy."""
    import torch
    from decomp_amd import template_matching as tm
    from decomp_amd.utils import normalize
    yd = _dev(y)
    T, Ch, S = D0.shape
    D = normalize.l2_strict(_dev(D0).reshape(T, Ch * S), axis=-1).reshape(T, Ch, S).contiguous()
    B, N = y.shape[0], y.shape[-1]
    C = tm._coef_size(S, N, stride, padding)
    XXt = torch.zeros((T * S, T * S), dtype=D.dtype, device=D.device)
    yX = torch.zeros((T * Ch * S,), dtype=D.dtype, device=D.device)
    if window is None:
        for _ in range(K):
            x = _coder(method, yd, D, s, stride, padding).contiguous()
            tm._mc_dstep_events(yd, x, D, XXt, yX, stride, padding, 0, min(s, C))
        return D.cpu().numpy(), x.cpu().numpy()
    m, w = window
    cw = tm._coef_size(S, w, stride, padding)
    pc = 0 if padding == 'VALID' else 1
    rng = np.random.RandomState(seed)
    x = torch.zeros((B, T, C), dtype=D.dtype, device=D.device)
    yw = torch.empty((m, Ch, w), dtype=D.dtype, device=D.device)
    xw = torch.empty((m, T, cw), dtype=D.dtype, device=D.device)
    for it in range(1, K + 1):
        rows, starts = tm._draw_windows(rng, B, N, w, m, C, cw)
        ib, inn = _dev(np.asarray(rows, np.int64)), _dev(np.asarray(starts, np.int64))
        tm._call(yd, 'mc_gather_windows', yd, x, ib, inn, m, B, T, Ch, S, N, w, stride, pc, yw, xw)
        xq = _coder(method, yw, D, s, stride, padding).contiguous()
        tm._call(yd, 'scatter_windows', xq, x, ib, inn, m, B, T, S, N, w, stride, pc)
        tm._mc_dstep_events(yw, xq, D, XXt, yX, stride, padding, it, min(s, cw))
    return D.cpu().numpy(), x.cpu().numpy()


@pytest.mark.parametrize('loop', ['batch', 'minibatch'])
@pytest.mark.parametrize('problem,dtype,method', COMPOSE)
def test_solve_is_the_mc_coder_and_the_mc_step(problem, dtype, method, loop):
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
    assert it == K + 1 and isinstance(D, np.ndarray) and isinstance(x, np.ndarray) and D.shape == D0.shape
    assert _same_bits(D, Dw) and _same_bits(x, xw)
    # torch tensors stay on the device; an x passed in is not read by the coder (the batch loop overwrites all of it)
    x_in = None if window else torch.full(x.shape, 7.0, dtype=_dev(y).dtype, device='cuda')
    it, Dt, xt = tm.solve(_dev(y), _dev(D0), 0, x=x_in, **kw)
    assert it == K + 1 and torch.is_tensor(Dt) and Dt.is_cuda and xt.is_cuda
    assert _same_bits(Dt.cpu().numpy(), Dw) and _same_bits(xt.cpu().numpy(), xw)


@pytest.mark.parametrize('problem,dtype,method', [(0, 'float32', 'omp'), (2, 'complex64', 'mp')])
def test_solve_one_signal(problem, dtype, method):
    """y [Ch, N]: x comes back as [T, C], the bits of the batch of one."""
    from decomp_amd import template_matching as tm
    y, D0, (stride, padding), nev = ref.planted(problem)
    y, D0 = y[3].astype(dtype), D0.astype(dtype)
    Dw, xw = _composed(y[None], D0, method, nev, stride, padding)
    it, D, x = tm.solve(y, D0, 0, stride=stride, padding=padding, tol=0, maxiter=K + 1, lasso_method=method,
                        lasso_iter=nev, lasso_tol=None)
    assert it == K + 1 and x.shape == xw.shape[1:]
    assert _same_bits(D, Dw) and _same_bits(x, xw[0])


@pytest.mark.parametrize('loop', ['batch', 'minibatch'])
@pytest.mark.parametrize('dtype,method', [('float32', 'omp'), ('float64', 'omp'), ('float32', 'mp'), ('float64', 'mp_pos')])
def test_solve_with_one_channel_is_the_2d_solve(dtype, method, loop):
    """D [T, 1, S], y [B, 1, N] in the real dtypes: D and x of the 2-D solve, bit for bit (the multichannel coders give
    the one-channel coders' bits there, and the step's sums are the one-channel step's)."""
    from decomp_amd import template_matching as tm
    y, D0, (stride, padding), nev = tm_learn_ref.planted(0)
    y, D0 = y.astype(dtype), D0.astype(dtype)
    kw = dict(stride=stride, padding=padding, tol=0, maxiter=K + 1, lasso_method=method, lasso_iter=nev,
              lasso_tol=None)
    if loop == 'minibatch':
        kw.update(minibatch=8, size_of_minibatch=60, random_seed=5)
    it2, D2, x2 = tm.solve(y.copy(), D0.copy(), 0, **kw)
    it3, D3, x3 = tm.solve(y[:, None, :].copy(), D0[:, None, :].copy(), 0, **kw)
    assert it2 == it3 == K + 1 and D3.shape == (D0.shape[0], 1, D0.shape[1]) and np.count_nonzero(x2) > 0
    assert _same_bits(D3[:, 0], D2) and _same_bits(x3, x2)


def test_solve_stops_on_tol():
    """The stop rule max|dD| < tol over all T Ch S entries: a tol above the first step's change stops at it = 1."""
    from decomp_amd import template_matching as tm
    y, D0, (stride, padding), nev = ref.planted(0)
    it, D, x = tm.solve(y.astype(np.float32), D0.astype(np.float32), 0, stride=stride, padding=padding, tol=10.0,
                        maxiter=5, lasso_method='omp', lasso_iter=nev, lasso_tol=None)
    assert it == 1 and np.count_nonzero(x) > 0 and D.shape == D0.shape


# ---- end to end on the planted problems ------------------------------------------------------------------------------------
@pytest.mark.parametrize('problem', [0, 1, 2])
def test_learns_the_planted_templates(problem):
    """solve(lasso_method='omp', maxiter=11, tol=0) in float32 / complex64 on D [T, Ch, S]: the templates it returns
    explain y as well as those of the NumPy loop (tm_mc_learn_ref.coded_residual: the median |y - x * D| / |y| over all
    channels of a fresh 'omp' code on the returned D, coded and measured in double on the CPU).

    The allowance and its reasoning are those of test_gpu_tm_learn.test_learns_the_planted_templates: the GPU's
    residual may exceed the double run's by at most twice the gap between the single- and the double-precision runs of
    the reference on the CPU (the values are in test_tm_mc_learn_host.test_reference_loop_learns_the_planted_templates),
    and never less than r64 / B: the kernels add in another order, so a near tie between two atoms can fall the other way
    on the GPU; one such choice alters the code of one signal in one iteration, D is a step along statistics summed
    over the B signals and so moves by O(1 / B) of what one signal contributes, and the residual at noise level r by at
    most about r / B.

    Observed on an MI355X (residual after 10 iterations; the double run's value in brackets):
      problem 0  float32    0.04978088  (0.04978088)
      problem 1  float32    0.04931928  (0.04931927)
      problem 2  complex64  0.06972247  (0.06972247)"""
    from decomp_amd import template_matching as tm
    seed, B, T, Ch, S, N, stride, padding, nev, cplx = ref.PLANTED[problem]
    y, D0, _, _ = ref.planted(problem)
    dt = ref.precision_dtype(cplx, 'single')
    start, r64 = ref.planted_run(problem, 'double')
    _, r32 = ref.planted_run(problem, 'single')
    it, D, x = tm.solve(y.astype(dt), D0.astype(dt), 0, stride=stride, padding=padding, tol=0, maxiter=11,
                        lasso_method='omp', lasso_iter=nev, lasso_tol=None)
    assert it == 11 and D.dtype == dt and D.shape == (T, Ch, S) and np.all(np.isfinite(D))
    assert np.count_nonzero(x.reshape(B, -1), axis=1).max() <= nev
    got = ref.coded_residual(y, D, stride, padding, nev)
    allow = max(2 * abs(r32 - r64), r64 / B)
    print('problem %d: start %.6f, double %.8f, single %.8f, GPU %.8f (allowance %.2e)' % (problem, start, r64, r32,
                                                                                           got, allow))
    assert got <= r64 + allow
