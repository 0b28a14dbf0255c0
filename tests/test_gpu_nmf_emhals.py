"""GPU: em-hals, HALS NMF for data with missing or weighted entries (nmf.solve(method='em-hals'),
dcp_nmf_emhals_*) and its imputing product (dcp_nmf_impute_*), against the float64 NumPy restatement in
tests/emhals_ref.py (pinned on the CPU by test_emhals_ref_host.py)."""
import ctypes

import numpy as np
import pytest

import emhals_ref
from test_emhals_ref_host import BINARY30_SEED

pytestmark = pytest.mark.gpu


def _rel(a, b):
    a = np.asarray(a, np.float64)
    b = np.asarray(b, np.float64)
    return float(np.max(np.abs(a - b)) / max(1e-300, float(np.max(np.abs(b)))))


def _np(a):
    import torch
    return a.detach().cpu().numpy() if isinstance(a, torch.Tensor) else np.asarray(a)


def _problem(N, F, K, seed, dtype=np.float64, noise=0.05):
    rng = np.random.RandomState(seed)
    x0 = np.maximum(rng.randn(N, K), 0)
    D0 = np.maximum(rng.randn(K, F), 0)
    y = x0.dot(D0) + noise * np.abs(rng.randn(N, F))
    D = np.abs(rng.randn(K, F)) + 0.05
    return y.astype(dtype), D.astype(dtype)


def _mask(kind, shape, seed, dtype):
    if kind == 'binary':
        return emhals_ref.binary_mask(shape, 0.3, seed, dtype)
    if kind == 'weighted':
        return emhals_ref.weights(shape, 0.0, seed, dtype)
    return (np.ones if kind == 'ones' else np.zeros)(shape, dtype)


# ---- the impute kernel --------------------------------------------------------------------------------------
GUARD = 3   # rows of NaN in front of and behind the output


def _impute_gpu(y, w, x, D):
    """dcp_nmf_impute_* into rows GUARD .. GUARD+N of a NaN-filled buffer.  Returns the whole buffer."""
    import torch
    from decomp_amd import _arrays, _hip
    N, F = y.shape
    K = D.shape[0]
    yd, wd, xd, Dd = (torch.from_numpy(np.ascontiguousarray(a)).cuda() for a in (y, w, x, D))
    buf = torch.full((N + 2 * GUARD, F), float('nan'), dtype=yd.dtype, device='cuda')
    out = buf[GUARD:GUARD + N]
    lib, h = _arrays.lib_handle(yd)
    fn = getattr(lib, 'dcp_nmf_impute_' + _arrays.suffix(yd))
    _hip.check(h, fn(h, _arrays.ptr(yd), _arrays.ptr(wd), _arrays.ptr(xd), _arrays.ptr(Dd), N, F, K,
                     _arrays.ptr(out)), 'dcp_nmf_impute')
    torch.cuda.synchronize()
    return buf.cpu().numpy()


@pytest.mark.parametrize('dtype', [np.float32, np.float64])
@pytest.mark.parametrize('kind', ['binary', 'weighted', 'ones', 'zeros'])
@pytest.mark.parametrize('shape', [(1, 1, 1), (63, 65, 3), (64, 64, 4), (65, 63, 5), (129, 130, 33), (300, 129, 37),
                                   (1000, 256, 64)])
def test_impute_matches_numpy(shape, kind, dtype):
    N, F, K = shape
    rng = np.random.RandomState(N * 7 + F + K)
    y = np.abs(rng.randn(N, F)).astype(dtype)
    x = np.abs(rng.randn(N, K)).astype(dtype)
    D = np.abs(rng.randn(K, F)).astype(dtype)
    w = _mask(kind, (N, F), N + K, dtype)
    ref = emhals_ref.impute_np(y, w, x, D)
    buf = _impute_gpu(y, w, x, D)
    got = buf[GUARD:GUARD + N]
    assert np.all(np.isnan(buf[:GUARD])) and np.all(np.isnan(buf[GUARD + N:]))   # nothing outside [N, F]
    assert got.dtype == dtype and np.all(np.isfinite(got))
    one = w == 1
    assert np.array_equal(got[one], y[one])                                       # observed: y bit for bit
    assert _rel(got, ref) <= (1e-5 if dtype == np.float32 else 1e-12)
    if kind == 'zeros':
        assert _rel(got, x.astype(np.float64).dot(D.astype(np.float64))) <= (1e-5 if dtype == np.float32 else 1e-12)
    again = _impute_gpu(y, w, x, D)
    assert np.array_equal(again[GUARD:GUARD + N], got)                            # deterministic


# ---- solve against the restatement ----------------------------------------------------------------------------
def _f32_np_iterates(y, D0, w, maxiter):
    """The same iterations in float32 NumPy: the rounding floor of a float32 run against the float64 restatement."""
    y, D0, w = (a.astype(np.float32) for a in (y, D0, w))

    def sweep(V, C, G):
        V = V.copy()
        for k in range(G.shape[0]):
            if G[k, k] > 0:
                V[:, k] = np.maximum(np.float32(0), V[:, k] - (V.dot(G[:, k]) - C[:, k]) / G[k, k])
        return V
    D = D0 / np.sqrt(np.sum(D0 * D0, axis=1, keepdims=True))
    x = np.ones((y.shape[0], D.shape[0]), np.float32)
    for _ in range(1, maxiter):
        yi = w * y + (np.float32(1) - w) * x.dot(D)
        x = sweep(x, yi.dot(D.T), D.dot(D.T))
        Dt = sweep(D.T, x.T.dot(yi).T, x.T.dot(x))
        n = np.sqrt(np.sum(Dt * Dt, axis=0))
        D = (Dt / n).T.copy()
        x = x * n
    return D, x


@pytest.mark.parametrize('kind', ['binary', 'weighted'])
@pytest.mark.parametrize('shape', [(64, 48, 4), (101, 20, 3), (300, 129, 37), (1000, 256, 64)])
def test_solve_f64_parity(shape, kind):
    from decomp_amd import nmf
    N, F, K = shape
    y, D0 = _problem(N, F, K, seed=N + K)
    w = _mask(kind, (N, F), N + 1, np.float64)
    it, D, x = nmf.solve(y, D0.copy(), tol=0.0, maxiter=6, method='em-hals', mask=w)
    ito, Do, xo = emhals_ref.emhals_solve_np(y, D0, w, tol=0.0, maxiter=6)
    assert it == ito == 6
    print('f64', shape, kind, _rel(D, Do), _rel(x, xo))
    assert _rel(D, Do) <= 1e-10
    assert _rel(x, xo) <= 1e-10


@pytest.mark.parametrize('mode', [0, 1])
@pytest.mark.parametrize('shape', [(64, 48, 4), (300, 129, 37), (1024, 256, 64)])
def test_solve_f32_parity(shape, mode):
    """The bound is that of the unmasked HALS test, 2e-4.  The same two iterations in float32 NumPy differ from
    the float64 restatement by 5.3e-7 / 3.4e-7 (64, 48, 4), 6.4e-6 / 1.7e-6 (300, 129, 37) and 1.5e-5 / 3.2e-6
    (1024, 256, 64) on D / x: under a third of the bound at every shape, so it stands."""
    import torch
    from decomp_amd import nmf, _arrays
    N, F, K = shape
    y, D0 = _problem(N, F, K, seed=N + K + 1, dtype=np.float32)
    w = _mask('binary', (N, F), N + 2, np.float32)
    ito, Do, xo = emhals_ref.emhals_solve_np(y, D0, w, tol=0.0, maxiter=3)
    D32, x32 = _f32_np_iterates(y, D0, w, 3)
    print('f32 numpy floor', shape, _rel(D32, Do), _rel(x32, xo))
    assert _rel(D32, Do) <= 2e-4 / 3 and _rel(x32, xo) <= 2e-4 / 3
    lib, h = _arrays.lib_handle(torch.zeros(1, device='cuda'))
    prev = lib.dcp_set_f32_product_mode(h, mode)
    try:
        it, D, x = nmf.solve(y, D0.copy(), tol=0.0, maxiter=3, method='em-hals', mask=w)
    finally:
        lib.dcp_set_f32_product_mode(h, prev)
    assert it == ito == 3
    assert D.dtype == np.float32 and x.dtype == np.float32
    print('f32', shape, mode, _rel(D, Do), _rel(x, xo))
    assert _rel(D, Do) <= 2e-4
    assert _rel(x, xo) <= 2e-4


# ---- identity with the existing solver --------------------------------------------------------------------------
@pytest.mark.parametrize('dtype,mode', [(np.float64, None), (np.float32, 0), (np.float32, 1)])
@pytest.mark.parametrize('mask', ['none', 'ones'])
def test_identical_to_hals_without_missing_entries(dtype, mode, mask):
    import torch
    from decomp_amd import nmf, _arrays
    y, D0 = _problem(300, 129, 37, seed=13, dtype=dtype)
    w = None if mask == 'none' else np.ones_like(y)
    lib, h = _arrays.lib_handle(torch.zeros(1, device='cuda'))
    prev = lib.dcp_set_f32_product_mode(h, -1 if mode is None else mode)
    try:
        it1, D1, x1 = nmf.solve(y, D0.copy(), tol=0.0, maxiter=6, method='hals')
        it2, D2, x2 = nmf.solve(y, D0.copy(), tol=0.0, maxiter=6, method='em-hals', mask=w)
    finally:
        if mode is not None:
            lib.dcp_set_f32_product_mode(h, prev)
    assert it1 == it2 == 6
    assert np.array_equal(D1, D2) and np.array_equal(x1, x2)


# ---- the objective never increases --------------------------------------------------------------------------------
def test_masked_loss_monotone_f64():
    import torch
    from decomp_amd import nmf
    y, D0 = _problem(500, 200, 20, seed=7)
    w = emhals_ref.binary_mask(y.shape, 0.3, seed=8)
    D = nmf._arrays.to_device(D0 / np.sqrt(np.sum(D0 * D0, axis=1, keepdims=True)), copy=True)
    x = torch.ones((500, 20), dtype=torch.float64, device=D.device)
    trace = []
    it = nmf._run_emhals(nmf._arrays.to_device(y), nmf._arrays.to_device(w), x, D, 0.0, 31, resid_trace=trace)
    assert it == 31 and len(trace) == 30
    loss = np.array(trace) ** 2
    assert np.all(loss[1:] <= loss[:-1] * (1 + 1e-12))
    ref = []
    emhals_ref.emhals_solve_np(y, D0, w, tol=0.0, maxiter=31, trace=ref)
    assert _rel(trace, ref) <= 1e-10


# ---- against masked MU ----------------------------------------------------------------------------------------
def test_beats_masked_mu_on_the_gpu():
    """The planted problem of the CPU test (30 % missing), 51 iterations from x = ones, both solvers on the GPU."""
    from decomp_amd import nmf
    y, D0 = emhals_ref.planted()
    w = emhals_ref.binary_mask(y.shape, 0.3, seed=BINARY30_SEED)
    x0 = np.ones((300, 12))
    _, Dh, xh = nmf.solve(y, D0.copy(), x=x0.copy(), tol=0.0, maxiter=51, method='em-hals', mask=w)
    _, Dm, xm = nmf.solve(y, D0.copy(), x=x0.copy(), tol=0.0, maxiter=51, method='mu', mask=w)
    rh, rm = emhals_ref.masked_rel_resid(y, w, xh, Dh), emhals_ref.masked_rel_resid(y, w, xm, Dm)
    hid = emhals_ref.hidden_rel_err(y, w, xh, Dh)
    print('em-hals %.4g  masked mu %.4g  hidden %.4g' % (rh, rm, hid))
    assert rh < 0.1 * rm, (rh, rm)
    assert hid < 0.05, hid


# ---- penalties with a mask ------------------------------------------------------------------------------------
@pytest.fixture(scope='module')
def penalty_case():
    y, D0 = _problem(300, 129, 37, seed=21)
    return y, D0, emhals_ref.binary_mask(y.shape, 0.3, seed=22)


@pytest.mark.parametrize('pen', [(0.1, 0.0), (0.0, 0.5), (0.1, 0.5)])
def test_penalty_f64_parity(penalty_case, pen):
    from decomp_amd import nmf
    y, D0, w = penalty_case
    it, D, x = nmf.solve(y, D0.copy(), tol=0.0, maxiter=6, method='em-hals', mask=w, l1_penalty=pen[0],
                         l2_penalty=pen[1])
    ito, Do, xo = emhals_ref.emhals_solve_np(y, D0, w, tol=0.0, maxiter=6, l1=pen[0], l2=pen[1])
    assert it == ito == 6
    assert _rel(D, Do) <= 1e-10 and _rel(x, xo) <= 1e-10


def test_l1_penalty_gives_more_zeros(penalty_case):
    from decomp_amd import nmf
    y, D0, w = penalty_case
    _, _, x0 = nmf.solve(y, D0.copy(), tol=0.0, maxiter=11, method='em-hals', mask=w)
    _, _, x1 = nmf.solve(y, D0.copy(), tol=0.0, maxiter=11, method='em-hals', mask=w, l1_penalty=0.5)
    assert np.sum(x1 == 0) > np.sum(x0 == 0)


# ---- the return contract ----------------------------------------------------------------------------------------
def test_tol_reached_and_not():
    from decomp_amd import nmf
    y, D0 = _problem(200, 80, 6, seed=5)
    w = emhals_ref.binary_mask(y.shape, 0.3, seed=6)
    it, D, x = nmf.solve(y, D0.copy(), tol=1e-4, maxiter=500, method='em-hals', mask=w)
    ito, Do, xo = emhals_ref.emhals_solve_np(y, D0, w, tol=1e-4, maxiter=500)
    assert it == ito and it < 500
    assert _rel(D, Do) <= 1e-9 and _rel(x, xo) <= 1e-9
    it, D, x = nmf.solve(y, D0.copy(), tol=1e-12, maxiter=4, method='em-hals', mask=w)
    ito, Do, xo = emhals_ref.emhals_solve_np(y, D0, w, tol=1e-12, maxiter=4)
    assert it == ito == 4
    assert _rel(D, Do) <= 1e-10 and _rel(x, xo) <= 1e-10


def test_maxiter_one_returns_normalised_input():
    from decomp_amd import nmf
    y, D0 = _problem(50, 30, 4, seed=2)
    w = emhals_ref.binary_mask(y.shape, 0.3, seed=3)
    x0 = np.abs(np.random.RandomState(0).randn(50, 4))
    it, D, x = nmf.solve(y, D0.copy(), x=x0.copy(), maxiter=1, method='em-hals', mask=w)
    assert it == 1
    np.testing.assert_allclose(D, D0 / np.sqrt(np.sum(D0 * D0, axis=1, keepdims=True)), rtol=1e-15)
    assert np.array_equal(x, x0)


def test_torch_in_torch_out():
    import torch
    from decomp_amd import nmf
    y, D0 = _problem(128, 64, 8, seed=4)
    w = emhals_ref.weights(y.shape, 0.2, seed=5)
    yt, Dt, wt = (torch.from_numpy(a).cuda() for a in (y, D0, w))
    it, D, x = nmf.solve(yt, Dt, tol=0.0, maxiter=4, method='em-hals', mask=wt)
    assert isinstance(D, torch.Tensor) and isinstance(x, torch.Tensor)
    assert D.is_cuda and x.is_cuda
    assert torch.equal(Dt, torch.from_numpy(D0).cuda())   # the caller's arrays are not modified
    assert torch.equal(yt, torch.from_numpy(y).cuda()) and torch.equal(wt, torch.from_numpy(w).cuda())
    ito, Do, xo = emhals_ref.emhals_solve_np(y, D0, w, tol=0.0, maxiter=4)
    assert _rel(_np(D), Do) <= 1e-10 and _rel(_np(x), xo) <= 1e-10


def test_unobserved_rows_and_columns_stay_finite():
    """A sample and a channel that were never observed: their entries are imputed entirely, nothing divides by
    zero, and the result is the restatement's."""
    from decomp_amd import nmf
    y, D0 = _problem(90, 40, 5, seed=6)
    w = emhals_ref.binary_mask(y.shape, 0.3, seed=7)
    w[11, :] = 0.0
    w[:, 7] = 0.0
    it, D, x = nmf.solve(y, D0.copy(), tol=0.0, maxiter=8, method='em-hals', mask=w)
    ito, Do, xo = emhals_ref.emhals_solve_np(y, D0, w, tol=0.0, maxiter=8)
    assert np.all(np.isfinite(D)) and np.all(np.isfinite(x))
    assert _rel(D, Do) <= 1e-10 and _rel(x, xo) <= 1e-10


@pytest.mark.parametrize('bad', [1.5, -0.25, float('nan'), float('inf')])
def test_weights_outside_unit_interval_are_an_error(bad):
    from decomp_amd import nmf
    y, D0 = _problem(40, 20, 3, seed=1)
    w = np.ones_like(y)
    w[17, 5] = bad
    with pytest.raises(ValueError):
        nmf.solve(y, D0, method='em-hals', mask=w)


def test_errors():
    from decomp_amd import nmf
    y, D0 = _problem(40, 20, 3, seed=1)
    w = np.ones_like(y)
    with pytest.raises(NotImplementedError):
        nmf.solve(y, D0, method='em-hals', mask=w, likelihood='kl')
    with pytest.raises(NotImplementedError):
        nmf.solve(y, D0, method='em-hals', mask=w, likelihood='is')
    with pytest.raises(NotImplementedError):
        nmf.solve(y, D0, method='em-hals', mask=w, minibatch=10)
    with pytest.raises(TypeError):
        nmf.solve(y, D0, method='em-hals', mask=w, unknown=1)
    lib = nmf._hip.load()
    h = nmf._arrays.lib_handle(nmf._arrays.to_device(D0))[1]
    it = ctypes.c_int(0)
    assert lib.dcp_nmf_emhals_f64(h, None, None, None, None, 4, 4, 2, 0.0, 3, ctypes.byref(it), None, None) \
        == -1
    assert lib.dcp_nmf_impute_f64(h, None, None, None, None, 4, 4, 2, None) == -1
