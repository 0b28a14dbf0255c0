"""GPU: NMF by HALS (nmf.solve(method='hals'), dcp_nmf_hals_*) and its non-negative coordinate sweep
(dcp_nn_cd_sweep_*), against a float64 NumPy restatement of the sweep and of one HALS iteration."""
import ctypes

import numpy as np
import pytest

pytestmark = pytest.mark.gpu


# ---- float64 NumPy restatement ----------------------------------------------------------------------------
def sweep_np(V, C, G):
    """for k = 0 .. K-1 in order, with the current V: where G[k,k] > 0,
    V[:,k] = max(0, V[:,k] - (V G[:,k] - C[:,k]) / G[k,k]); V [R, K], C [R, K], G [K, K]."""
    V = np.array(V, np.float64)
    C = np.asarray(C, np.float64)
    G = np.asarray(G, np.float64)
    for k in range(G.shape[0]):
        if G[k, k] > 0:
            V[:, k] = np.maximum(0.0, V[:, k] - (V.dot(G[:, k]) - C[:, k]) / G[k, k])
    return V


def hals_step_np(y, x, D):
    """One HALS iteration -> (x, D_new, max|D - D_new|)."""
    y, x, D = (np.asarray(a, np.float64) for a in (y, x, D))
    x = sweep_np(x, y.dot(D.T), D.dot(D.T))
    Dt = sweep_np(D.T, x.T.dot(y).T, x.T.dot(x))
    n = np.sqrt(np.sum(Dt * Dt, axis=0))
    pos = n > 0
    D_new = Dt.T.copy()
    D_new[pos] /= n[pos][:, None]
    x = x.copy()
    x[:, pos] *= n[pos]
    return x, D_new, float(np.max(np.abs(D - D_new)))


def hals_solve_np(y, D, x=None, tol=1e-3, maxiter=1000, trace=None):
    """nmf.solve(method='hals') restated: x = ones by default, D l2_strict normalised, then the MU loop's
    stop rule (it = 1 .. maxiter-1; (it, D_new, x) at the first max|D - D_new| < tol, else (maxiter, D, x))."""
    y = np.asarray(y, np.float64)
    D = np.asarray(D, np.float64)
    x = np.ones((y.shape[0], D.shape[0])) if x is None else np.asarray(x, np.float64)
    D = D / np.sqrt(np.sum(D * D, axis=1, keepdims=True))
    for it in range(1, maxiter):
        x, D_new, diff = hals_step_np(y, x, D)
        if trace is not None:
            trace.append(np.linalg.norm(y - x.dot(D_new)))
        if diff < tol:
            return it, D_new, x
        D = D_new
    return maxiter, D, x


def mu_solve_np(y, D, x, maxiter):
    """Plain multiplicative updates (the 'mu' method, l2), the same normalisation, maxiter-1 iterations."""
    y, D, x = (np.asarray(a, np.float64) for a in (y, D, x))
    D = D / np.sqrt(np.sum(D * D, axis=1, keepdims=True))
    for _ in range(1, maxiter):
        x = x * np.maximum(y.dot(D.T), 0) / np.maximum(x.dot(D.dot(D.T)), 1e-15)
        U = D * np.maximum(x.T.dot(y), 0) / np.maximum(x.T.dot(x).dot(D), 1e-15)
        D = U / np.sqrt(np.sum(U * U, axis=1, keepdims=True))
    return D, x


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


def _planted(N, F, K, seed):
    rng = np.random.RandomState(seed)
    x0 = rng.uniform(size=(N, K)) * (rng.uniform(size=(N, K)) < 0.5)
    D0 = rng.uniform(size=(K, F)) * (rng.uniform(size=(K, F)) < 0.5)
    return x0.dot(D0), rng.uniform(size=(K, F)) + 0.1


# ---- the sweep kernel ---------------------------------------------------------------------------------------
def _sweep_gpu(V, C, G, coord_major):
    """dcp_nn_cd_sweep_* on [R, K] NumPy V, C (passed as [K, R] when coord_major).  Returns [R, K]."""
    import torch
    from decomp_amd import _arrays, _hip
    lay = (lambda a: np.ascontiguousarray(a.T)) if coord_major else np.ascontiguousarray
    v = torch.from_numpy(lay(V)).cuda()
    c = torch.from_numpy(lay(C)).cuda()
    g = torch.from_numpy(np.ascontiguousarray(G)).cuda()
    out = torch.full_like(v, float('nan'))
    lib, h = _arrays.lib_handle(v)
    sfx = _arrays.suffix(v)
    R, K = V.shape
    _hip.check(h, getattr(lib, 'dcp_nn_cd_sweep_' + sfx)(h, _arrays.ptr(v), _arrays.ptr(out), _arrays.ptr(c),
                                                          _arrays.ptr(g), R, K, int(coord_major)),
               'dcp_nn_cd_sweep')
    torch.cuda.synchronize()
    o = out.cpu().numpy()
    return o.T if coord_major else o


def _sweep_case(R, K, seed, dtype):
    rng = np.random.RandomState(seed)
    B = rng.randn(K + 3, K)
    G = B.T.dot(B) / (K + 3)                      # symmetric positive semi-definite
    G[np.arange(3, K, 7), np.arange(3, K, 7)] = 0.0  # some G[k,k] = 0: those coordinates stay
    V = np.abs(rng.randn(R, K))
    C = rng.randn(R, K)                           # negative entries: the clamp at 0 is active
    return V.astype(dtype), C.astype(dtype), G.astype(dtype)


@pytest.mark.parametrize('dtype', [np.float32, np.float64])
@pytest.mark.parametrize('coord_major', [0, 1])
@pytest.mark.parametrize('R', [1, 63, 64, 65, 1000])
@pytest.mark.parametrize('K', [1, 31, 32, 33, 256, 640])
def test_sweep_matches_numpy(dtype, coord_major, R, K):
    V, C, G = _sweep_case(R, K, seed=R * 1000 + K, dtype=dtype)
    ref = sweep_np(V, C, G)
    got = _sweep_gpu(V, C, G, coord_major)
    assert np.all(np.isfinite(got))
    assert np.all(got >= 0)
    zero = np.diag(G) == 0
    assert np.array_equal(got[:, zero], V[:, zero])   # G[k,k] = 0: unchanged, bit for bit
    if R * K >= 1000:
        assert np.mean(ref == 0) > 0.05                # the clamp did act
    tol = 1e-5 if dtype == np.float32 else 1e-12
    assert _rel(got, ref) <= tol


def test_sweep_in_place_and_large_rows():
    """V_in == V_out, and R past the two-tile-per-wave threshold (32768 rows)."""
    import torch
    from decomp_amd import _arrays, _hip
    V, C, G = _sweep_case(40000, 48, seed=3, dtype=np.float32)
    ref = sweep_np(V, C, G)
    v = torch.from_numpy(V).cuda()
    c = torch.from_numpy(C).cuda()
    g = torch.from_numpy(G).cuda()
    lib, h = _arrays.lib_handle(v)
    _hip.check(h, lib.dcp_nn_cd_sweep_f32(h, _arrays.ptr(v), _arrays.ptr(v), _arrays.ptr(c), _arrays.ptr(g),
                                          40000, 48, 0), 'dcp_nn_cd_sweep')
    torch.cuda.synchronize()
    assert _rel(v.cpu().numpy(), ref) <= 1e-5


# ---- solve against the restatement ----------------------------------------------------------------------
@pytest.mark.parametrize('shape', [(64, 48, 4), (101, 20, 3), (300, 129, 37), (1000, 256, 64)])
def test_solve_f64_parity(shape):
    from decomp_amd import nmf
    N, F, K = shape
    y, D0 = _problem(N, F, K, seed=N + K)
    it, D, x = nmf.solve(y, D0.copy(), tol=0.0, maxiter=6, method='hals')
    ito, Do, xo = hals_solve_np(y, D0, tol=0.0, maxiter=6)
    assert it == ito == 6
    assert _rel(D, Do) <= 1e-10
    assert _rel(x, xo) <= 1e-10


@pytest.mark.parametrize('mode', [0, 1])
@pytest.mark.parametrize('shape', [(64, 48, 4), (300, 129, 37), (1024, 256, 64)])
def test_solve_f32_parity(shape, mode):
    import torch
    from decomp_amd import nmf, _arrays
    N, F, K = shape
    y, D0 = _problem(N, F, K, seed=N + K + 1, dtype=np.float32)
    lib, h = _arrays.lib_handle(torch.zeros(1, device='cuda'))
    prev = lib.dcp_set_f32_product_mode(h, mode)
    try:
        it, D, x = nmf.solve(y, D0.copy(), tol=0.0, maxiter=3, method='hals')
    finally:
        lib.dcp_set_f32_product_mode(h, prev)
    ito, Do, xo = hals_solve_np(y, D0, tol=0.0, maxiter=3)
    assert it == ito == 3
    assert D.dtype == np.float32 and x.dtype == np.float32
    assert _rel(D, Do) <= 2e-4
    assert _rel(x, xo) <= 2e-4


def test_loss_monotone_f64():
    from decomp_amd import nmf
    y, D0 = _problem(500, 200, 20, seed=7)
    D = nmf._arrays.to_device(D0 / np.sqrt(np.sum(D0 * D0, axis=1, keepdims=True)), copy=True)
    import torch
    x = torch.ones((500, 20), dtype=torch.float64, device=D.device)
    yd = nmf._arrays.to_device(y)
    trace = []
    it = nmf._run_hals(yd, x, D, 0.0, 31, resid_trace=trace)
    assert it == 31 and len(trace) == 30
    loss = np.array(trace) ** 2
    assert np.all(loss[1:] <= loss[:-1] * (1 + 1e-12))
    ref = []
    hals_solve_np(y, D0, tol=0.0, maxiter=31, trace=ref)
    assert _rel(trace, ref) <= 1e-10


def test_kkt_at_convergence():
    """min(v, df/dv) ~ 0 elementwise for x and D after many iterations (f = 1/2 |y - xD|^2)."""
    from decomp_amd import nmf
    y, D0 = _problem(120, 60, 5, seed=11, noise=0.02)
    it, D, x = nmf.solve(y, D0, tol=0.0, maxiter=1500, method='hals')
    r = x.dot(D) - y
    gx = r.dot(D.T)
    gD = x.T.dot(r)
    scale = np.max(np.abs(y)) * np.max(np.abs(D)) * y.shape[1]
    assert np.max(np.abs(np.minimum(x, gx))) <= 1e-6 * scale
    assert np.max(np.abs(np.minimum(D, gD))) <= 1e-6 * np.max(np.abs(y)) * np.max(np.abs(x)) * y.shape[0]


def test_faster_than_mu():
    """A planted non-negative problem, the same start, the same number of iterations: HALS's residual is
    below MU's, and the GPU agrees with the restatement on both."""
    from decomp_amd import nmf
    y, D0 = _planted(300, 129, 12, seed=0)
    x0 = np.ones((300, 12))
    _, Dh, xh = nmf.solve(y, D0.copy(), x=x0.copy(), tol=0.0, maxiter=51, method='hals')
    _, Dm, xm = nmf.solve(y, D0.copy(), x=x0.copy(), tol=0.0, maxiter=51, method='mu')
    rh = np.linalg.norm(y - xh.dot(Dh)) / np.linalg.norm(y)
    rm = np.linalg.norm(y - xm.dot(Dm)) / np.linalg.norm(y)
    Dmo, xmo = mu_solve_np(y, D0, x0, 51)
    rmo = np.linalg.norm(y - xmo.dot(Dmo)) / np.linalg.norm(y)
    assert abs(rm - rmo) <= 1e-8
    assert rh < 0.1 * rm, (rh, rm)


# ---- the return contract --------------------------------------------------------------------------------
def test_tol_reached_and_not():
    from decomp_amd import nmf
    y, D0 = _problem(200, 80, 6, seed=5)
    it, D, x = nmf.solve(y, D0.copy(), tol=1e-4, maxiter=500, method='hals')
    ito, Do, xo = hals_solve_np(y, D0, tol=1e-4, maxiter=500)
    assert it == ito and it < 500
    assert _rel(D, Do) <= 1e-9 and _rel(x, xo) <= 1e-9
    it, D, x = nmf.solve(y, D0.copy(), tol=1e-12, maxiter=4, method='hals')
    ito, Do, xo = hals_solve_np(y, D0, tol=1e-12, maxiter=4)
    assert it == ito == 4
    assert _rel(D, Do) <= 1e-10 and _rel(x, xo) <= 1e-10


def test_maxiter_one_returns_normalised_input():
    from decomp_amd import nmf
    y, D0 = _problem(50, 30, 4, seed=2)
    x0 = np.abs(np.random.RandomState(0).randn(50, 4))
    it, D, x = nmf.solve(y, D0.copy(), x=x0.copy(), maxiter=1, method='hals')
    assert it == 1
    np.testing.assert_allclose(D, D0 / np.sqrt(np.sum(D0 * D0, axis=1, keepdims=True)), rtol=1e-15)
    assert np.array_equal(x, x0)


@pytest.mark.parametrize('dtype', [np.float32, np.float64])
def test_result_properties_and_determinism(dtype):
    from decomp_amd import nmf
    y, D0 = _problem(700, 96, 10, seed=9, dtype=dtype)
    it1, D1, x1 = nmf.solve(y, D0.copy(), tol=0.0, maxiter=20, method='hals')
    it2, D2, x2 = nmf.solve(y, D0.copy(), tol=0.0, maxiter=20, method='hals')
    assert isinstance(D1, np.ndarray) and isinstance(x1, np.ndarray)
    assert D1.dtype == dtype and x1.dtype == dtype
    assert it1 == it2 == 20
    assert np.array_equal(D1, D2) and np.array_equal(x1, x2)
    assert np.all(D1 >= 0) and np.all(x1 >= 0)
    np.testing.assert_allclose(np.sqrt(np.sum(D1.astype(np.float64) ** 2, axis=1)), 1.0,
                               rtol=1e-5 if dtype == np.float32 else 1e-12)


def test_torch_in_torch_out():
    import torch
    from decomp_amd import nmf
    y, D0 = _problem(128, 64, 8, seed=4)
    yt = torch.from_numpy(y).cuda()
    Dt = torch.from_numpy(D0).cuda()
    it, D, x = nmf.solve(yt, Dt, tol=0.0, maxiter=4, method='hals')
    assert isinstance(D, torch.Tensor) and isinstance(x, torch.Tensor)
    assert D.is_cuda and x.is_cuda
    assert torch.equal(Dt, torch.from_numpy(D0).cuda())   # the caller's D is not modified
    ito, Do, xo = hals_solve_np(y, D0, tol=0.0, maxiter=4)
    assert _rel(_np(D), Do) <= 1e-10 and _rel(_np(x), xo) <= 1e-10


def test_zero_column_of_x_gives_no_nan():
    """A zero column of x makes its atom's D-side Gram entry zero: the atom stays (zero norm allowed)."""
    from decomp_amd import nmf
    y, D0 = _problem(90, 40, 5, seed=6)
    x0 = np.abs(np.random.RandomState(1).randn(90, 5))
    x0[:, 2] = 0.0
    it, D, x = nmf.solve(y, D0.copy(), x=x0.copy(), tol=0.0, maxiter=8, method='hals')
    ito, Do, xo = hals_solve_np(y, D0, x=x0, tol=0.0, maxiter=8)
    assert np.all(np.isfinite(D)) and np.all(np.isfinite(x))
    assert _rel(D, Do) <= 1e-10 and _rel(x, xo) <= 1e-10


# ---- what HALS does not cover ---------------------------------------------------------------------------
def test_errors():
    from decomp_amd import nmf
    y, D0 = _problem(40, 20, 3, seed=1)
    mask = np.ones_like(y)
    with pytest.raises(NotImplementedError):
        nmf.solve(y, D0, method='hals', mask=mask)
    with pytest.raises(NotImplementedError):
        nmf.solve(y, D0, method='hals', likelihood='kl')
    with pytest.raises(NotImplementedError):
        nmf.solve(y, D0, method='hals', likelihood='is')
    with pytest.raises(NotImplementedError):
        nmf.solve(y, D0, method='hals', minibatch=10)
    with pytest.raises(TypeError):
        nmf.solve(y, D0, method='hals', unknown=1)


# ---- one large run: many tiles, many blocks ---------------------------------------------------------------
def test_large_f32():
    from decomp_amd import nmf
    rng = np.random.RandomState(0)
    N, F, K = 16384, 4096, 256
    y = (np.maximum(rng.randn(N, K), 0).astype(np.float32).dot(
        np.maximum(rng.randn(K, F), 0).astype(np.float32)) / K).astype(np.float32)
    D0 = (np.abs(rng.randn(K, F)) + 0.1).astype(np.float32)
    it, D, x = nmf.solve(y, D0.copy(), tol=0.0, maxiter=3, method='hals')
    ito, Do, xo = hals_solve_np(y, D0, tol=0.0, maxiter=3)
    assert it == ito == 3
    # 256 strongly correlated atoms: the same two iterations in float32 NumPy differ from the float64
    # restatement by 2.6e-4 (D) and 1.4e-4 (x), so the bound is a few times that rounding floor
    assert _rel(D, Do) <= 1e-3
    assert _rel(x, xo) <= 1e-3
