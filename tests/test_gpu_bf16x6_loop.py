"""GPU: the float32 MU loop (dcp_nmf_mu_f32) with both large products on the split-bf16 core (product mode 0).

Shapes where nmf_stats puts both Y . D^T and x^T [Y | x] on the core (see the path table of
test_gpu_bf16x6_paths.py):
  65536 x 1024, 256 atoms: Y . D^T on 256 x 256 tiles with the fused quotient; x^T [Y | x] on the 256 x 256 TN tile
                           (plan_splits_x6_tn: 5 tiles, 51 splits of 1296).
  16384 x 1024, 128 atoms: Y . D^T split over F on 128 x 128 tiles, EpiMuDenSlabs; x^T [Y | x] on 128 x 128.
Each iteration is compared with oracle.nmf.mu_step (the reference's formulation in NumPy) with the tolerances of
test_gpu_tile_tiers.py; and the stop iteration of a converging solve is compared between the two product modes."""
import ctypes

import numpy as np
import pytest

from test_gpu_nmf_bf16x6 import _Mode

pytestmark = pytest.mark.gpu

SHAPES = [(65536, 1024, 256), (16384, 1024, 128)]


def _problem(N, F, K, seed):
    rng = np.random.RandomState(seed)
    xt = np.maximum(rng.randn(N, K), 0).astype(np.float32)
    Dt = np.maximum(rng.randn(K, F), 0).astype(np.float32)
    y = xt.dot(Dt) + 0.1 * np.abs(rng.randn(N, F)).astype(np.float32)
    d0 = np.maximum(Dt + 0.3 * rng.randn(K, F), 0.1).astype(np.float32)
    return y.astype(np.float32), d0


def _residual(yg, x, d):
    """||Y - x D||_F in float64 on the device (x, d: device tensors or host arrays)."""
    import torch
    x = torch.as_tensor(x, device='cuda').double()
    d = torch.as_tensor(d, device='cuda').double()
    return float(torch.linalg.norm(yg.double() - x @ d))


def _mu(lib, h, Yg, xg, Dg, tol, maxiter):
    from decomp_amd import _arrays, _hip
    N, F = Yg.shape
    K = Dg.shape[0]
    it = ctypes.c_int(0)
    md = ctypes.c_float(0.0)
    _hip.check(h, lib.dcp_nmf_mu_f32(h, _arrays.ptr(Yg), None, _arrays.ptr(xg), _arrays.ptr(Dg), N, F, K,
                                     _hip.LIK_L2, ctypes.c_float(tol), maxiter, ctypes.byref(it), ctypes.byref(md),
                                     None), 'dcp_nmf_mu_f32')
    return it.value, md.value


@pytest.mark.parametrize('shape', SHAPES, ids=lambda s: '%dx%dk%d' % s)
def test_mu_iterations_on_core_match_oracle(shape):
    import torch
    from decomp_amd import _arrays
    from oracle import nmf as onmf, common
    N, F, K = shape
    y, d0 = _problem(N, F, K, seed=N + F + K)
    Yg, Dg = torch.from_numpy(y).cuda(), torch.from_numpy(d0).cuda()
    _arrays.l2_normalize_(Dg, strict=True)
    xg = torch.ones((N, K), device='cuda')
    lib, h = _arrays.lib_handle(Yg)
    x, d = np.ones((N, K), np.float32), common.l2_strict(d0)
    tol_r, tol_d, tol_x = 2e-5, 2e-4, 2e-4
    with _Mode(0):
        for step in range(4):
            _mu(lib, h, Yg, xg, Dg, 0.0, 2)          # one iteration
            x, d, _ = onmf.mu_step(y, x, d)
            torch.cuda.synchronize()
            r_cpu = _residual(Yg, x, d)
            r_hip = _residual(Yg, xg, Dg)
            assert abs(r_hip - r_cpu) <= tol_r * r_cpu, (shape, step, r_hip, r_cpu)
            dd = float(np.max(np.abs(Dg.cpu().numpy() - d)))
            dx = float(np.max(np.abs(xg.cpu().numpy() - x)) / max(1.0, float(np.max(np.abs(x)))))
            assert dd <= tol_d and dx <= tol_x, (shape, step, dd, dx)
    del Yg, Dg, xg
    torch.cuda.empty_cache()


def _trace(lib, h, Yg, x0, D0, n):
    """max|dD| of iterations 1 .. n, one dcp_nmf_mu_f32 call per iteration (the same kernels as one solve)."""
    x, D = x0.clone(), D0.clone()
    return np.array([_mu(lib, h, Yg, x, D, 0.0, 2)[1] for _ in range(n)], dtype=np.float64)


def test_stop_iteration_both_modes_on_core():
    """65536 x 1024, 256 atoms, started near the planted factors so that max|dD| decays.  Both modes' max|dD| traces
    must agree to 1 %; the tolerance is then placed where both traces first cross it at the same iteration t
    (10 <= t <= 50) with the widest margin, and a solve in each mode must stop at t."""
    import torch
    from decomp_amd import _arrays
    N, F, K = 65536, 1024, 256
    rng = np.random.RandomState(5)
    xt = np.maximum(rng.randn(N, K), 0).astype(np.float32)
    Dt = np.maximum(rng.randn(K, F), 0).astype(np.float32) + 0.05
    y = (xt.dot(Dt) + 0.1 * np.abs(rng.randn(N, F))).astype(np.float32)
    scale = np.sqrt(np.sum(Dt.astype(np.float64) ** 2, axis=1)).astype(np.float32)
    Yg = torch.from_numpy(y).cuda()
    lib, h = _arrays.lib_handle(Yg)
    D0 = torch.from_numpy(np.abs(Dt + 0.05 * rng.randn(K, F)).astype(np.float32)).cuda()
    _arrays.l2_normalize_(D0, strict=True)
    x0 = torch.from_numpy(((xt + 0.1) * scale).astype(np.float32)).cuda()
    traces = []
    for mode in (0, 1):
        with _Mode(mode):
            traces.append(_trace(lib, h, Yg, x0, D0, 55))
    t0, t1 = traces
    agree = float(np.max(np.abs(t0 - t1) / t1))
    assert agree <= 1e-2, (agree, t0, t1)
    # stopping at iteration t needs trace[t-1] < tol <= min(trace[:t-1]) in both modes
    best = None
    for t in range(10, 51):
        hi = min(float(np.min(t0[:t - 1])), float(np.min(t1[:t - 1])))
        lo = max(float(t0[t - 1]), float(t1[t - 1]))
        if lo < hi and (best is None or hi / lo > best[1]):
            best = (t, hi / lo, float(np.sqrt(hi * lo)))
    assert best is not None and best[1] >= 1.01, (best, t0, t1)
    t, _, tol = best
    stops = []
    for mode in (0, 1):
        with _Mode(mode):
            stops.append(_mu(lib, h, Yg, x0.clone(), D0.clone(), tol, 200)[0])
    print('\nstop test: traces agree to %.2g, tol %.4g, margin %.4f, stops %s (expected %d)' % (agree, tol, best[1], stops, t))
    assert stops == [t, t], (stops, t, tol, t0[t - 3:t + 2], t1[t - 3:t + 2])
    del Yg, x0, D0
    torch.cuda.empty_cache()
