"""GPU: the split-bf16 ("bf16x6") core for float32 products (gemm_mfma_bf16x6.hpp) and the NMF step that uses it.

The core splits each fp32 operand into three bf16 planes and sums six bf16 products in the fp32 accumulator.
Its error must stay of the fp32 core's size: elementwise |C - C64| / (|A||B|) no more than twice the exact fp32
MFMA core's on the same inputs."""

import numpy as np
import pytest

pytestmark = pytest.mark.gpu


def _lib_h():
    import torch
    from decomp_amd import _arrays
    return _arrays.lib_handle(torch.empty(1, device='cuda'))


def _run(fn_name, form, a, b, M, N, K, ksplits):
    import torch
    from decomp_amd import _arrays, _hip
    lib, h = _lib_h()
    c = torch.empty((M, N), dtype=torch.float32, device='cuda')
    args = [h, form, _arrays.ptr(a), _arrays.ptr(b), _arrays.ptr(c), M, N, K, ksplits]
    if fn_name == 'dcp_gemm_f32':
        args.append(0)
    _hip.check(h, getattr(lib, fn_name)(*args), fn_name)
    torch.cuda.synchronize()
    return c


def _operands(form, M, N, K, kind, seed):
    """Device operands of an NT (A[M,K], B[N,K]) or TN (A[K,M], B[K,N]) product."""
    import torch
    g = torch.Generator(device='cuda')
    g.manual_seed(seed)
    sa = (M, K) if form == 0 else (K, M)
    sb = (N, K) if form == 0 else (K, N)

    def make(shape, lo, hi):
        u = torch.rand(shape, generator=g, device='cuda', dtype=torch.float32)
        if kind == 'nonneg':
            return u + 0.01
        if kind == 'signed':
            return 2.0 * u - 1.0
        # 'wide': random sign, exponent uniform in [lo, hi], about 1 % exact zeros
        e = torch.randint(lo, hi + 1, shape, generator=g, device='cuda').to(torch.float32)
        s = torch.where(torch.rand(shape, generator=g, device='cuda') < 0.5, -1.0, 1.0)
        v = s * (1.0 + u) * torch.exp2(e)
        return torch.where(torch.rand(shape, generator=g, device='cuda') < 0.01, torch.zeros_like(v), v)

    # A over 2^-100 .. 2^100, B over 2^-20 .. 2^20: every product stays a normal float32
    return make(sa, -100, 100).contiguous(), make(sb, -20, 20).contiguous()


def _rel_err(form, a, b, c, rows, cols):
    """max over the sampled outputs of |C - C64| / (|A||B|), in float64 on the host."""
    A = a.cpu().numpy().astype(np.float64)
    B = b.cpu().numpy().astype(np.float64)
    if form == 0:
        Ar, Bc = A[rows], B[cols]
        ref = Ar @ Bc.T
        bound = np.abs(Ar) @ np.abs(Bc).T
    else:
        Ar, Bc = A[:, rows], B[:, cols]
        ref = Ar.T @ Bc
        bound = np.abs(Ar).T @ np.abs(Bc)
    C = c.cpu().numpy()[np.ix_(rows, cols)].astype(np.float64)
    keep = bound > 0
    assert keep.any()
    return float(np.max(np.abs(C - ref)[keep] / bound[keep]))


def _sample(n, k, rng):
    if n <= k:
        return np.arange(n)
    return np.unique(np.concatenate([np.arange(64), n - 64 + np.arange(64), rng.choice(n, k - 128, replace=False)]))


CASES = [
    # form, M, N, K, ksplits
    (0, 65536, 256, 4096, 1),    # the NMF x update, Y . D^T (256 x 256 tiles)
    (0, 8192, 256, 4096, 8),     # the same product split over F (one shard of a multi-GPU run)
    (0, 4096, 2048, 512, 1),     # 128 x 128 tiles
    (2, 256, 4352, 65536, 15),   # the statistics product x^T [Y | x], split over the samples
    (2, 256, 2048, 16384, 4),
    (2, 2048, 4096, 256, 1),
]


@pytest.mark.parametrize('kind', ['nonneg', 'signed', 'wide'])
@pytest.mark.parametrize('case', CASES, ids=lambda c: 'f%d_%dx%dx%d_s%d' % c)
def test_error_within_twice_fp32(case, kind):
    form, M, N, K, ks = case
    a, b = _operands(form, M, N, K, kind, seed=M + N + K + ks)
    c6 = _run('dcp_gemm_bf16x6_f32', form, a, b, M, N, K, ks)
    c32 = _run('dcp_gemm_f32', form, a, b, M, N, K, ks)
    rng = np.random.RandomState(1)
    rows, cols = _sample(M, 512, rng), _sample(N, 512, rng)
    e6 = _rel_err(form, a, b, c6, rows, cols)
    e32 = _rel_err(form, a, b, c32, rows, cols)
    assert np.isfinite(e6) and e6 <= 2.0 * e32 + 1e-9, (case, kind, e6, e32)
    assert e6 < 1e-5, (case, kind, e6)


def test_zeros_and_exact_values():
    """Zero operands give exact zeros; small integers (exact in bf16) give the exact product."""
    import torch
    M, N, K = 8192, 1024, 256     # 128 x 128 tiles
    z = torch.zeros((M, K), device='cuda')
    b = torch.rand((N, K), device='cuda')
    assert torch.count_nonzero(_run('dcp_gemm_bf16x6_f32', 0, z, b, M, N, K, 1)).item() == 0
    g = torch.Generator(device='cuda')
    g.manual_seed(3)
    ai = torch.randint(-8, 9, (M, K), generator=g, device='cuda').float()
    bi = torch.randint(-8, 9, (N, K), generator=g, device='cuda').float()
    c = _run('dcp_gemm_bf16x6_f32', 0, ai, bi, M, N, K, 1)
    ref = ai.cpu().numpy().astype(np.int64) @ bi.cpu().numpy().astype(np.int64).T
    assert np.array_equal(c.cpu().numpy().astype(np.int64), ref)


@pytest.mark.parametrize('case', [(0, 65536, 256, 4096, 1), (2, 256, 4352, 65536, 15)],
                         ids=['nt', 'tn_split'])
def test_bitwise_rerun(case):
    import torch
    form, M, N, K, ks = case
    a, b = _operands(form, M, N, K, 'signed', seed=11)
    c0 = _run('dcp_gemm_bf16x6_f32', form, a, b, M, N, K, ks)
    for _ in range(2):
        assert torch.equal(c0, _run('dcp_gemm_bf16x6_f32', form, a, b, M, N, K, ks))


def test_unsupported_shape_is_an_error():
    import torch
    from decomp_amd import _arrays
    lib, h = _lib_h()
    a = torch.rand((100, 64), device='cuda')
    b = torch.rand((128, 64), device='cuda')
    c = torch.empty((100, 128), device='cuda')
    rc = lib.dcp_gemm_bf16x6_f32(h, 0, _arrays.ptr(a), _arrays.ptr(b), _arrays.ptr(c), 100, 128, 64, 1)
    assert rc != 0
    assert lib.dcp_gemm_bf16x6_f32(h, 1, _arrays.ptr(a), _arrays.ptr(b), _arrays.ptr(c), 128, 128, 64, 1) != 0


class _Mode:
    """dcp_set_f32_product_mode on the device-0 handle for the duration of a block."""

    def __init__(self, mode):
        self.mode = mode

    def __enter__(self):
        lib, h = _lib_h()
        self.prev = lib.dcp_set_f32_product_mode(h, self.mode)
        assert self.prev in (0, 1)

    def __exit__(self, *exc):
        lib, h = _lib_h()
        lib.dcp_set_f32_product_mode(h, self.prev)


def test_mode_switch_default_and_query():
    lib, h = _lib_h()
    assert lib.dcp_set_f32_product_mode(h, -1) == 0          # the default is the split-bf16 core
    assert lib.dcp_set_f32_product_mode(h, 1) == 0
    assert lib.dcp_set_f32_product_mode(h, -1) == 1
    assert lib.dcp_set_f32_product_mode(h, 0) == 1
    assert lib.dcp_set_f32_product_mode(h, 2) < 0
    assert lib.dcp_set_f32_product_mode(None, 0) < 0


def test_golden_solve_same_stop_iteration_both_modes():
    """The golden fixtures' solves stop at the same iteration in both product modes.  These shapes are far below a
    whole bf16x6 tile, so both modes run the fp32 core here and this only checks that the mode switch changes
    nothing else; test_gpu_bf16x6_loop.py compares the stop iteration at a shape that takes the core."""
    import decomp_amd
    import os
    g = np.load(os.path.join(os.path.dirname(os.path.abspath(__file__)), 'golden', 'nmf_golden.npz'))
    for case in ('nmf_64x48k4', 'nmf_101x20k3', 'nmf_256x128k8'):
        base = '%s_float32_l2' % case
        name = base + '_nomask'
        y, D0 = g[base + '/y'], g[base + '/D0']
        out = []
        for mode in (0, 1):
            with _Mode(mode):
                out.append(decomp_amd.nmf.solve(y, D0.copy(), tol=float(g[name + '/tol']), maxiter=400,
                                                method='mu', likelihood='l2', random_seed=0))
        assert out[0][0] == out[1][0], (case, out[0][0], out[1][0])


def _trace(y, D0, n):
    import torch
    from decomp_amd import _arrays, nmf as hnmf
    yd = y
    Dd = D0.clone()
    _arrays.l2_normalize_(Dd, strict=True)
    xd = torch.ones((y.shape[0], D0.shape[0]), dtype=yd.dtype, device='cuda')
    trace = []
    it = hnmf._run_mu(yd, None, xd, Dd, hnmf._likelihood_code('l2'), 0.0, n + 1, resid_trace=trace)
    assert it == n + 1
    return Dd, xd, np.array(trace)


def test_c2_residual_trace_both_modes():
    """The headline shape (Y 65536 x 4096, k = 256), 25 iterations: per-iteration residuals of the two product
    modes agree to 1e-6 relative, and both products take the bf16x6 path only in mode 0."""
    import torch
    N, F, K = 65536, 4096, 256
    g = torch.Generator(device='cuda')
    g.manual_seed(0)
    xt = torch.relu(torch.randn((N, K), generator=g, device='cuda')) * 0.1
    Dt = torch.randn((K, F), generator=g, device='cuda').abs()
    y = xt @ Dt + 0.1 * torch.randn((N, F), generator=g, device='cuda').abs()
    D0 = (Dt + 0.3 * torch.randn((K, F), generator=g, device='cuda')).abs() + 0.1
    del xt, Dt
    res = []
    for mode in (0, 1):
        with _Mode(mode):
            D, x, r = _trace(y, D0, 25)
        res.append(r)
        del D, x
        torch.cuda.empty_cache()
    rel = np.abs(res[0] - res[1]) / res[1]
    assert np.max(rel) <= 1e-6, rel
