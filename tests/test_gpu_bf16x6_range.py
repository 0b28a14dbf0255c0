"""GPU: the operand magnitude range of the split-bf16 ("bf16x6") core, through dcp_gemm_bf16x6_f32.

The core splits a float32 operand into three bf16 planes h + m + l (gemm_mfma_bf16x6.hpp).  bf16 has the exponent
range of float32, so the planes need no scaling, but the lower planes of a tiny operand fall below the smallest
normal bf16 (2^-126): m ~ 2^-9 |a| for |a| < 2^-117, l ~ 2^-18 |a| for |a| < 2^-108, and bf16 subnormals sit on a
2^-133 grid.  The split then keeps a to within about 2^-134 absolutely instead of 2^-27 |a| relatively, so every
output carries, besides the fp32-size relative term, an absolute floor of 2^-133 per unit of the other operand's
row or column sum:

    |C - C64| <= 2 e32 (|A||B|) + 2^-133 (sum_k |a_ik| + sum_k |b_kj|)

where e32 is the largest |C - C64| / (|A||B|) of the exact fp32 MFMA core on the same inputs.  The sweep below
covers one operand at 2^-96 .. 2^-126 (the other scaled so that every product and C stay normal float32), both
operands, both forms and both tiles, a tiny row among O(1) rows, float32 subnormals, exact zeros, and the upper end
of the range (operands above the largest bf16 overflow the split)."""

import numpy as np
import pytest

from test_gpu_nmf_bf16x6 import _run, _sample

pytestmark = pytest.mark.gpu

EXPONENTS = [-96, -100, -104, -108, -110, -113, -116, -120, -124, -126]
FLOOR = 2.0 ** -133      # absolute error per unit of sum |other operand| (bf16 subnormal grid)

# form, M, N, K, ksplits: the tile each one takes is fixed by x6_tier (gemm.hpp)
CONFIGS = {
    'nt256': (0, 8192, 1536, 256, 1),      # TIER_HUGE: 32 x 6 = 192 tiles of 256 x 256
    'nt128': (0, 4096, 2048, 512, 1),      # 128 tiles of 256 x 256 < 192: TIER_LARGE, 128 x 128
    'tn256': (2, 256, 1280, 32768, 8),     # 8 splits of 4096 (>= 1024 deep), whole 256-tiles: the TN 256 x 256 tile
    'tn128': (2, 2048, 4096, 256, 1),      # unsplit, 256 deep (< 1024): the TN 128 x 128 tile
}


def _shapes(form, M, N, K):
    return ((M, K), (N, K)) if form == 0 else ((K, M), (K, N))


def _mag(shape, e, g):
    """Random sign, mantissa uniform in [1, 2), exponent e (exact: powers of two scale exactly)."""
    import torch
    u = torch.rand(shape, generator=g, device='cuda', dtype=torch.float32)
    s = torch.where(torch.rand(shape, generator=g, device='cuda') < 0.5, -1.0, 1.0)
    return (s * (1.0 + u)) * (2.0 ** e)


def _errors(form, a, b, c, rows, cols):
    """|C - C64|, |A||B| and sum|a| + sum|b| at the sampled outputs, float64 on the device."""
    import torch
    r = torch.as_tensor(rows, device='cuda')
    q = torch.as_tensor(cols, device='cuda')
    if form == 0:
        Ar, Bc = a[r].double(), b[q].double().T          # [m, K], [K, n]
    else:
        Ar, Bc = a[:, r].double().T, b[:, q].double()
    ref = Ar @ Bc
    bound = Ar.abs() @ Bc.abs()
    sums = Ar.abs().sum(1, keepdim=True) + Bc.abs().sum(0, keepdim=True)
    err = (c[r][:, q].double() - ref).abs()
    return err, bound, sums


def _rel(err, bound):
    keep = bound > 0
    assert bool(keep.any())
    return float((err[keep] / bound[keep]).max())


def _excess(err, bound, sums):
    """max of (|C - C64| - FLOOR (sum|a| + sum|b|)) / (|A||B|): the relative part of the error once the floor is
    granted (negative where the floor alone covers it)."""
    keep = bound > 0
    return float(((err - FLOOR * sums)[keep] / bound[keep]).max())


@pytest.mark.parametrize('tiny', ['A', 'B'])
@pytest.mark.parametrize('cfg', list(CONFIGS), ids=list(CONFIGS))
def test_exponent_sweep(cfg, tiny):
    """One operand at 2^e (e = -96 .. -126), the other at 2^(-e-20): products about 2^-20, C normal."""
    import torch
    form, M, N, K, ks = CONFIGS[cfg]
    sa, sb = _shapes(form, M, N, K)
    rng = np.random.RandomState(3)
    rows, cols = _sample(M, 256, rng), _sample(N, 256, rng)
    table = []
    for e in EXPONENTS:
        g = torch.Generator(device='cuda')
        g.manual_seed(1000 - e)
        ea, eb = (e, -e - 20) if tiny == 'A' else (-e - 20, e)
        a, b = _mag(sa, ea, g).contiguous(), _mag(sb, eb, g).contiguous()
        c6 = _run('dcp_gemm_bf16x6_f32', form, a, b, M, N, K, ks)
        c32 = _run('dcp_gemm_f32', form, a, b, M, N, K, ks)
        err6, bound, sums = _errors(form, a, b, c6, rows, cols)
        err32, _, _ = _errors(form, a, b, c32, rows, cols)
        e6, e32, x6 = _rel(err6, bound), _rel(err32, bound), _excess(err6, bound, sums)
        table.append((e, e6, e32, x6))
        assert bool(torch.isfinite(c6).all()), (cfg, tiny, e)
        assert x6 <= 2.0 * e32 + 1e-9, (cfg, tiny, e, e6, e32, x6)
        assert e32 < 1e-5, (cfg, tiny, e, e32)
        del a, b, c6, c32
    print('\n%s tiny %s: e, max|C-C64|/(|A||B|) bf16x6, fp32 core, bf16x6 beyond the floor' % (cfg, tiny))
    for row in table:
        print('  %5d  %.3g  %.3g  %.3g' % row)
    # above 2^-100 the floor is below the fp32 rounding of these sums: the plain relative bound holds there
    for e, e6, e32, _ in table:
        if e >= -100:
            assert e6 <= 2.0 * e32 + 1e-9, (cfg, tiny, e, e6, e32)


@pytest.mark.parametrize('cfg', ['nt256', 'tn256', 'nt128', 'tn128'])
def test_dead_row_among_live_rows(cfg):
    """A few rows of A at 2^-120 (a dead atom of x), the rest O(1), B O(1): the live rows keep the plain relative
    bound, the dead rows the bound with the floor.  An all-zero row next to them gives exact zeros."""
    import torch
    form, M, N, K, ks = CONFIGS[cfg]
    sa, sb = _shapes(form, M, N, K)
    g = torch.Generator(device='cuda')
    g.manual_seed(17)
    a = _mag(sa, 0, g)
    b = _mag(sb, 0, g).contiguous()
    dead = [5, M // 2 + 37, M - 1]
    zero = 6
    tiny = _mag(sa, -120, g)
    if form == 0:
        a[dead] = tiny[dead]
        a[zero] = 0.0
    else:
        a[:, dead] = tiny[:, dead]
        a[:, zero] = 0.0
    a = a.contiguous()
    c6 = _run('dcp_gemm_bf16x6_f32', form, a, b, M, N, K, ks)
    c32 = _run('dcp_gemm_f32', form, a, b, M, N, K, ks)
    rng = np.random.RandomState(4)
    cols = _sample(N, 256, rng)
    live = np.setdiff1d(_sample(M, 256, rng), dead + [zero])
    err6, bound, _ = _errors(form, a, b, c6, live, cols)
    err32, _, _ = _errors(form, a, b, c32, live, cols)
    e6, e32 = _rel(err6, bound), _rel(err32, bound)
    assert e6 <= 2.0 * e32 + 1e-9, (cfg, 'live', e6, e32)
    err6, bound, sums = _errors(form, a, b, c6, np.array(dead), cols)
    err32, _, _ = _errors(form, a, b, c32, np.array(dead), cols)
    e32d = _rel(err32, bound)
    print('\n%s dead rows: bf16x6 %.3g (beyond the floor %.3g), fp32 core %.3g' %
          (cfg, _rel(err6, bound), _excess(err6, bound, sums), e32d))
    assert _excess(err6, bound, sums) <= 2.0 * e32d + 1e-9, (cfg, 'dead')
    assert torch.count_nonzero(c6[zero]).item() == 0


@pytest.mark.parametrize('cfg', ['nt256', 'tn256'])
def test_float32_subnormals_and_zeros(cfg):
    """A mixes float32 subnormals (2^-149 .. 2^-127), tiny normals (2^-126 .. 2^-110) and exact zeros; B at
    2^100 .. 2^110, so that every product is a normal float32."""
    import torch
    form, M, N, K, ks = CONFIGS[cfg]
    sa, sb = _shapes(form, M, N, K)
    g = torch.Generator(device='cuda')
    g.manual_seed(23)
    u = torch.rand(sa, generator=g, device='cuda')
    e = torch.where(u < 0.4, torch.randint(-149, -126, sa, generator=g, device='cuda'),
                    torch.randint(-126, -109, sa, generator=g, device='cuda')).float()
    s = torch.where(torch.rand(sa, generator=g, device='cuda') < 0.5, -1.0, 1.0)
    # mantissa on a 2^-20 grid times 2^e (subnormals round to the 2^-149 grid; the references read A as stored)
    m = 1.0 + torch.floor(torch.rand(sa, generator=g, device='cuda') * 2 ** 20) * 2.0 ** -20
    a = s * m * torch.exp2(e)
    a = torch.where(u > 0.8, torch.zeros_like(a), a).contiguous()
    assert bool(((a != 0) & (a.abs() < 2.0 ** -126)).any())            # subnormals really are there
    b = _mag(sb, 100, g) * torch.exp2(torch.randint(0, 11, sb, generator=g, device='cuda').float())
    b = b.contiguous()
    c6 = _run('dcp_gemm_bf16x6_f32', form, a, b, M, N, K, ks)
    c32 = _run('dcp_gemm_f32', form, a, b, M, N, K, ks)
    rng = np.random.RandomState(5)
    rows, cols = _sample(M, 256, rng), _sample(N, 256, rng)
    err6, bound, sums = _errors(form, a, b, c6, rows, cols)
    err32, _, _ = _errors(form, a, b, c32, rows, cols)
    e32 = _rel(err32, bound)
    print('\n%s subnormal A: bf16x6 %.3g (beyond the floor %.3g), fp32 core %.3g' %
          (cfg, _rel(err6, bound), _excess(err6, bound, sums), e32))
    assert bool(torch.isfinite(c6).all())
    assert _excess(err6, bound, sums) <= 2.0 * e32 + 1e-9, cfg


@pytest.mark.parametrize('cfg', ['nt256', 'tn128'])
def test_above_largest_bf16_is_not_finite(cfg):
    """an operand above the largest bf16 (about 3.39e38) rounds to infinity in the split, so the
    outputs it feeds are not finite, where the fp32 core's are.  Pinned so that a change shows."""
    import torch
    form, M, N, K, ks = CONFIGS[cfg]
    sa, sb = _shapes(form, M, N, K)
    g = torch.Generator(device='cuda')
    g.manual_seed(29)
    a = _mag(sa, 0, g)
    b = _mag(sb, -40, g).contiguous()
    big = 3.4e38                                    # finite float32, above bf16's 3.3895e38
    assert np.isfinite(np.float32(big))
    r = 7
    if form == 0:
        a[r, 3] = big
    else:
        a[3, r] = big
    a = a.contiguous()
    c6 = _run('dcp_gemm_bf16x6_f32', form, a, b, M, N, K, ks)
    c32 = _run('dcp_gemm_f32', form, a, b, M, N, K, ks)
    assert bool(torch.isfinite(c32).all())
    assert not bool(torch.isfinite(c6[r]).any())
    others = torch.ones(M, dtype=torch.bool, device='cuda')
    others[r] = False
    assert bool(torch.isfinite(c6[others]).all())
