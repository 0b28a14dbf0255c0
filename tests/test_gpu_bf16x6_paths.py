"""GPU: every path the float32 NMF step takes for its two large products, through dcp_nmf_mu_stats_f32.

The step (nmf_stats, nmf_impl.hpp) computes, on the l2 no-mask (Gram) path,
    X_out = X o max(Y . D^T, 0) / max(X . (D . D^T), eps)        the x update
    stats = X_out^T [Y | X_out]                                  the statistics product
and runs Y . D^T and X_out^T [Y | X_out] on the split-bf16 core (gemm_mfma_bf16x6.hpp) in product mode 0 when the
shape has a bf16x6 form, on the fp32 MFMA core otherwise and always in mode 1.  Each case below calls the entry in
both modes on the same inputs and compares both outputs elementwise with float64:
  X_out against the formula above, from the same float32 inputs;
  stats against X_out^T [Y | X_out] from that mode's own X_out (so the two products' errors stay apart).
All operands are positive, so |A||B| is the reference itself and the metric is the plain relative error.

The path each case claims is checked at run time: the two modes run identical code exactly when a product does not
take the core, so X_out is bitwise equal across modes if and only if the x update is on the fp32 core.  The
statistics product is checked the same way with integer Y and D: every x-update product is then exact in both
cores, X_out is bitwise equal, and stats is bitwise equal if and only if the statistics product is on the fp32
core."""

import numpy as np
import pytest

from test_gpu_bf16x6_range import FLOOR
from test_gpu_nmf_bf16x6 import _Mode, _lib_h, _sample

pytestmark = pytest.mark.gpu

CAP = 1e-5      # both modes, elementwise relative error (as test_gpu_nmf_bf16x6.py)
# Mode 0 may exceed twice mode 1's largest error by this much.  The statistics product sums 65536 positive terms;
# there the core's largest error has measured up to 2.2x the fp32 core's (2.6e-6 against 1.2e-6 at the headline
# shape), both far below CAP.
SLACK = 5e-7

# Paths, from pick_tier, x6_tier, nmf_xupdate_splits (nmf_impl.hpp) and plan_splits_x6_tn (gemm.hpp).
# x update Y . D^T (NT, M = N rows, N = K atoms, reduction F):
#   nmf_xupdate_splits plans 256 x 256 tiles when pick_tier says TIER_HUGE; it splits F only when there are fewer
#   than 192 such tiles (N / 256 * K / 256 < 192, i.e. N < 49152 at K = 256): then EpiSlab writes split slabs and
#   either EpiMuDenSlabs (out of place: `split_gram`) or mu_quotient_slabs_kernel (in place) forms the quotient;
#   unsplit, EpiMuNum fuses the quotient, always in its 16-byte form on the core.  x6_tier takes 256 x 256 when the
#   rows and atoms are whole 256-tiles, 128 x 128 when they are whole 128-tiles, and needs F % 16 == 0 and 16-byte
#   aligned operands; otherwise (65520 rows, F = 4104, Y 4 bytes off) the fp32 core runs.
# statistics X^T [Y | X] (TN, M = K, N = F + K in two B segments, reduction over the N rows):
#   plan_splits_x6_tn plans one round of 256 x 256 workgroups when K and F are whole 256-tiles and every split is
#   at least 1024 deep; 65536 rows: 17 tiles -> 15 splits of 4384; 16384 rows: 15 splits of 1104.  It plans from
#   shape alone.  Otherwise plan_splits plans for the fp32 tiles (8192 rows: 15 splits of 560 < 1024) and x6_tier
#   takes 128 x 128 where the segments are whole 128-tiles.  K >= 512 gives TIER_HUGE_DEEP, which has no bf16x6
#   form; F % 128 != 0 leaves the first segment ragged.
# name, rows, F, atoms, layout ('oop': X_out separate, 'inplace': X_out is X, 'misaligned': Y starts 4 bytes past
# a 16-byte boundary), x update on the core, statistics on the core
CASES = [
    # 256 tiles of 256 x 256, unsplit: fused EpiMuNum | TN 256 x 256, 15 splits, two segments
    ('x256_epimunum', 65536, 4096, 256, 'oop', True, True),
    ('x256_epimunum_inplace', 65536, 4096, 256, 'inplace', True, True),
    # 64 tiles: split F (4), EpiSlab then EpiMuDenSlabs | TN 256 x 256 on its own plan (15 x 1104)
    ('x256_split_dens', 16384, 4096, 256, 'oop', True, True),
    # in place: EpiSlab then mu_quotient_slabs_kernel | the same TN plan
    ('x256_split_inplace', 16384, 4096, 256, 'inplace', True, True),
    # 32 tiles: split F (8), EpiMuDenSlabs | plan_splits_x6_tn rejects (560-deep splits): fp32 plan, TN 128 x 128
    ('x256_split_tn128', 8192, 4096, 256, 'oop', True, True),
    # TIER_LARGE, 512 tiles of 128 x 128: EpiMuNum on 128 x 128 | K = 128 is no 256-tile: TN 128 x 128
    ('x128_k128', 65536, 4096, 128, 'oop', True, True),
    # TIER_HUGE, but 384 atoms are no whole 256-tiles: NT 128 x 128 | TN 128 x 128
    ('x128_k384', 65536, 4096, 384, 'oop', True, True),
    # 256 x 256 EpiMuNum | F = 1152 is a multiple of 128, not of 256: TN 128 x 128
    ('x256_tn128_f1152', 65536, 1152, 256, 'oop', True, True),
    # NT 256 x 256 | K = 512: TIER_HUGE_DEEP, fp32 core
    ('tn_fp32_k512', 65536, 4096, 512, 'oop', True, False),
    # 65520 rows are no whole 256-tiles: NT fp32 | TN 256 x 256 (15 splits of 4368)
    ('nt_fp32_ragged_rows', 65520, 4096, 256, 'oop', False, True),
    # NT 256 x 256 (F % 16 == 0) | F % 128 != 0: TN fp32
    ('tn_fp32_f4000', 65536, 4000, 256, 'oop', True, False),
    # F % 16 != 0: both fp32
    ('both_fp32_f4104', 65536, 4104, 256, 'oop', False, False),
    # Y 4 bytes off: NT fp32; TN fp32 too, but mode 0 plans its splits with plan_splits_x6_tn (shape only) and
    # mode 1 with plan_splits.  Both give 15 splits of 4384 here, but nothing ties the two plans together, so the two
    # fp32 runs may sum in a different order: stats held to the bound only
    ('misaligned_y', 65536, 4096, 256, 'misaligned', False, False),
]


def _y(N, F, misaligned, fill):
    import torch
    if not misaligned:
        return fill(torch.empty((N, F), device='cuda'))
    buf = torch.empty(N * F + 1, device='cuda')
    y = buf[1:].view(N, F)
    assert y.data_ptr() % 16 == 4
    return fill(y)


def _step(Y, X, D, layout):
    """(X_out, stats) of one dcp_nmf_mu_stats_f32 call; X is left as it was."""
    import torch
    from decomp_amd import _arrays, _hip
    lib, h = _lib_h()
    N, F = Y.shape
    K = D.shape[0]
    stats = torch.empty((K, F + K), device='cuda')
    if layout == 'inplace':
        xo = X.clone()
        xi = xo
    else:
        xo = torch.empty_like(X)
        xi = X
    _hip.check(h, lib.dcp_nmf_mu_stats_f32(h, _arrays.ptr(Y), None, _arrays.ptr(xi), _arrays.ptr(xo),
                                            _arrays.ptr(D), N, F, K, _hip.LIK_L2, _arrays.ptr(stats)),
               'dcp_nmf_mu_stats_f32')
    torch.cuda.synchronize()
    return xo, stats


def _both_modes(Y, X, D, layout):
    out = []
    for mode in (0, 1):
        with _Mode(mode):
            out.append(_step(Y, X, D, layout))
    return out


def _x_ref(Y, X, D, rows):
    """float64 X o max(Y D^T, 0) / max(X (D D^T), eps) at the sampled rows."""
    import torch
    r = torch.as_tensor(rows, device='cuda')
    D64 = D.double()
    X64 = X[r].double()
    num = Y[r].double() @ D64.T
    den = X64 @ (D64 @ D64.T)
    return X64 * num.clamp_min(0.0) / den.clamp_min(1e-15)


def _stats_ref(Y, xo, cy, cx):
    """float64 X_out^T [Y | X_out] at the sampled columns (cy of Y, cx of X_out), with the matching float32
    outputs' column indices, |a| sums and |b| sums for the floor."""
    import torch
    x64 = xo.double()
    B = torch.cat([Y[:, torch.as_tensor(cy, device='cuda')].double(), x64[:, torch.as_tensor(cx, device='cuda')]], 1)
    return x64.T @ B, x64.abs().sum(0)[:, None] + B.abs().sum(0)[None, :]


def _gather_stats(stats, F, cy, cx):
    import torch
    idx = torch.as_tensor(np.concatenate([cy, F + np.asarray(cx)]), device='cuda')
    return stats[:, idx].double()


def _rel(got, ref):
    return ((got - ref).abs() / ref).max().item()


def _inputs(N, F, K, layout, seed):
    import torch
    from decomp_amd import _arrays
    g = torch.Generator(device='cuda')
    g.manual_seed(seed)
    Y = _y(N, F, layout == 'misaligned', lambda t: t.uniform_(0.0, 1.0, generator=g))
    X = torch.rand((N, K), generator=g, device='cuda') + 0.01
    D = torch.rand((K, F), generator=g, device='cuda') + 0.01
    _arrays.l2_normalize_(D, strict=True)   # rows of D have unit norm, as in the loop
    return Y, X, D


def _free():
    import torch
    torch.cuda.synchronize()
    torch.cuda.empty_cache()


def _check_stats_path(N, F, K, layout, tn_core, seed):
    """Integer Y and D (exact in bf16, sums below 2^24): the x update is exact in both cores."""
    import torch
    g = torch.Generator(device='cuda')
    g.manual_seed(seed)
    Y = _y(N, F, layout == 'misaligned', lambda t: t.copy_(torch.randint(0, 4, (N, F), generator=g, device='cuda')))
    D = torch.randint(0, 4, (K, F), generator=g, device='cuda').float()
    X = torch.rand((N, K), generator=g, device='cuda') + 0.01
    (x0, s0), (x1, s1) = _both_modes(Y, X, D, layout)
    assert torch.equal(x0, x1), 'integer x update differs between the modes'
    same = torch.equal(s0, s1)
    del Y, D, X, x0, x1, s0, s1
    _free()
    return same


@pytest.mark.parametrize('case', CASES, ids=[c[0] for c in CASES])
def test_step_both_modes_against_float64(case):
    import torch
    name, N, F, K, layout, nt_core, tn_core = case
    seed = N + F + K + len(layout)
    if layout != 'misaligned':
        assert _check_stats_path(N, F, K, layout, tn_core, seed + 1) == (not tn_core), (name, 'statistics path')
    Y, X, D = _inputs(N, F, K, layout, seed)
    (x0, s0), (x1, s1) = _both_modes(Y, X, D, layout)
    # the x update's path, and (where it is on the fp32 core) the statistics product's on these inputs
    assert torch.equal(x0, x1) == (not nt_core), (name, 'x-update path')
    if not nt_core and layout != 'misaligned':
        assert torch.equal(s0, s1) == (not tn_core), (name, 'statistics path')

    rng = np.random.RandomState(N % 9973 + K)
    rows = _sample(N, 1024, rng)
    xref = _x_ref(Y, X, D, rows)
    r = torch.as_tensor(rows, device='cuda')
    ex = [_rel(xo[r].double(), xref) for xo in (x0, x1)]
    cy, cx = _sample(F, 384, rng), _sample(K, 128, rng)
    es = []
    for xo, st in ((x0, s0), (x1, s1)):
        ref, _ = _stats_ref(Y, xo, cy, cx)
        es.append(_rel(_gather_stats(st, F, cy, cx), ref))
    print('\n%s: X_out %.3g / %.3g, stats %.3g / %.3g (mode 0 / mode 1)' % (name, ex[0], ex[1], es[0], es[1]))
    assert max(ex) < CAP and max(es) < CAP, (name, ex, es)
    assert ex[0] <= 2.0 * ex[1] + SLACK, (name, 'X_out', ex)
    assert es[0] <= 2.0 * es[1] + SLACK, (name, 'stats', es)
    del Y, X, D, x0, x1, s0, s1
    _free()


def test_dead_atom():
    """One column of X at about 2^-120 among O(1) columns, at the headline shape (both products on the 256 x 256
    core).  The x update reads X only in its epilogue and in the fp32 X . G, so every column of X_out keeps the
    relative bound.  In the statistics product the dead column of X_out is the tiny row of A and the tiny column of
    the second B segment: those outputs are held to the relative bound plus the floor of test_gpu_bf16x6_range.py,
    FLOOR (sum|a| + sum|b|), and the rest to twice mode 1's error."""
    import torch
    N, F, K = 65536, 4096, 256
    dead = 37
    Y, X, D = _inputs(N, F, K, 'oop', seed=41)
    g = torch.Generator(device='cuda')
    g.manual_seed(43)
    X[:, dead] = (1.0 + torch.rand(N, generator=g, device='cuda')) * 2.0 ** -120
    (x0, s0), (x1, s1) = _both_modes(Y, X, D, 'oop')
    assert not torch.equal(x0, x1)
    rng = np.random.RandomState(47)
    rows = _sample(N, 1024, rng)
    xref = _x_ref(Y, X, D, rows)
    r = torch.as_tensor(rows, device='cuda')
    ex = [_rel(xo[r].double(), xref) for xo in (x0, x1)]
    assert max(ex) < CAP and ex[0] <= 2.0 * ex[1] + SLACK, ex
    assert float(x0[:, dead].abs().max()) < 2.0 ** -100       # the atom stays dead

    cy, cx = _sample(F, 384, rng), np.union1d(_sample(K, 128, rng), [dead])
    jd = len(cy) + int(np.searchsorted(cx, dead))             # the dead atom's column among the gathered ones
    live_r = torch.ones(K, dtype=torch.bool, device='cuda')
    live_r[dead] = False
    live_c = torch.ones(len(cy) + len(cx), dtype=torch.bool, device='cuda')
    live_c[jd] = False
    res = []
    for xo, st in ((x0, s0), (x1, s1)):
        ref, sums = _stats_ref(Y, xo, cy, cx)
        got = _gather_stats(st, F, cy, cx)
        err = (got - ref).abs()
        live = (err / ref)[live_r][:, live_c].max().item()
        # x_dead^2 summed is about 2^-224: below float32's range in both modes
        under = err[dead, jd].item()
        err[dead, jd] = 0.0
        res.append((live, err, ref, sums, under, got[dead, jd].item()))
    (l0, err0, ref0, sums0, _, v0), (l1, err1, ref1, _, _, v1) = res
    assert l0 < CAP and l1 < CAP and l0 <= 2.0 * l1 + SLACK, (l0, l1)
    assert abs(v0) < 2.0 ** -126 and abs(v1) < 2.0 ** -126, (v0, v1)
    # the dead row and column: relative bound plus the floor
    edge = torch.zeros_like(err0, dtype=torch.bool)
    edge[dead, :] = True
    edge[:, jd] = True
    edge[dead, jd] = False
    beyond = ((err0 - FLOOR * sums0) / ref0)[edge].max().item()
    plain = (err0 / ref0)[edge].max().item()
    plain1 = (err1 / ref1)[edge].max().item()
    print('\ndead atom: live stats %.3g / %.3g, dead row and column %.3g (beyond the floor %.3g) / %.3g' %
          (l0, l1, plain, beyond, plain1))
    assert beyond <= 2.0 * l1 + SLACK, (beyond, l1)
    del Y, X, D, x0, x1, s0, s1
    _free()
