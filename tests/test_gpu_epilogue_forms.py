"""GPU: the element form and the 16-byte form of a GEMM epilogue give the same bits.

An epilogue functor (decomp_amd/csrc/epilogue.hpp) reaches memory one element at a time or four float columns at
once; launch_gemm_mfma picks the form per launch (vec_epi) from the shape and from the addresses of the arrays the
functor's vec_ok() names.  Both forms call one arithmetic function, and this file holds them to it: every case runs
one step twice on identical data, once with every array as allocated (16-byte aligned: the 16-byte form) and once
with ONE array of the epilogue as a view that starts one element into a larger buffer (4 bytes off: the element form,
inside the same kernel instantiation, on the same accumulators), and asserts torch.equal on every output.

All cases are float32 with dcp_set_f32_product_mode(h, 1), so every product runs on the fp32 MFMA core.  The shapes
are the smallest at which the 16-byte form is live at all (it needs whole tiles): 256 x 128 with 64 atoms and
256 x 256 with 128 atoms.  The route gives both the 64 x 64 tile (16-deep K blocks; 64-deep for Y.D^T of the second
shape) -- the 128 x 128 and 256 x 256 tiles start at sizes far beyond a quick test, and they share the core's one
16-byte epilogue.  dcp_debug_gemm_route confirms per case that the tile launched for the product that carries the
epilogue divides its shape -- otherwise both runs would take the element form.  F < 1024, so Y.D^T is never split
and the quotient is fused into it (nmf_xupdate_splits).

case            entry                  array moved  epilogue whose form it switches (product)
l2              dcp_nmf_mu_stats_f32   X_out        EpiMuNum, full denominator x.G            (Y.D^T, NT)
l2_penalty      dcp_nmf_mu_stats_f32   X_out        EpiMuNumPen                               (Y.D^T, NT)
kl              dcp_nmf_mu_stats_f32   X_out        EpiMuNum, one denominator per column      (r.D^T, NT)
kl_y            dcp_nmf_mu_stats_f32   Y            EpiKlRatio (without a mask it reads Y)    (x.D, NN)
l2_mask         dcp_nmf_mu_stats_f32   mask         EpiMulMask                                (x.D, NN)
kl_mask         dcp_nmf_mu_stats_f32   mask         none: EpiKlRatio reads the pre-masked Y; the mask is the left
                                                    operand of M.D^T, whose panel loads change with its alignment
beta_mask       dcp_nmf_mu_stats_f32   mask         EpiBetaParts, beta = 0.5                  (x.D, NN)
impute          dcp_nmf_impute_f32     Y_out        EpiImpute                                 (x.D, NN)
The masks are not binary, so the row-bit path (EpiMulMaskBits) is not taken.  The LASSO epilogues read library
workspace only; their forms cannot be switched through the ABI at a fixed problem."""
import ctypes

import pytest

from test_gpu_nmf_bf16x6 import _Mode, _lib_h

pytestmark = pytest.mark.gpu

SHAPES = [(256, 128, 64), (256, 256, 128)]   # rows, F, atoms: whole 64 x 64 tiles
# name, likelihood, masked, penalty, beta, the array moved, form of the product that carries the epilogue
CASES = [
    ('l2', 'l2', False, None, None, 'X_out', 'NT'),
    ('l2_penalty', 'l2', False, (0.05, 0.1), None, 'X_out', 'NT'),
    ('kl', 'kl', False, None, None, 'X_out', 'NT'),
    ('kl_y', 'kl', False, None, None, 'Y', 'NN'),
    ('l2_mask', 'l2', True, None, None, 'mask', 'NN'),
    ('kl_mask', 'kl', True, None, None, 'mask', 'NN'),
    ('beta_mask', 'beta', True, None, 0.5, 'mask', 'NN'),
]


def _off4(t):
    """A copy of t that starts one float past a 16-byte boundary."""
    import torch
    buf = torch.empty(t.numel() + 1, dtype=t.dtype, device=t.device)
    v = buf[1:].view(t.shape)
    assert v.data_ptr() % 16 == 4
    v.copy_(t)
    return v


def _whole_tiles(form, M, N, K):
    """The fp32 MFMA tile that dcp_debug_gemm_route launches for this product divides it."""
    from decomp_amd import _hip
    out = (ctypes.c_int32 * 13)()
    rc = _hip.load().dcp_debug_gemm_route(0, {'NT': 0, 'NN': 1}[form], M, N, K, 0, 0, 0, 0, 0, 0,
                                          ctypes.cast(out, ctypes.c_void_p))
    assert rc == 0
    core, _, BM, BN, BK = out[0], out[1], out[2], out[3], out[4]
    return core == 0 and M % BM == 0 and N % BN == 0 and K % BK == 0


def _inputs(N, F, K, seed):
    import torch
    g = torch.Generator(device='cuda')
    g.manual_seed(seed)
    def u(*shape):
        return torch.rand(shape, generator=g, device='cuda') + 0.1
    X, D = u(N, K), u(K, F)
    Y = X @ D * (0.5 + u(N, F))
    mask = torch.rand((N, F), generator=g, device='cuda')   # weights in [0, 1), not binary
    return Y, mask, X, D


def _mu_stats(Y, mask, X, X_out, D, lik, pen, beta):
    import torch
    from decomp_amd import _arrays, _hip, nmf
    lib, h = _lib_h()
    N, F = Y.shape
    K = D.shape[0]
    code = {'l2': _hip.LIK_L2, 'kl': _hip.LIK_KL, 'beta': _hip.LIK_BETA}[lik]
    W = lib.dcp_nmf_mu_stats_width(F, K, code, 0 if mask is None else 1)
    stats = torch.empty((K, W), device='cuda')
    if beta is not None:
        _hip.check(h, lib.dcp_set_nmf_beta(h, beta), 'dcp_set_nmf_beta')
    nmf._set_penalty(h, pen or (0.0, 0.0))
    try:
        _hip.check(h, lib.dcp_nmf_mu_stats_f32(h, _arrays.ptr(Y), _arrays.ptr(mask), _arrays.ptr(X),
                                                _arrays.ptr(X_out), _arrays.ptr(D), N, F, K, code,
                                                _arrays.ptr(stats)), 'dcp_nmf_mu_stats_f32')
        torch.cuda.synchronize()
    finally:
        nmf._set_penalty(h, (0.0, 0.0))
        if beta is not None:
            lib.dcp_set_nmf_beta(h, 0.0)
    return stats


@pytest.mark.parametrize('shape', SHAPES, ids=lambda s: '%dx%dx%d' % s)
@pytest.mark.parametrize('case', CASES, ids=lambda c: c[0])
def test_mu_stats_forms_agree(case, shape):
    import torch
    name, lik, masked, pen, beta, moved, form = case
    N, F, K = shape
    assert _whole_tiles(form, N, K, F) if form == 'NT' else _whole_tiles(form, N, F, K)
    Y, mask, X, D = _inputs(N, F, K, seed=N + F + K)
    if not masked:
        mask = None
    got = []
    with _Mode(1):
        for off in (False, True):
            y = _off4(Y) if off and moved == 'Y' else Y
            m = _off4(mask) if off and moved == 'mask' else mask
            xo = torch.empty_like(X)
            if off and moved == 'X_out':
                xo = _off4(xo)
            stats = _mu_stats(y, m, X, xo, D, lik, pen, beta)
            got.append((xo, stats))
    assert _lib_h()[0].dcp_set_f32_product_mode(_lib_h()[1], -1) == 0
    (x0, s0), (x1, s1) = got
    assert torch.isfinite(x0).all() and torch.isfinite(s0).all()
    assert torch.equal(x0, x1), 'X_out: %d elements differ' % int((x0 != x1).sum())
    assert torch.equal(s0, s1), 'stats: %d elements differ' % int((s0 != s1).sum())


@pytest.mark.parametrize('shape', SHAPES, ids=lambda s: '%dx%dx%d' % s)
def test_impute_forms_agree(shape):
    import torch
    from decomp_amd import _arrays, _hip
    N, F, K = shape
    assert _whole_tiles('NN', N, F, K)
    Y, mask, X, D = _inputs(N, F, K, seed=N + F + K + 1)
    mask[:, ::7] = 1.0    # the bit-exact ends of the weight range as well
    mask[:, 3::7] = 0.0
    lib, h = _lib_h()
    got = []
    with _Mode(1):
        for off in (False, True):
            yo = torch.empty_like(Y)
            if off:
                yo = _off4(yo)
            _hip.check(h, lib.dcp_nmf_impute_f32(h, _arrays.ptr(Y), _arrays.ptr(mask), _arrays.ptr(X), _arrays.ptr(D),
                                                  N, F, K, _arrays.ptr(yo)), 'dcp_nmf_impute_f32')
            torch.cuda.synchronize()
            got.append(yo)
    assert torch.isfinite(got[0]).all()
    assert torch.equal(got[0], got[1]), 'Y_out: %d elements differ' % int((got[0] != got[1]).sum())
