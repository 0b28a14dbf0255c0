"""GPU: the 256 x 256 TN body of the split-bf16 core (x^T [Y | x], the NMF statistics product).

Row-contiguous (XMAJOR) panels are staged with one 16-byte load of 4 rows at one k, split in registers and stored
as a [k][row] image per plane, then read back with ds_read_b64_tr_b16.  Small integers are exact in bf16 and
their sums exact in fp32, so any slip in that layout shows as a wrong integer; real data must keep the error of the
fp32 core (elementwise |C - C64| / (|A||B|) at most twice the fp32 MFMA core's) and re-run bit for bit."""

import numpy as np
import pytest

from test_gpu_nmf_bf16x6 import _operands, _rel_err, _run, _sample

pytestmark = pytest.mark.gpu

# form 2 (TN): A [K, M], B [K, N]; every split at least 1024 deep, so the 256 x 256 tile runs
TN256 = [
    (2, 256, 4352, 65536, 15),   # the headline statistics product (17 tiles x 15 splits)
    (2, 256, 1280, 32768, 8),
    (2, 256, 512, 16384, 2),     # two tiles, two splits
]


@pytest.mark.parametrize('case', TN256, ids=lambda c: 'f%d_%dx%dx%d_s%d' % c)
def test_tn256_exact_integers(case):
    import torch
    form, M, N, K, ks = case
    g = torch.Generator(device='cuda')
    g.manual_seed(M + N + ks)
    # |sum| <= 65536 * 16 < 2^24: every partial sum is exact in fp32
    a = torch.randint(-4, 5, (K, M), generator=g, device='cuda').float()
    b = torch.randint(-4, 5, (K, N), generator=g, device='cuda').float()
    c = _run('dcp_gemm_bf16x6_f32', form, a, b, M, N, K, ks)
    ref = a.double().T @ b.double()
    assert torch.equal(c.double(), ref)


@pytest.mark.parametrize('kind', ['nonneg', 'wide'])
@pytest.mark.parametrize('case', TN256[1:], ids=lambda c: 'f%d_%dx%dx%d_s%d' % c)
def test_tn256_error_within_twice_fp32(case, kind):
    form, M, N, K, ks = case
    a, b = _operands(form, M, N, K, kind, seed=7 * M + N + ks)
    c6 = _run('dcp_gemm_bf16x6_f32', form, a, b, M, N, K, ks)
    c32 = _run('dcp_gemm_f32', form, a, b, M, N, K, ks)
    rng = np.random.RandomState(2)
    rows, cols = _sample(M, 512, rng), _sample(N, 512, rng)
    e6 = _rel_err(form, a, b, c6, rows, cols)
    e32 = _rel_err(form, a, b, c32, rows, cols)
    assert np.isfinite(e6) and e6 <= 2.0 * e32 + 1e-9, (case, kind, e6, e32)
    assert e6 < 1e-5, (case, kind, e6)


def test_tn256_bitwise_rerun():
    import torch
    form, M, N, K, ks = TN256[1]
    a, b = _operands(form, M, N, K, 'signed', seed=5)
    c0 = _run('dcp_gemm_bf16x6_f32', form, a, b, M, N, K, ks)
    assert torch.equal(c0, _run('dcp_gemm_bf16x6_f32', form, a, b, M, N, K, ks))
