"""GPU: which bf16 products the split-bf16 ("bf16x6") core sums, term by term, on every tile and form.

Every operand value is t (1 + 2^-9 + 2^-18) in A and t (1 + 2^-10 + 2^-20) in B with t in {-1, 0, 1}; the split
gives these planes exactly (h = t, m = t 2^-9 or t 2^-10, l = t 2^-18 or t 2^-20).  The six products the core keeps
then add distinct powers of two per pair of nonzero t:

    hh 1,  mh 2^-9,  hm 2^-10,  lh 2^-18,  mm 2^-19,  hl 2^-20        (dropped: lm 2^-28, ml 2^-30, ll 2^-38)

A row of A is nonzero at one k in every P, a column of B on one of every Q runs of P k, so an output sums at most
12 nonzero pairs: every partial sum, in any order, lies on the 2^-20 grid below 16 and is exact in fp32.  The
result must equal the float64 sum of the six kept terms exactly.  A lost or doubled term, a plane read from the
wrong lane half or the wrong K block, or a stale staging buffer moves a result by at least 2^-20.  The shapes
include one, two and three K blocks per tile (the staging pipeline's prologue and last block)."""

import numpy as np
import pytest

from test_gpu_nmf_bf16x6 import _run

pytestmark = pytest.mark.gpu

KEPT = 1.0 + 2.0 ** -9 + 2.0 ** -10 + 2.0 ** -18 + 2.0 ** -19 + 2.0 ** -20

# form, M, N, K, ksplits; the tile follows from x6_tier (gemm.hpp), and dcp_gemm_bf16x6_f32 fails rather than
# fall back when no bf16x6 tile fits
CASES = [
    (0, 8192, 1536, 256, 1),     # NT 256 x 256 (TIER_HUGE: 192 tiles)
    (0, 8192, 1536, 16, 1),      # NT 256 x 256, one K block
    (0, 8192, 1536, 32, 1),      # two K blocks
    (0, 8192, 1536, 48, 1),      # three K blocks
    (0, 8192, 256, 4096, 8),     # NT split over K: EpiSlab slabs, reduced in fp32
    (0, 4096, 2048, 512, 1),     # NT 128 x 128 (TIER_LARGE)
    (0, 4096, 2048, 32, 1),      # NT 128 x 128, two K blocks
    (2, 256, 1280, 32768, 8),    # TN 256 x 256: 8 splits of 4096
    (2, 256, 512, 16384, 2),     # TN 256 x 256: two tiles, two splits
    (2, 2048, 4096, 256, 1),     # TN 128 x 128 (unsplit, < 1024 deep)
    (2, 2048, 4096, 16, 1),      # TN 128 x 128, one K block
]


def _signs(shape, nonzero, rng):
    return rng.choice(np.array([-1.0, 1.0]), size=shape) * nonzero


def _pattern(M, N, K, seed):
    """t_a [M, K] and t_b [K, N] in {-1, 0, 1} with at most 12 nonzero products per output."""
    rng = np.random.RandomState(seed)
    P = min(64, K)
    Q = max(1, -(-(K // P) // 12))
    k = np.arange(K)
    a_on = (k[None, :] % P) == (np.arange(M)[:, None] % P)
    b_on = ((k[:, None] // P) % Q) == (np.arange(N)[None, :] % Q)
    return _signs((M, K), a_on, rng), _signs((K, N), b_on, rng)


@pytest.mark.parametrize('case', CASES, ids=lambda c: 'f%d_%dx%dx%d_s%d' % c)
def test_six_kept_terms_exact(case):
    import torch
    form, M, N, K, ks = case
    ta, tb = _pattern(M, N, K, seed=M + 3 * N + K + ks)
    a64 = ta * (1.0 + 2.0 ** -9 + 2.0 ** -18)
    b64 = tb * (1.0 + 2.0 ** -10 + 2.0 ** -20)
    assert np.array_equal(a64.astype(np.float32).astype(np.float64), a64)
    assert np.array_equal(b64.astype(np.float32).astype(np.float64), b64)
    if form == 0:   # NT: A [M, K], B [N, K]
        a = torch.from_numpy(a64.astype(np.float32)).cuda()
        b = torch.from_numpy(np.ascontiguousarray(b64.T).astype(np.float32)).cuda()
    else:           # TN: A [K, M], B [K, N]
        a = torch.from_numpy(np.ascontiguousarray(a64.T).astype(np.float32)).cuda()
        b = torch.from_numpy(b64.astype(np.float32)).cuda()
    c = _run('dcp_gemm_bf16x6_f32', form, a, b, M, N, K, ks).double().cpu().numpy()
    pairs = ta @ tb                       # signed count of nonzero pairs, exact
    assert (np.abs(ta) @ np.abs(tb)).max() <= 12
    ref = pairs * KEPT
    assert np.count_nonzero(pairs) > pairs.size // 4
    bad = np.argwhere(c != ref)
    assert bad.size == 0, (case, bad[:4].tolist(), [(c[i, j], ref[i, j]) for i, j in bad[:4]])
