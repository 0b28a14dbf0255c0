"""GPU: the LDS ring of the split-bf16 ("bf16x6") GEMM core (gemm_mfma_bf16x6.hpp), exactly, on small integers.

The 256 x 256 tile keeps three K blocks of planes in LDS and synchronises once per block, inside the block; the
128 x 128 tile keeps two and synchronises between blocks.  A fragment read from a stage that is stale or half
written pairs A of one K block with B of another.  Operands here are dense random integers in [-4, 4], every K
block drawn independently.  Such a value is its own h plane (m = l = 0), every product is an integer of magnitude
<= 16 and every partial sum stays below 16 K < 2^24, so the float32 result must EQUAL the int64 NumPy product: no
tolerance, and the NumPy side is exact by the same argument.  Every case runs twice and the two results are compared
bitwise (a race need not fail the same way twice).

Shapes go through dcp_gemm_bf16x6_f32, whose front end picks the tile (gemm.hpp, pick_tier / x6_tier):
  NT 24576 x 512   192 tiles of 256 x 256 -> the 256 x 256 tile at any depth
  NT 4096 x 2048   128 tiles of 256 x 256, 512 of 128 x 128 -> the 128 x 128 tile
  TN 1024 x 8192 (unsplit), 256 x 16384 (split)  -> the 128 x 128 tile: TN takes 256 x 256 only when every split
                   is at least 1024 deep, so one to eight K blocks per split exist on 128 x 128 only
  TN 256 x 4352, splits of 64 .. 70 K blocks, and 256 x 32768 unsplit, 64 .. 66 K blocks -> the 256 x 256 tile in
                   every ring phase mod 3, 17 and 128 column tiles.  These products are too deep for a whole int64
                   product on the host in reasonable time: they are compared on every 16th column (all rows, so
                   every column tile, every wave and every 32-column fragment block of each), and bitwise between
                   the two runs on the whole output.
"""

import numpy as np
import pytest

pytestmark = pytest.mark.gpu

BK = 16


def _run(form, a, b, M, N, K, ksplits):
    import torch
    from decomp_amd import _arrays, _hip
    lib, h = _arrays.lib_handle(torch.empty(1, device='cuda'))
    c = torch.full((M, N), float('nan'), dtype=torch.float32, device='cuda')
    rc = lib.dcp_gemm_bf16x6_f32(h, form, _arrays.ptr(a), _arrays.ptr(b), _arrays.ptr(c), M, N, K, ksplits)
    _hip.check(h, rc, 'dcp_gemm_bf16x6_f32')
    torch.cuda.synchronize()
    return c


def _int_operands(form, M, N, K, seed):
    """Host int64 operands of an NT (A[M,K], B[N,K]) or TN (A[K,M], B[K,N]) product, dense in [-4, 4]."""
    rng = np.random.RandomState(seed)
    sa = (M, K) if form == 0 else (K, M)
    sb = (N, K) if form == 0 else (K, N)
    return rng.randint(-4, 5, sa).astype(np.int64), rng.randint(-4, 5, sb).astype(np.int64)


def _check(form, M, N, K, ksplits, col_step=1):
    import torch
    assert 16 * K < 2 ** 24
    A, B = _int_operands(form, M, N, K, seed=1000 * form + K + ksplits)
    a = torch.from_numpy(A.astype(np.float32)).cuda().contiguous()
    b = torch.from_numpy(B.astype(np.float32)).cuda().contiguous()
    c0 = _run(form, a, b, M, N, K, ksplits)
    c1 = _run(form, a, b, M, N, K, ksplits)
    cols = np.arange(0, N, col_step)
    if form == 0:
        ref = A @ np.ascontiguousarray(B[cols].T)
    else:
        ref = np.ascontiguousarray(A.T) @ np.ascontiguousarray(B[:, cols])
    got = c0.cpu().numpy()
    assert np.isfinite(got).all(), (form, M, N, K, ksplits)
    assert np.array_equal(got[:, cols].astype(np.int64), ref), (form, M, N, K, ksplits)
    assert np.array_equal(got[:, cols], ref.astype(np.float32))
    assert torch.equal(c0, c1), ('two runs differ', form, M, N, K, ksplits)


# one to eight K blocks in an unsplit product: every ring phase mod 3, fewer blocks than stages, the peeled tail
UNSPLIT_K = [BK * n for n in range(1, 9)]
# (K blocks per split, splits); the last pair leaves the final split two blocks short of the others
SPLIT_BLOCKS = [(1, 3), (2, 3), (3, 3), (4, 3), (7, 3)]

SHAPES_SMALL = {
    # name: (form, M, N) unsplit, (form, M, N) split
    'nt256': ((0, 24576, 512), (0, 24576, 512)),
    'nt128': ((0, 4096, 2048), (0, 4096, 2048)),
    'tn128': ((2, 1024, 8192), (2, 256, 16384)),
}


@pytest.mark.parametrize('K', UNSPLIT_K)
@pytest.mark.parametrize('shape', sorted(SHAPES_SMALL))
def test_unsplit_exact(shape, K):
    form, M, N = SHAPES_SMALL[shape][0]
    _check(form, M, N, K, 1)


@pytest.mark.parametrize('blocks,splits', SPLIT_BLOCKS)
@pytest.mark.parametrize('shape', sorted(SHAPES_SMALL))
def test_split_exact(shape, blocks, splits):
    form, M, N = SHAPES_SMALL[shape][1]
    _check(form, M, N, blocks * BK * splits, splits)


@pytest.mark.parametrize('shape', sorted(SHAPES_SMALL))
def test_split_ragged_last_exact(shape):
    """10 K blocks over 3 splits: 4 + 4 + 2 blocks, two ring phases in one launch."""
    form, M, N = SHAPES_SMALL[shape][1]
    _check(form, M, N, 10 * BK, 3)


@pytest.mark.parametrize('blocks', [64, 65, 66, 67, 70])
def test_tn256_split_exact(blocks):
    """The statistics product's own shape class: 17 column tiles of the 256 x 256 tile, 4 splits."""
    _check(2, 256, 4352, blocks * BK * 4, 4, col_step=16)


@pytest.mark.parametrize('blocks', [64, 65, 66])
def test_tn256_unsplit_exact(blocks):
    _check(2, 256, 32768, blocks * BK, 1, col_step=16)
