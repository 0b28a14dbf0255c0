"""GPU: which fragment each product of the split-bf16 ("bf16x6") K loop reads, exactly (gemm_mfma_bf16x6.hpp).

The K loop refills a fragment register as soon as its plane is dead: inside a K block with the second 32-row
group's fragment of that plane, and (ring of three) in the second group with the next block's fragments from the
next buffer.  A fragment taken from the wrong K block, buffer, plane or 32-row group must change an exact result.

Operands (math orientation A [M, K], B [K, N]), every plane a small integer on its own power-of-two scale:
    a = s (ih + im 2^-9 + il 2^-18),  ih, im in {2, 3}, il in {1, 2, 3}
    b = s (1  + bm 2^-10 + bl 2^-20), bm, bl in {1, 2, 3},         s = +-1 at random
The digits depend on the K block, on the 32-row (32-column) group and on the position; the round-to-nearest split
gives exactly these planes (checked on the device with torch's bfloat16 rounding before anything runs).  A row of A
is nonzero at one k of every K block, at a position that depends on row, block and group; a column of B is dense in
one of every Q K blocks (all of them up to four blocks) and zero in the others, so an output sums at most four
pairs.  The six kept products then lie on distinct scales
    hh 1,  mh 2^-9,  hm 2^-10,  lh 2^-18,  mm 2^-19,  hl 2^-20        (dropped: lm, ml, ll)
and every partial sum, in any order, is a multiple of 2^-20 below 4 * 3.03 < 16: exact in fp32.  The reference is
the integer product of the planes scaled by 2^20 (three float64 products of integers below 2^24, at most 4480
terms each: exact, converted to int64), and the output must be torch.equal to it.  Every case runs twice.

Shapes go through dcp_gemm_bf16x6_f32 as in test_gpu_bf16x6_ring.py (the front end picks the tile):
  NT 24576 x 512    the 256 x 256 tile (an unsplit NT product gets it from 192 tiles upward; a single 256 x 256
                    output would run on the 128 x 128 tile), 1 .. 7 K blocks: every ring phase, every peeled exit
  TN 256 x 4352 in 4 splits and 256 x 32768 unsplit, 64 .. 70 K blocks per split: the 256 x 256 tile (TN takes it
                    only when every split is at least 1024 deep)
  NT 4096 x 2048, TN 1024 x 8192, 1 .. 5 K blocks: the 128 x 128 tile (two buffers)
The TN 256 x 256 cases also run with B in two column segments (dcp_gemm_bf16x6_seg_f32), as the statistics product
x^T [Y | x] of the NMF step has it: 4096 + 256 columns in 4 splits, 24576 + 8192 columns unsplit, the same operands
cut at that column, so the same exact reference.  Every case first asks dcp_gemm_bf16x6_tier which tile the front
end gives its shape and asserts the one it is meant for: a later change of the thresholds fails here instead of
moving the cases onto the other tile.
One NT case goes through dcp_nmf_mu_stats_f32 at 49152 x 16, 256 atoms, the smallest shape whose K loop is followed
by the denominator tail: integer Y and D, product mode 0 against mode 1, bitwise."""

import pytest

from test_gpu_bf16x6_ring import _run

pytestmark = pytest.mark.gpu

BK = 16


def _operands(M, N, K, seed):
    """(a [M, K] float32, b [K, N] float32, ref [M, N] float32): ref is the exact sum of the six kept products."""
    import torch
    dev = 'cuda'
    g = torch.Generator(device=dev)
    g.manual_seed(seed)
    Q = max(1, -(-(K // BK) // 4))

    def sign(shape):
        return torch.randint(0, 2, shape, generator=g, device=dev) * 2 - 1

    r = torch.arange(M, device=dev)[:, None]
    k = torch.arange(K, device=dev)[None, :]
    kb, grp = k // BK, r // 32
    sa = sign((M, K)) * ((k % BK) == (5 * r + 3 * kb + 7 * grp) % BK)
    ah = sa * (2 + (kb + grp) % 2)
    am = sa * (2 + ((kb >> 1) + grp + r) % 2)
    al = sa * (1 + (kb + 2 * grp + r) % 3)

    k = torch.arange(K, device=dev)[:, None]
    c = torch.arange(N, device=dev)[None, :]
    kb, grp = k // BK, c // 32
    bh = sign((K, N)) * (((kb + c) % Q) == 0)
    bm = bh * (1 + (kb + grp + k) % 3)
    bl = bh * (1 + (kb + 2 * grp + k + c) % 3)

    a64 = ah.double() + am.double() * 2.0 ** -9 + al.double() * 2.0 ** -18
    b64 = bh.double() + bm.double() * 2.0 ** -10 + bl.double() * 2.0 ** -20
    a, b = a64.float(), b64.float()
    assert torch.equal(a.double(), a64) and torch.equal(b.double(), b64)
    # the planes the kernel's split (round to nearest, then the exact residual) makes of these values
    for v, planes, scales in ((a, (ah, am, al), (0, 9, 18)), (b, (bh, bm, bl), (0, 10, 20))):
        rest = v
        for p, s in zip(planes, scales):
            q = rest.bfloat16().float()
            assert torch.equal(q.double(), p.double() * 2.0 ** -s), 'split does not give the designed planes'
            rest = rest - q
        assert not rest.any()
    assert float((ah.abs().double() @ bh.abs().double()).max()) <= 3 * 4     # at most four pairs per output

    # kept: (h + m + l) bh, (h + m) bm, h bl; in units of 2^-20
    ref = ((ah * 2 ** 20 + am * 2 ** 11 + al * 2 ** 2).double() @ bh.double()
           + (ah * 2 ** 10 + am * 2).double() @ bm.double() + ah.double() @ bl.double())
    assert float(ref.abs().max()) < 2.0 ** 24
    ref = ref.to(torch.int64)
    assert int((ref != 0).sum()) > ref.numel() // 4
    return a, b, (ref.double() * 2.0 ** -20).float()


HUGE, LARGE = 1, 0      # dcp_gemm_bf16x6_tier: the 256 x 256 tile (ring of three), the 128 x 128 tile (two buffers)


def _run_seg(form, a, b, b2, M, N, n1, K, ksplits):
    import torch
    from decomp_amd import _arrays, _hip
    lib, h = _arrays.lib_handle(a)
    c = torch.full((M, N), float('nan'), dtype=torch.float32, device='cuda')
    rc = lib.dcp_gemm_bf16x6_seg_f32(h, form, _arrays.ptr(a), _arrays.ptr(b), _arrays.ptr(b2), _arrays.ptr(c), M, N, n1,
                                     K, ksplits)
    _hip.check(h, rc, 'dcp_gemm_bf16x6_seg_f32')
    torch.cuda.synchronize()
    return c


def _check(form, M, N, K, ksplits, tier, n1=None):
    """n1: the width of the first of two B segments (None: one segment, through dcp_gemm_bf16x6_f32)."""
    import torch
    from decomp_amd import _hip
    assert _hip.load().dcp_gemm_bf16x6_tier(form, M, N, N if n1 is None else n1, K, ksplits) == tier
    a, b, ref = _operands(M, N, K, seed=1000 * form + K + ksplits)
    if form == 0:       # NT: A [M, K], B [N, K]
        a, b = a.contiguous(), b.T.contiguous()
    else:               # TN: A [K, M], B [K, N]
        a, b = a.T.contiguous(), b.contiguous()
    if n1 is None:
        run = lambda: _run(form, a, b, M, N, K, ksplits)
    else:
        assert form == 2
        b1, b2 = b[:, :n1].contiguous(), b[:, n1:].contiguous()
        run = lambda: _run_seg(form, a, b1, b2, M, N, n1, K, ksplits)
    c0 = run()
    c1 = run()
    bad = (c0 != ref).nonzero()
    assert torch.equal(c0, ref), ((form, M, N, K, ksplits), int(bad.shape[0]), bad[:4].tolist(),
                                  [(float(c0[i, j]), float(ref[i, j])) for i, j in bad[:4].tolist()])
    assert torch.equal(c0, c1), ('two runs differ', form, M, N, K, ksplits)
    del a, b, ref, c0, c1, run
    torch.cuda.empty_cache()


@pytest.mark.parametrize('nkb', [1, 2, 3, 4, 5, 6, 7])
def test_nt256_exact(nkb):
    _check(0, 24576, 512, BK * nkb, 1, HUGE)


@pytest.mark.parametrize('n1', [None, 4096], ids=['one_segment', 'two_segments'])
@pytest.mark.parametrize('nkb', [64, 65, 66, 67, 68, 69, 70])
def test_tn256_split_exact(nkb, n1):
    """17 column tiles, 4 splits of nkb K blocks each (slabs summed in fp32: still on the 2^-20 grid below 16)."""
    _check(2, 256, 4352, BK * nkb * 4, 4, HUGE, n1)


@pytest.mark.parametrize('n1', [None, 24576], ids=['one_segment', 'two_segments'])
@pytest.mark.parametrize('nkb', [64, 65, 66, 67, 68, 69, 70])
def test_tn256_unsplit_exact(nkb, n1):
    _check(2, 256, 32768, BK * nkb, 1, HUGE, n1)


@pytest.mark.parametrize('nkb', [1, 2, 3, 4, 5])
@pytest.mark.parametrize('form', [0, 2])
def test_128_exact(form, nkb):
    if form == 0:
        _check(0, 4096, 2048, BK * nkb, 1, LARGE)
    else:
        _check(2, 1024, 8192, BK * nkb, 1, LARGE)


def test_den_tail_after_the_loop_bitwise():
    """49152 x 16, 256 atoms: one K block, then the denominator tail through the ring the loop has left."""
    import torch
    from test_gpu_bf16x6_paths import _both_modes, _free
    from test_gpu_nmf_fused_den import _integer_inputs
    N, F, K = 49152, 16, 256
    Y, X, D = _integer_inputs(N, F, K, seed=12)
    for _ in range(2):
        (x0, _s0), (x1, _s1) = _both_modes(Y, X, D, 'oop')
        assert torch.isfinite(x0).all()
        assert torch.equal(x0, x1), int((x0 != x1).sum())
    del Y, X, D, x0, x1
    _free()
