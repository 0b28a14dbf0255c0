"""GPU: the NMF x update with x . G formed inside the Y . D^T launch (the denominator tail of the 256 x 256
split-bf16 NT kernel, gemm_mfma_bf16x6.hpp; dispatch in nmf_stats, nmf_impl.hpp), through dcp_nmf_mu_stats_f32.

In product mode 0, out of place, with an unsplit x update on 256 x 256 tiles, one launch computes
    X_out = X o max(Y . D^T, 0) / max(X . G, eps),   G = D . D^T   (penalised: max(X . G + l1 + l2 X, eps))
and Q = X . G never reaches memory.  Mode 1 keeps the two launches (fp32 X . G into Q, then the quotient in the
epilogue of the fp32 Y . D^T) and is the comparator: the tail issues, per element of X . G, the v_mfma_f32_32x32x2_f32
sequence of the stand-alone fp32 kernel, so with Y and D small integers (Y . D^T exact on both cores) X_out must be
bitwise equal between the modes for arbitrary float32 X.

Shapes: the path needs the 256 x 256 tile, which pick_tier gives an unsplit product only from 192 tiles upward, so
the smallest are 49152 rows x 256 atoms (one column tile, 16 K blocks of x . G) and 24576 x 512 (two column tiles,
32 K blocks).  F = 16, 32, 48, 64 gives one to four bf16 K blocks in front of the tail: every exit of the peeled
ring loop.  At F < 1024 nmf_xupdate_splits never splits, so here it is the tile choice, not its `tiles >= 192`
branch, that decides the path; that branch decides at F = 4096, in test_gpu_fullsize.py and
test_gpu_bf16x6_paths.py.  test_q_product_is_not_launched shows that these shapes do take the fused path.

What no test here can tell apart is G from its transpose: G = D . D^T is bitwise symmetric for integer D and for
random D alike (G[i, j] and G[j, i] are the same ordered sums of commutative products), and the entry offers no way
to pass another G.  That the tail reads G as [k][column] (not assuming symmetry) rests on the code."""

import ctypes

import pytest

from test_gpu_bf16x6_paths import CAP, SLACK, _both_modes, _free, _inputs, _rel, _step, _x_ref
from test_gpu_nmf_bf16x6 import _Mode, _lib_h, _sample

pytestmark = pytest.mark.gpu

SHAPES = [(49152, 256), (24576, 512)]
FS = [16, 32, 48, 64]
CASES = [(N, F, K) for (N, K) in SHAPES for F in FS]
IDS = ['%dx%dk%d' % c for c in CASES]
PROF_XNEG, PROF_XUPDATE = 1, 2


def _integer_inputs(N, F, K, seed, dead=None):
    """Y and D integers in 0..3 (exact in bf16, sums far below 2^24), X = rand + 0.01; `dead`: that column of X
    at about 2^-120."""
    import torch
    g = torch.Generator(device='cuda')
    g.manual_seed(seed)
    Y = torch.randint(0, 4, (N, F), generator=g, device='cuda').float()
    D = torch.randint(0, 4, (K, F), generator=g, device='cuda').float()
    X = torch.rand((N, K), generator=g, device='cuda') + 0.01
    if dead is not None:
        X[:, dead] = (1.0 + torch.rand(N, generator=g, device='cuda')) * 2.0 ** -120
    return Y, X, D


class _Penalty:
    def __init__(self, l1, l2):
        self.pen = (l1, l2)

    def __enter__(self):
        from decomp_amd import nmf
        nmf._set_penalty(_lib_h()[1], self.pen)

    def __exit__(self, *exc):
        from decomp_amd import nmf
        nmf._set_penalty(_lib_h()[1], (0.0, 0.0))


def _launches(Y, X, D, layout):
    """(x_neg launches, x_update launches) of one step."""
    lib, h = _lib_h()
    assert lib.dcp_profile_reset(h) == 0 and lib.dcp_profile_select(h, 0xffffffff) == 0
    assert lib.dcp_profile_enable(h, 1) == 0
    try:
        _step(Y, X, D, layout)
    finally:
        lib.dcp_profile_enable(h, 0)
    out = []
    for lab in (PROF_XNEG, PROF_XUPDATE):
        ms, cnt = ctypes.c_double(0), ctypes.c_int64(0)
        assert lib.dcp_profile_read(h, lab, ctypes.byref(ms), ctypes.byref(cnt)) == 0
        out.append(cnt.value)
    lib.dcp_profile_reset(h)
    return tuple(out)


@pytest.mark.parametrize('case', CASES, ids=IDS)
def test_bitwise_equal_to_fp32_product(case):
    """Integer Y and D, arbitrary X: mode 0 (fused denominator) and mode 1 (stand-alone fp32 x . G) give the same
    bits; also with one column of X at 2^-120 (terms of x . G about 2^-111 beside terms of order one)."""
    import torch
    N, F, K = case
    for dead in (None, 37):
        Y, X, D = _integer_inputs(N, F, K, seed=N + F + K, dead=dead)
        (x0, _), (x1, _) = _both_modes(Y, X, D, 'oop')
        assert torch.isfinite(x0).all()
        assert torch.equal(x0, x1), (case, dead, int((x0 != x1).sum()))
        if dead is not None:
            assert float(x0[:, dead].abs().max()) < 2.0 ** -100
        del Y, X, D, x0, x1
        _free()


@pytest.mark.parametrize('F', FS)
def test_bitwise_equal_in_place(F):
    """X_out is X, 256 atoms: whichever path the step takes, the modes agree bit for bit and with the
    out-of-place result."""
    import torch
    N, K = 49152, 256
    Y, X, D = _integer_inputs(N, F, K, seed=7 + F)
    (x0, _), (x1, _) = _both_modes(Y, X, D, 'inplace')
    assert torch.equal(x0, x1), (F, int((x0 != x1).sum()))
    with _Mode(0):
        xo, _ = _step(Y, X, D, 'oop')
    assert torch.equal(x0, xo)
    del Y, X, D, x0, x1, xo
    _free()


@pytest.mark.parametrize('case', CASES, ids=IDS)
def test_bitwise_equal_penalised(case):
    import torch
    N, F, K = case
    Y, X, D = _integer_inputs(N, F, K, seed=3 * N + F + K)
    with _Penalty(0.7, 0.2):
        (x0, _), (x1, _) = _both_modes(Y, X, D, 'oop')
    (u0, _), _ = _both_modes(Y, X, D, 'oop')
    assert torch.equal(x0, x1), (case, int((x0 != x1).sum()))
    assert not torch.equal(x0, u0)       # the penalty was read
    del Y, X, D, x0, x1, u0
    _free()


@pytest.mark.parametrize('case', CASES, ids=IDS)
def test_against_float64_formula(case):
    """Random positive float32 inputs: X_out against the float64 formula with the cap and slack of
    test_gpu_bf16x6_paths.py; two runs give the same bits."""
    import numpy as np
    import torch
    N, F, K = case
    Y, X, D = _inputs(N, F, K, 'oop', seed=N + 2 * F + K)
    (x0, _), (x1, _) = _both_modes(Y, X, D, 'oop')
    with _Mode(0):
        again, _ = _step(Y, X, D, 'oop')
    assert torch.equal(x0, again)
    rows = _sample(N, 1024, np.random.RandomState(N % 9973 + K + F))
    xref = _x_ref(Y, X, D, rows)
    r = torch.as_tensor(rows, device='cuda')
    ex = [_rel(xo[r].double(), xref) for xo in (x0, x1)]
    print('\n%dx%dk%d: X_out %.3g / %.3g (mode 0 / mode 1)' % (N, F, K, ex[0], ex[1]))
    assert max(ex) < CAP, (case, ex)
    assert ex[0] <= 2.0 * ex[1] + SLACK, (case, ex)
    del Y, X, D, x0, x1, again
    _free()


@pytest.mark.parametrize('shape', SHAPES, ids=['%dk%d' % s for s in SHAPES])
def test_q_product_is_not_launched(shape):
    """The path claim, at run time: on the fused path the step brackets one x_update launch and no x_neg launch
    (Q = X . G is neither written nor read); mode 1 and the in-place step keep both launches."""
    N, K = shape
    Y, X, D = _integer_inputs(N, 64, K, seed=5)
    with _Mode(0):
        assert _launches(Y, X, D, 'oop') == (0, 1)
        assert _launches(Y, X, D, 'inplace') == (1, 1)
    with _Mode(1):
        assert _launches(Y, X, D, 'oop') == (1, 1)
    with _Mode(0), _Penalty(0.7, 0.2):
        assert _launches(Y, X, D, 'oop') == (0, 1)
    del Y, X, D
    _free()
