"""GPU: the two flat-reduction templates of csrc/reduce.hpp (reduce_partial_kernel, reduce_vector_kernel) through
entry points that use them.

Sum, order-exact: dcp_nmf_residual_* with x = 0 returns sqrt(sum y^2); the sum is compared BIT FOR BIT with a NumPy
model of the documented order -- every thread adds float64(T(y * y)) over its grid-stride elements in increasing
index, the six shift-down steps 32 .. 1 leave the wave's sum in lane 0, the four wave sums are added left to right,
the host adds the per-workgroup partials in workgroup order and takes the square root.
Max: dcp_l2_normalize_diff_* (one workgroup over the K row maxima) and the K-SVD sweep's max|D_new - D_old|
(kKsvdMdParts workgroups, then the host): the position of the maximum, NaN at that position, all-equal input.
Count: dcp_count_negative_* (a sum whose partials are integers)."""
import ctypes
import os
import re

import numpy as np
import pytest

gpu = pytest.mark.gpu

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def _constant(path, pattern):
    text = open(os.path.join(ROOT, 'decomp_amd', 'csrc', path)).read()
    return int(re.search(pattern, text).group(1))


RESID_BLOCKS = _constant('nmf.hip', r'struct NmfScalarWs \{\s*static constexpr int blocks = (\d+);')
MD_PARTS = _constant('ksvd.hpp', r'constexpr int kKsvdMdParts = (\d+);')
COUNT_CAP = 1024   # count_negative_api: grid_for(n, 1024)


def _dev(a):
    import torch
    return torch.from_numpy(np.ascontiguousarray(a)).cuda()


def _grid(n, cap):
    return max(1, min(cap, (n + 255) // 256))


# ---- the sum template ---------------------------------------------------------------------------------------------
def _model_sumsq(y, blocks, tree=True):
    """sum y^2 in the kernel's order (tree = False: the same per-thread sums added lane by lane instead)."""
    sq = (y * y).astype(np.float64)                      # squared in T, then widened
    stride = blocks * 256
    rounds = (sq.size + stride - 1) // stride
    padded = np.zeros(rounds * stride)
    padded[:sq.size] = sq
    acc = np.zeros(stride)
    for j in range(rounds):                              # a thread's elements, in increasing index
        acc = acc + padded[j * stride:(j + 1) * stride]
    v = acc.reshape(blocks, 4, 64)
    if tree:
        for o in (32, 16, 8, 4, 2, 1):                   # lane l += lane l + o (lane 0 only sees lanes in range)
            v = v + np.concatenate([v[..., o:], v[..., :o]], axis=-1)
        wave = v[..., 0]
    else:
        wave = np.zeros((blocks, 4))
        for lane in range(64):
            wave = wave + v[..., lane]
    part = ((wave[:, 0] + wave[:, 1]) + wave[:, 2]) + wave[:, 3]
    total = 0.0
    for b in range(blocks):                              # the host, in workgroup order
        total += float(part[b])
    return total


def _mixed(rng, n, dt):
    """Full mantissas on thirty binary scales: many addends of every size, so the sums round all the way (a few
    dominant values would hide the order, and float32 squares of ONE scale add up exactly in double)."""
    return (rng.uniform(1, 2, n) * 2.0 ** -rng.integers(0, 30, n)).astype(dt)


SUM_SIZES = [1, 255, 256, 257, RESID_BLOCKS * 256 + 1]


SEED = 3


def test_sum_model_orders_disagree():
    """The inputs tell summation orders apart (host only): at every size past one wave the kernel's order gives
    other bits than the same per-thread sums added lane by lane, or than NumPy's pairwise sum; at the largest size
    also after the square root."""
    for dt in (np.float32, np.float64):
        for n in SUM_SIZES[1:]:
            y = _mixed(np.random.default_rng(SEED), n, dt)
            tree = _model_sumsq(y, RESID_BLOCKS)
            others = (_model_sumsq(y, RESID_BLOCKS, tree=False), float(np.sum((y * y).astype(np.float64))))
            assert any(tree != o for o in others), (dt, n)
            if n == SUM_SIZES[-1]:
                assert any(np.sqrt(tree) != np.sqrt(o) for o in others), (dt, n)


@gpu
@pytest.mark.parametrize('n', SUM_SIZES)
@pytest.mark.parametrize('dt', ['float32', 'float64'])
def test_residual_sum_is_order_exact(dt, n):
    from decomp_amd import _arrays, _hip
    y = _mixed(np.random.default_rng(SEED), n, dt)
    Y, X, D = _dev(y.reshape(1, n)), _dev(np.zeros((1, 1), dt)), _dev(np.ones((1, n), dt))
    lib, h = _arrays.lib_handle(Y)
    out = ctypes.c_double(-1.0)
    name = 'dcp_nmf_residual_' + _arrays.suffix(Y)
    _hip.check(h, getattr(lib, name)(h, _arrays.ptr(Y), None, _arrays.ptr(X), _arrays.ptr(D), 1, n, 1,
                                     ctypes.byref(out)), name)
    want = float(np.sqrt(_model_sumsq(y, RESID_BLOCKS)))
    print('residual', dt, n, out.value.hex(), want.hex())
    assert out.value == want


# ---- the max template, one workgroup: dcp_l2_normalize_diff ---------------------------------------------------------
def _normalize_diff(ref):
    """max |ref - 1| over K rows of one element: U = 1 normalises to exactly 1."""
    from decomp_amd import _arrays, _hip
    K = ref.size
    U, R = _dev(np.ones((K, 1), ref.dtype)), _dev(ref.reshape(K, 1))
    import torch
    out = torch.empty_like(U)
    lib, h = _arrays.lib_handle(U)
    md = ctypes.c_double(-1.0)
    name = 'dcp_l2_normalize_diff_' + _arrays.suffix(U)
    _hip.check(h, getattr(lib, name)(h, _arrays.ptr(U), _arrays.ptr(R), _arrays.ptr(out), K, 1, 1,
                                     ctypes.byref(md)), name)
    assert np.all(out.cpu().numpy() == 1)
    return md.value


@gpu
@pytest.mark.parametrize('K', [1, 255, 256, 257, 600])
@pytest.mark.parametrize('dt', ['float32', 'float64'])
def test_vector_max_positions_nan_and_equal(dt, K):
    rng = np.random.default_rng(K)
    v = (rng.integers(0, 512, K) / 1024.0).astype(dt)    # 1 + v and (1 + v) - 1 are exact
    for pos in sorted({0, K - 1}):
        d = v.copy()
        d[pos] = 0.75
        assert _normalize_diff(1 + d) == 0.75
        d[pos] = np.nan
        assert np.isnan(_normalize_diff(1 + d))
    assert _normalize_diff(np.full(K, 1.375, dt)) == 0.375


# ---- the max template, many workgroups: the K-SVD sweep's maxdiff ---------------------------------------------------
def _sweep(y, x, D):
    from decomp_amd import _arrays, _hip
    Y, X, Dt = _dev(y), _dev(x), _dev(D)
    N, F = y.shape
    K = D.shape[0]
    lib, h = _arrays.lib_handle(Y)
    md = ctypes.c_double(-1.0)
    name = 'dcp_ksvd_sweep_' + _arrays.suffix(Y)
    _hip.check(h, getattr(lib, name)(h, _arrays.ptr(Y), _arrays.ptr(X), _arrays.ptr(Dt), N, F, K, 1,
                                     ctypes.byref(md)), name)
    return Dt.cpu().numpy(), md.value


# K x F elements around one workgroup (256) and around the grid cap (kKsvdMdParts workgroups of 256)
MAX_SHAPES = [(1, 255), (1, 256), (1, 257), (3, (MD_PARTS * 256 - 1) // 3), (4, MD_PARTS * 64),
              (5, (MD_PARTS * 256 + 1) // 5)]


@gpu
@pytest.mark.parametrize('K,F', MAX_SHAPES)
@pytest.mark.parametrize('dt', ['float32', 'float64'])
def test_partial_max_positions_nan_and_zero(dt, K, F):
    n = K * F
    assert n in (255, 256, 257, MD_PARTS * 256 - 1, MD_PARTS * 256, MD_PARTS * 256 + 1)
    last_group = min(n - 1, (_grid(n, MD_PARTS) - 1) * 256 + 5)    # an element of the last workgroup
    for q in sorted({0, n - 1, last_group}):
        k, p = divmod(q, F)
        j = (p + 1) % F
        # one row coded by atom k alone: d_k = e_j and y = 3 e_j + 4 e_p give d' = (3 e_j + 4 e_p) / 5, so
        # |d' - d| is 0.8 at p, 0.4 at j and 0 elsewhere; the other atoms have no support and stay
        D = np.zeros((K, F), dt)
        D[:, 0] = 1
        D[k] = 0
        D[k, j] = 1
        y = np.zeros((1, F), dt)
        y[0, j], y[0, p] = 3, 4
        x = np.zeros((1, K), dt)
        x[0, k] = 1
        Dn, md = _sweep(y, x, D)
        diff = np.abs(Dn - D)
        assert int(np.argmax(diff)) == q and md == float(diff.reshape(-1)[q]), (q, md)
        assert abs(md - 0.8) < 1e-6
        # NaN at q, nothing coded: D stays as it is and the NaN wins
        Dnan = D.copy()
        Dnan.reshape(-1)[q] = np.nan
        _, md = _sweep(y, np.zeros((1, K), dt), Dnan)
        assert np.isnan(md)
    _, md = _sweep(np.ones((1, F), dt), np.zeros((1, K), dt), np.full((K, F), 0.5, dt))
    assert md == 0.0


# ---- count_negative -------------------------------------------------------------------------------------------------
def _count_negative(x):
    from decomp_amd import _arrays, _hip
    X = _dev(x)
    lib, h = _arrays.lib_handle(X)
    cnt = ctypes.c_int64(-1)
    name = 'dcp_count_negative_' + _arrays.suffix(X)
    _hip.check(h, getattr(lib, name)(h, _arrays.ptr(X), x.size, ctypes.byref(cnt)), name)
    return cnt.value


@gpu
@pytest.mark.parametrize('n', [1, 257, COUNT_CAP * 256 + 1])
@pytest.mark.parametrize('dt', ['float32', 'float64'])
def test_count_negative(dt, n):
    assert _grid(n, COUNT_CAP) == min(COUNT_CAP, (n + 255) // 256)
    x = np.abs(_mixed(np.random.default_rng(n), n, dt))
    assert _count_negative(x) == 0
    assert _count_negative(-x - 1) == n
    some = x.copy()
    picks = sorted({0, n - 1, n // 2})
    some[picks] = np.nan                                  # fails `x >= 0`, so it counts
    assert _count_negative(some) == len(picks)
    some[picks] = -0.0                                    # -0 >= 0 holds
    assert _count_negative(some) == 0
    mixed = np.where(np.arange(n) % 3 == 0, -x - 1, x)
    assert _count_negative(mixed) == (n + 2) // 3
