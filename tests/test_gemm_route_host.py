"""CPU: the GEMM front end routes every product as it did before the route existed.

tests/golden/gemm_route_golden.npz holds what plan_splits() followed by gemm() handed to the four GEMM launchers
(tile, core-side dimensions, klen, ksplits) before gemm_route() was written, recorded on the host over
4 dtypes x 3 forms x tile selectors 0..5 x M, N in {1, 20, 32, 33, 64, 65, 128, 129, 200, 256, 260, 512, 1024,
4096} x K in {16, 256, 1024, 8192, 65536} x scratch present / absent (complex) x one / two B segments (the first
ceil(N / 2) wide, N >= 2) x the five split plans of `plans` (row 0: none).  Kept of that grid, so that the two
passes take seconds: the automatic tile whole; the forced selectors 1..5 with one B segment and M, N in {20, 33, 64,
129, 260, 1024}.  dcp_debug_gemm_route() must give every row back exactly, with the pair schedule and with the plain
one (PIPE is the only column the knob changed in the recording)."""
import ctypes
import os

import numpy as np
import pytest

GOLD = os.path.join(os.path.dirname(os.path.abspath(__file__)), 'golden', 'gemm_route_golden.npz')
IN = ('dtype', 'form', 'M', 'N', 'K', 'n_b1', 'tile_sel', 'ext_ws')
OUT = ('core', 'image', 'BM', 'BN', 'BK', 'WM', 'WN', 'PIPE', 'core_M', 'core_N', 'core_K', 'klen', 'ksplits')

# (core, BM, BN, BK, WM, WN, PIPE) of every tile typedef of gemm.hpp, and the generic core's tile
TILES = {
    'CfgHuge': (0, 256, 256, 16, 64, 64, 0), 'CfgLarge': (0, 128, 128, 16, 64, 64, 0),
    'CfgMid': (0, 128, 128, 64, 32, 64, 0), 'CfgSmall': (0, 64, 64, 16, 32, 32, 0),
    'CfgFlat': (0, 32, 128, 32, 32, 32, 0), 'CfgTall': (0, 128, 32, 32, 32, 32, 0),
    'CfgHugeDeep': (0, 256, 256, 32, 64, 64, 0), 'CfgLargeX': (0, 128, 128, 16, 64, 64, 3),
    'CfgHugeDeepX': (0, 256, 256, 32, 64, 64, 3), 'CfgSmallDeep': (0, 64, 64, 64, 32, 32, 0),
    'F64Tile': (1, 128, 128, 16, 32, 32, 0), 'F64Sq64': (1, 64, 64, 16, 32, 32, 0),
    'F64Tall64': (1, 128, 64, 16, 32, 32, 0), 'F64Tall32': (1, 128, 32, 16, 32, 32, 0),
    'F64Flat64': (1, 64, 128, 16, 32, 32, 0), 'F64Flat32': (1, 32, 128, 16, 32, 32, 0),
    'generic': (2, 64, 64, 16, 0, 0, 0),
}


@pytest.fixture(scope='module')
def gold():
    z = np.load(GOLD)
    return {k: z[k] for k in z.files}


def test_golden_covers_every_core_image_and_tile(gold):
    assert set(np.unique(gold['core'])) == {0, 1, 2}
    assert set(np.unique(gold['image'])) == {0, 1, 2, 3}
    seen = set()
    for pipe in ('PIPE', 'PIPE_plain'):
        cols = np.stack([gold[k].astype(np.int64) for k in ('core', 'BM', 'BN', 'BK', 'WM', 'WN', pipe)], 1)
        seen |= set(map(tuple, np.unique(cols, axis=0).tolist()))
    assert seen == set(TILES.values())


def _route_all(lib, gold):
    plans = gold['plans'].tolist()
    fn = lib.dcp_debug_gemm_route
    cols = [gold[k].tolist() for k in IN] + [gold['plan'].tolist()]
    got = np.full((len(cols[0]), 13), -1, np.int32)
    outp = got.ctypes.data   # row i is written in place
    for dt, form, M, N, K, nb1, tile, ext, plan in zip(*cols):
        t, s, b = plans[plan]
        assert fn(dt, form, M, N, K, nb1, tile, ext, t, s, b, outp) == 0
        outp += 52
    return got


@pytest.mark.parametrize('plain', [0, 1])
def test_route_matches_recorded_launches(gold, plain):
    from decomp_amd import _hip
    lib = _hip.load()
    want = np.stack([gold[k].astype(np.int32) for k in OUT], 1)
    if plain:
        want[:, OUT.index('PIPE')] = gold['PIPE_plain']
    prev = lib.dcp_debug_tn_plain(plain)
    try:
        got = _route_all(lib, gold)
    finally:
        lib.dcp_debug_tn_plain(prev)
    bad = np.nonzero((got != want).any(1))[0]
    first = [(dict((k, int(gold[k][i])) for k in IN + ('plan',)), got[i].tolist(), want[i].tolist()) for i in bad[:5]]
    assert len(bad) == 0, '%d of %d rows differ, first: %s' % (len(bad), len(want), first)


def test_route_rejects_bad_arguments():
    from decomp_amd import _hip
    lib = _hip.load()
    out = (ctypes.c_int32 * 13)()
    outp = ctypes.cast(out, ctypes.c_void_p)
    assert lib.dcp_debug_gemm_route(4, 0, 8, 8, 8, 0, 0, 0, 0, 0, 0, outp) == -1
    assert lib.dcp_debug_gemm_route(0, 3, 8, 8, 8, 0, 0, 0, 0, 0, 0, outp) == -1
    assert lib.dcp_debug_gemm_route(0, 0, 8, 8, 8, 8, 0, 0, 0, 0, 0, outp) == -1
    assert lib.dcp_debug_gemm_route(0, 0, 8, 8, 8, 0, 0, 0, 0, 0, 0, None) == -1
