"""In-kernel stamps of the split-bf16 256 x 256 K loop (diagnostic build only).

Build a second library with the stamps compiled in, e.g.
    hipcc --offload-arch=gfx950 -O3 -std=c++17 -fPIC -Iinclude -DDCP_X6_STAMPS -c decomp_amd/csrc/util.hip -o util_stamps.o
    hipcc --offload-arch=gfx950 -shared -fPIC -o libdecomp_stamps.so util_stamps.o <the other objects of build/obj>
and run  python3 tools/bf16x6_stamps.py --lib libdecomp_stamps.so.  It launches the two products of the NMF step
through dcp_gemm_bf16x6_f32 (NT 65536 x 256 x 4096, TN 256 x 4352 x 65536 in 15 splits, random operands), reads the
clock sums of workgroup 0 (gemm_mfma_bf16x6.hpp, DCP_X6_STAMPS) and prints, per product, the two stamped segments
as shares of a K block, the stamps' own cost taken off: one JSON line.  The run time of this build means nothing."""
import argparse
import ctypes
import json
import os
import sys

import torch

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
from decomp_amd import _hip  # noqa: E402

SHAPES = {'nt_x_update': (0, 65536, 256, 4096, 1), 'tn_stats': (2, 256, 4352, 65536, 15)}


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument('--lib', required=True, help='library built with -DDCP_X6_STAMPS')
    args = ap.parse_args()
    _hip.LIB_PATH = os.path.abspath(args.lib)
    from decomp_amd import _arrays
    out = {}
    for name, (form, M, N, K, ks) in SHAPES.items():
        a = torch.rand((M, K) if form == 0 else (K, M), device='cuda')
        b = torch.rand((N, K) if form == 0 else (K, N), device='cuda')
        c = torch.empty((M, N), device='cuda')
        lib, h = _arrays.lib_handle(a)
        for _ in range(3):
            _hip.check(h, lib.dcp_gemm_bf16x6_f32(h, form, _arrays.ptr(a), _arrays.ptr(b), _arrays.ptr(c), M, N, K, ks),
                       name)
        buf = (ctypes.c_ulonglong * 128)()
        assert lib.dcp_x6_stamps_read(buf) == 0
        waves = []
        for w in range(16):
            sa, sb, span, n, cost = buf[8 * w:8 * w + 5]
            # a block holds four stamps; each of the two segments ends in one
            block = span / (n - 1) - 4 * cost
            waves.append(((sa / n - cost) / block, (sb / n - cost) / block, block, cost, n))
        waves.sort()
        out[name] = {
            'shape': [form, M, N, K, ks], 'blocks_stamped': waves[0][4], 'stamp_cycles': waves[0][3],
            'block_cycles_median': round(sorted(w[2] for w in waves)[8], 1),
            'share_start_to_first_mfma': {'min': round(waves[0][0], 4), 'median': round(waves[8][0], 4),
                                          'max': round(waves[-1][0], 4)},
            'share_group0_end_to_barrier_exit': {'min': round(min(w[1] for w in waves), 4),
                                                 'median': round(sorted(w[1] for w in waves)[8], 4),
                                                 'max': round(max(w[1] for w in waves), 4)},
        }
        del a, b, c
        torch.cuda.empty_cache()
    print(json.dumps(out))


if __name__ == '__main__':
    main()
