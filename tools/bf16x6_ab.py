"""Kernel A/B: the split-bf16 core (dcp_gemm_bf16x6_f32) against the fp32 MFMA core (dcp_gemm_f32) on the two
products of the NMF step, interleaved in one process, median of R timed launches each (random operands)."""
import argparse
import json
import sys
import os

import torch

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
from decomp_amd import _arrays, _hip  # noqa: E402

SHAPES = {'nt_x_update': (0, 65536, 256, 4096, 1), 'tn_stats': (2, 256, 4352, 65536, 15)}


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument('--reps', type=int, default=20)
    args = ap.parse_args()
    out = {}
    for name, (form, M, N, K, ks) in SHAPES.items():
        sa = (M, K) if form == 0 else (K, M)
        sb = (N, K) if form == 0 else (K, N)
        a = torch.rand(sa, device='cuda')
        b = torch.rand(sb, device='cuda')
        c = torch.empty((M, N), device='cuda')
        lib, h = _arrays.lib_handle(a)
        calls = {
            'bf16x6': lambda: lib.dcp_gemm_bf16x6_f32(h, form, _arrays.ptr(a), _arrays.ptr(b), _arrays.ptr(c),
                                                      M, N, K, ks),
            'fp32': lambda: lib.dcp_gemm_f32(h, form, _arrays.ptr(a), _arrays.ptr(b), _arrays.ptr(c), M, N, K, ks, 0),
        }
        ms = {k: [] for k in calls}
        for k, f in calls.items():   # warm-up
            for _ in range(3):
                _hip.check(h, f(), k)
        torch.cuda.synchronize()
        for _ in range(args.reps):
            for k, f in calls.items():
                e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
                e0.record()
                _hip.check(h, f(), k)
                e1.record()
                e1.synchronize()
                ms[k].append(e0.elapsed_time(e1))
        flop = 2.0 * M * N * K
        res = {}
        for k, v in ms.items():
            v.sort()
            med = v[len(v) // 2]
            res[k] = {'ms_median': round(med, 4), 'ms_min': round(v[0], 4), 'ms_max': round(v[-1], 4),
                      'fp32_equiv_tflops': round(flop / med / 1e9, 1)}
        res['speedup'] = round(res['fp32']['ms_median'] / res['bf16x6']['ms_median'], 3)
        out[name] = {'shape': [form, M, N, K, ks], **res}
        del a, b, c
        torch.cuda.empty_cache()
    print(json.dumps(out))


if __name__ == '__main__':
    main()
