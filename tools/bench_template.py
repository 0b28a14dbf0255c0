#!/usr/bin/env python3
"""Timing record of decomp_amd.template_matching on one GPU; prints one JSON line.

    python tools/bench_template.py [--reps 20]

Shape A (B = 64, N = 4096, T = 16, S = 64, float32, stride 1, SAME, acc_ista, lasso_iter = 10):
  us per structured LASSO iteration  ((time of 110 iterations - time of 10) / 100, no early stop)
  us of the dictionary statistics (XXt, yX) and of the D update (Gershgorin + step + l2 + max|dD|)
  ms per outer iteration of solve (batch)
Shape B (B = 16, N = 2048, T = 8, S = 64, same settings): ms per outer iteration, beside the reference's
4.4 s per outer iteration measured on a CPU for that shape.
"""
import argparse
import ctypes
import json
import os
import sys
import time

import numpy as np

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))


def _problem(B, N, T, S, seed=0):
    import torch
    rng = np.random.RandomState(seed)
    y = torch.from_numpy(rng.randn(B, N).astype(np.float32)).cuda()
    D = rng.randn(T, S).astype(np.float32)
    D /= np.linalg.norm(D, axis=1, keepdims=True)
    return y, torch.from_numpy(D).cuda()


def _timed(fn, reps):
    import torch
    fn()
    torch.cuda.synchronize()
    ts = []
    for _ in range(reps):
        t0 = time.perf_counter()
        fn()
        torch.cuda.synchronize()
        ts.append(time.perf_counter() - t0)
    return float(np.median(ts))


def main():
    import torch
    from decomp_amd import template_matching as tm, _arrays, _hip
    ap = argparse.ArgumentParser()
    ap.add_argument('--reps', type=int, default=20)
    a = ap.parse_args()
    out = {'workload': 'template_matching', 'dtype': 'float32', 'stride': 1, 'padding': 'SAME',
           'lasso_method': 'acc_ista', 'lasso_iter': 10}

    B, N, T, S = 64, 4096, 16, 64
    C = tm._coef_size(S, N, 1, 'SAME')
    y, D = _problem(B, N, T, S)
    x = torch.zeros((B, T, C), dtype=torch.float32, device='cuda')
    t10 = _timed(lambda: tm._lasso(y, D, x.zero_(), 0.1, 1, 'SAME', 'acc_ista', 10, 0.0), a.reps)
    t110 = _timed(lambda: tm._lasso(y, D, x.zero_(), 0.1, 1, 'SAME', 'acc_ista', 110, 0.0), a.reps)
    tm._lasso(y, D, x.zero_(), 0.1, 1, 'SAME', 'acc_ista', 10, 0.0)
    XXt = torch.empty((T * S, T * S), dtype=torch.float32, device='cuda')
    yX = torch.empty((T * S,), dtype=torch.float32, device='cuda')
    D2 = D.clone()
    t_d = _timed(lambda: tm._dstep(y, x, D2.copy_(D), XXt, yX, 1, 'SAME', 0), a.reps)
    lib, h = _arrays.lib_handle(y)
    lib.dcp_profile_enable(h, 1)
    lib.dcp_profile_reset(h)
    for _ in range(a.reps):
        tm._dstep(y, x, D2.copy_(D), XXt, yX, 1, 'SAME', 0)
    ms, cnt = ctypes.c_double(0), ctypes.c_int64(0)
    _hip.check(h, lib.dcp_profile_read(h, _hip.PROF_STATS, ctypes.byref(ms), ctypes.byref(cnt)), 'profile')
    lib.dcp_profile_enable(h, 0)
    stats_us = 1e3 * ms.value / max(cnt.value, 1)
    outer = _timed(lambda: tm.solve(y, D, 0.1, maxiter=4, tol=0.0, lasso_iter=10), max(3, a.reps // 4)) / 3
    out['A'] = {'B': B, 'N': N, 'T': T, 'S': S, 'C': C,
                'lasso_us_per_iter': round(1e6 * (t110 - t10) / 100, 2),
                'lasso_call_10_iter_us': round(1e6 * t10, 1),
                'dstep_stats_us': round(stats_us, 1),
                'dstep_update_us': round(1e6 * t_d - stats_us, 1),
                'dstep_call_us': round(1e6 * t_d, 1),
                'outer_iter_ms': round(1e3 * outer, 3)}

    B, N, T, S = 16, 2048, 8, 64
    y, D = _problem(B, N, T, S, seed=1)
    outer = _timed(lambda: tm.solve(y, D, 0.1, maxiter=4, tol=0.0, lasso_iter=10), max(3, a.reps // 4)) / 3
    out['B'] = {'B': B, 'N': N, 'T': T, 'S': S, 'outer_iter_ms': round(1e3 * outer, 3),
                'reference_cpu_outer_iter_ms': 4400.0,
                'speedup_vs_reference_cpu': round(4400.0 / (1e3 * outer), 1)}
    print(json.dumps(out))


if __name__ == '__main__':
    main()
