#!/usr/bin/env python3
"""What one rank's step of row-sharded HALS costs: the rows one rank holds at the headline shape on 8 GPUs
(Y = 8192 x 4096, k = 256, float32, a planted problem as in tools/nmf_hals_vs_mu.py), on one GPU, for

  single  dcp_nmf_hals_f32 (the one-GPU loop);
  inlib   dcp_nmf_hals_sharded_f32 on a 1-rank RCCL communicator (the loop a rank of a multi-GPU run executes;
          the all-reduce is the identity, so this is the compute side plus the cost of issuing it);
  python  HipHalsStepBackend (dcp_nmf_hals_stats_* / dcp_nmf_hals_update_*) driven by sharded.mu_loop.

Each: a warm-up of 3 iterations, then --runs runs of --steps iterations with tol = 0 between two events; the
median ms per iteration.  --mode picks one loop (for a kernel trace of it alone).  Prints one line per loop and
a JSON summary line.
    python tools/nmf_hals_sharded_step.py [--rows 8192] [--f 4096] [--k 256] [--steps 20] [--runs 5]
                                          [--mode all|single|inlib|python]"""
import argparse
import ctypes
import json
import os
import statistics
import sys

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))

import torch  # noqa: E402
from decomp_amd import _arrays, _hip, sharded  # noqa: E402


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument('--rows', type=int, default=8192)
    ap.add_argument('--f', type=int, default=4096)
    ap.add_argument('--k', type=int, default=256)
    ap.add_argument('--steps', type=int, default=20)
    ap.add_argument('--runs', type=int, default=5)
    ap.add_argument('--mode', choices=['all', 'single', 'inlib', 'python'], default='all')
    a = ap.parse_args()
    N, F, K = a.rows, a.f, a.k
    torch.cuda.set_device(0)
    g = torch.Generator(device='cuda')
    g.manual_seed(0)
    x0 = torch.rand((N, K), generator=g, device='cuda') * (torch.rand((N, K), generator=g, device='cuda') < 0.5)
    D0 = torch.rand((K, F), generator=g, device='cuda') * (torch.rand((K, F), generator=g, device='cuda') < 0.5)
    Y = x0 @ D0 + 0.01 * torch.rand((N, F), generator=g, device='cuda')
    del x0, D0
    Dstart = torch.rand((K, F), generator=g, device='cuda') + 0.1
    _arrays.l2_normalize_(Dstart, strict=True)
    lib, h = _arrays.lib_handle(Y)
    it = ctypes.c_int(0)

    def single(x, D, n):
        _hip.check(h, lib.dcp_nmf_hals_f32(h, _arrays.ptr(Y), _arrays.ptr(x), _arrays.ptr(D), N, F, K,
                                           ctypes.c_float(0.0), n + 1, ctypes.byref(it), None, None),
                   'dcp_nmf_hals_f32')

    def inlib(x, D, n):
        assert sharded.hals_solve_in_library(Y, x, D, 0.0, n + 1) == n + 1

    def python(x, D, n):
        backend = sharded.HipHalsStepBackend(Y, x, D)
        itp, _ = sharded.mu_loop(backend, D, 0.0, n + 1, new_like=torch.empty_like)
        assert itp == n + 1

    loops = {'single': single, 'inlib': inlib, 'python': python}
    modes = ['single', 'python', 'inlib'] if a.mode == 'all' else [a.mode]
    result = {}
    for mode in modes:
        if mode == 'inlib':
            assert sharded.attach_communicator(Dstart), 'no RCCL communicator'
            assert sharded.communicator_kind(Dstart) == 'rccl'
        x = torch.ones((N, K), device='cuda')
        D = Dstart.clone()
        loops[mode](x, D, 3)   # warm-up (workspace, code objects, communicator)
        samples = []
        for _ in range(a.runs):
            x = torch.ones((N, K), device='cuda')
            D = Dstart.clone()
            torch.cuda.synchronize()
            e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
            e0.record()
            loops[mode](x, D, a.steps)
            e1.record()
            torch.cuda.synchronize()
            samples.append(e0.elapsed_time(e1) / a.steps)
        if mode == 'inlib':
            sharded.detach_communicator(Dstart)
        ms = statistics.median(samples)
        result[mode] = {'ms_per_iter': round(ms, 4), 'samples': [round(s, 4) for s in samples]}
        print('%-6s %dx%d k=%d float32: %.4f ms/iter (median of %d runs of %d)' % (mode, N, F, K, ms, a.runs,
                                                                                    a.steps))
    summary = {'shape': [N, F, K], 'steps': a.steps, 'runs': a.runs, 'timing': result}
    if 'single' in result:
        for mode in ('inlib', 'python'):
            if mode in result:
                summary[mode + '_over_single'] = round(result[mode]['ms_per_iter'] / result['single']['ms_per_iter'],
                                                       4)
    print(json.dumps(summary))


if __name__ == '__main__':
    main()
