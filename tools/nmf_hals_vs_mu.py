#!/usr/bin/env python3
"""HALS (method='hals', dcp_nmf_hals_*) against the multiplicative update (dcp_nmf_mu_*, l2) on one planted
non-negative problem, default float32 65536 x 4096, k = 256, both started from x = ones and the same D:

  * ms per iteration of each loop: a warm-up, then --steps iterations between two events, median of --runs;
  * the relative residual |Y - xD| / |Y| after every iteration (the loops' resid_trace, a separate run), the
    iterations each method needs to reach a common residual (what MU reaches after --iters iterations), and
    the wall time that takes at the measured ms per iteration.

Prints one line per measurement and a JSON summary line.
    python tools/nmf_hals_vs_mu.py [--rows 65536] [--f 4096] [--k 256] [--steps 20] [--runs 5] [--iters 200]"""
import argparse
import ctypes
import json
import os
import statistics
import sys

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))

import torch  # noqa: E402
from decomp_amd import _arrays, _hip  # noqa: E402


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument('--rows', type=int, default=65536)
    ap.add_argument('--f', type=int, default=4096)
    ap.add_argument('--k', type=int, default=256)
    ap.add_argument('--steps', type=int, default=20)
    ap.add_argument('--runs', type=int, default=5)
    ap.add_argument('--iters', type=int, default=200)
    ap.add_argument('--dtype', choices=['float32', 'float64'], default='float32')
    a = ap.parse_args()
    N, F, K = a.rows, a.f, a.k
    dt = getattr(torch, a.dtype)
    sfx = 'f32' if dt == torch.float32 else 'f64'
    ctype = ctypes.c_float if sfx == 'f32' else ctypes.c_double
    g = torch.Generator(device='cuda')
    g.manual_seed(0)
    x0 = torch.rand((N, K), generator=g, device='cuda', dtype=dt) * (torch.rand((N, K), generator=g, device='cuda') < 0.5)
    D0 = torch.rand((K, F), generator=g, device='cuda', dtype=dt) * (torch.rand((K, F), generator=g, device='cuda') < 0.5)
    Y = x0 @ D0 + 0.01 * torch.rand((N, F), generator=g, device='cuda', dtype=dt)
    del x0, D0
    Dstart = torch.rand((K, F), generator=g, device='cuda', dtype=dt) + 0.1
    _arrays.l2_normalize_(Dstart, strict=True)
    ynorm = float(torch.linalg.vector_norm(Y.double()))
    lib, h = _arrays.lib_handle(Y)
    it = ctypes.c_int(0)

    def call(method, x, D, n, trace=None):
        if method == 'hals':
            rc = getattr(lib, 'dcp_nmf_hals_' + sfx)(h, _arrays.ptr(Y), _arrays.ptr(x), _arrays.ptr(D), N, F, K,
                                                      ctype(0.0), n + 1, ctypes.byref(it), None, trace)
        else:
            rc = getattr(lib, 'dcp_nmf_mu_' + sfx)(h, _arrays.ptr(Y), None, _arrays.ptr(x), _arrays.ptr(D), N, F, K,
                                                    _hip.LIK_L2, ctype(0.0), n + 1, ctypes.byref(it), None, trace)
        _hip.check(h, rc, method)

    result = {}
    for method in ('mu', 'hals'):
        x = torch.ones((N, K), device='cuda', dtype=dt)
        D = Dstart.clone()
        call(method, x, D, 3)   # warm-up (workspace, code objects)
        samples = []
        for _ in range(a.runs):
            torch.cuda.synchronize()
            e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
            e0.record()
            call(method, x, D, a.steps)
            e1.record()
            torch.cuda.synchronize()
            samples.append(e0.elapsed_time(e1) / a.steps)
        ms = statistics.median(samples)
        x = torch.ones((N, K), device='cuda', dtype=dt)
        D = Dstart.clone()
        trace = (ctype * (a.iters + 1))()
        call(method, x, D, a.iters, trace)
        rel = [float(trace[i]) / ynorm for i in range(a.iters)]
        result[method] = {'ms_per_iter': round(ms, 4), 'samples': [round(s, 4) for s in samples], 'rel_resid': rel}
        print('%-5s %dx%d k=%d %s: %.3f ms/iter (median of %d); rel. residual after 1/10/%d iterations: %.3e %.3e %.3e'
              % (method, N, F, K, a.dtype, ms, a.runs, a.iters, rel[0], rel[min(9, a.iters - 1)], rel[-1]))

    target = result['mu']['rel_resid'][-1]
    summary = {}
    for method in ('mu', 'hals'):
        r = result[method]['rel_resid']
        n = next((i + 1 for i, v in enumerate(r) if v <= target), None)
        ms = result[method]['ms_per_iter']
        summary[method] = {'ms_per_iter': ms, 'iters_to_target': n,
                           'ms_to_target': None if n is None else round(n * ms, 2)}
        print('%-5s reaches rel. residual %.4e after %s iterations = %s ms'
              % (method, target, n, 'n/a' if n is None else '%.1f' % (n * ms)))
    ratio = round(result['hals']['ms_per_iter'] / result['mu']['ms_per_iter'], 3)
    print('hals / mu time per iteration: %.3f' % ratio)
    for method in result:
        del result[method]['rel_resid']
    print(json.dumps({'shape': [N, F, K], 'dtype': a.dtype, 'steps': a.steps, 'runs': a.runs, 'iters': a.iters,
                      'target_rel_resid': target, 'summary': summary, 'hals_over_mu_per_iter': ratio,
                      'timing': result}))


if __name__ == '__main__':
    main()
