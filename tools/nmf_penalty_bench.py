#!/usr/bin/env python3
"""The L1/L2 penalty on the NMF codes (dcp_set_nmf_penalty): penalised against unpenalised iterations of the MU
(l2, no mask) and HALS loops, float32, default product mode.  Times dcp_nmf_mu_f32 / dcp_nmf_hals_f32 per
iteration (tol = 0), median of --runs runs of --steps iterations, the two variants of a case alternating run by
run in one process.  Shapes: 65536 x 4096, k = 256, and one rank's rows of it on 8 GPUs (8192 x 4096: the split
x-update paths).  Prints one line per case and a JSON summary line.
    python tools/nmf_penalty_bench.py [--steps 20] [--runs 5] [--l1 1e-3] [--l2 1e-3]"""
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
    ap.add_argument('--steps', type=int, default=20)
    ap.add_argument('--runs', type=int, default=5)
    ap.add_argument('--l1', type=float, default=1e-3)
    ap.add_argument('--l2', type=float, default=1e-3)
    a = ap.parse_args()
    F, K = 4096, 256
    lib, h = _arrays.lib_handle(torch.empty(1, device='cuda'))
    result = {}
    for N in (65536, 8192):
        g = torch.Generator(device='cuda')
        g.manual_seed(1)
        Y = torch.rand((N, F), generator=g, device='cuda')
        D0 = torch.rand((K, F), generator=g, device='cuda') + 0.05
        _arrays.l2_normalize_(D0, strict=True)
        for method in ('mu', 'hals'):
            samples = {'plain': [], 'penalised': []}
            finite = True
            for r in range(a.runs + 1):   # run 0: warm-up
                for variant in ('plain', 'penalised'):
                    pen = (a.l1, a.l2) if variant == 'penalised' else (0.0, 0.0)
                    D, x = D0.clone(), torch.ones((N, K), device='cuda')
                    it = ctypes.c_int(0)
                    _hip.check(h, lib.dcp_set_nmf_penalty(h, pen[0], pen[1]), 'dcp_set_nmf_penalty')
                    torch.cuda.synchronize()
                    e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
                    e0.record()
                    if method == 'mu':
                        rc = lib.dcp_nmf_mu_f32(h, _arrays.ptr(Y), None, _arrays.ptr(x), _arrays.ptr(D), N, F, K,
                                                _hip.LIK_L2, ctypes.c_float(0.0), a.steps + 1, ctypes.byref(it),
                                                None, None)
                    else:
                        rc = lib.dcp_nmf_hals_f32(h, _arrays.ptr(Y), _arrays.ptr(x), _arrays.ptr(D), N, F, K,
                                                  ctypes.c_float(0.0), a.steps + 1, ctypes.byref(it), None, None)
                    _hip.check(h, rc, 'dcp_nmf_%s_f32' % method)
                    e1.record()
                    torch.cuda.synchronize()
                    if r > 0:
                        samples[variant].append(e0.elapsed_time(e1) / a.steps)
                    finite = finite and bool(torch.isfinite(D).all()) and bool(torch.isfinite(x).all())
            _hip.check(h, lib.dcp_set_nmf_penalty(h, 0.0, 0.0), 'dcp_set_nmf_penalty')
            plain, penal = statistics.median(samples['plain']), statistics.median(samples['penalised'])
            spread = (max(samples['plain']) - min(samples['plain'])) / plain
            name = '%s_%dx%dk%d' % (method, N, F, K)
            result[name] = {'plain_ms': round(plain, 4), 'penalised_ms': round(penal, 4),
                            'ratio': round(penal / plain, 4), 'plain_spread': round(spread, 4),
                            'plain_samples': [round(s, 4) for s in samples['plain']],
                            'penalised_samples': [round(s, 4) for s in samples['penalised']], 'finite': finite}
            print('%-22s plain %.4f ms/iter  penalised %.4f ms/iter  ratio %.4f  (plain run-to-run spread %.2f%%, '
                  'median of %d)  finite=%s' % (name, plain, penal, penal / plain, 100 * spread, a.runs, finite))
        del Y, D0
        torch.cuda.empty_cache()
    print(json.dumps({'steps': a.steps, 'runs': a.runs, 'l1': a.l1, 'l2': a.l2, 'cases': result}))


if __name__ == '__main__':
    main()
