#!/usr/bin/env python3
"""One fused MU iteration of the beta-divergence likelihood (DCP_LIK_BETA) against KL, float32, at the
benchmark shape 16384 x 4096, k = 256 (one GPU's rows of BASELINE configs[3]).  Times dcp_nmf_mu_f32 per
iteration after a warm-up, median over --runs runs, every case in one process; prints one line per case
and a JSON summary line.    python tools/bench_nmf_beta.py [--rows 16384] [--steps 20] [--runs 5]"""
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
    ap.add_argument('--rows', type=int, default=16384)
    ap.add_argument('--f', type=int, default=4096)
    ap.add_argument('--k', type=int, default=256)
    ap.add_argument('--steps', type=int, default=20)
    ap.add_argument('--runs', type=int, default=5)
    a = ap.parse_args()
    N, F, K = a.rows, a.f, a.k
    g = torch.Generator(device='cuda')
    g.manual_seed(1)
    Dt = torch.rand((K, F), generator=g, device='cuda') * 0.9 + 0.1
    xt = torch.rand((N, K), generator=g, device='cuda') * 0.9 + 0.1
    Y = (xt @ Dt) * (torch.rand((N, F), generator=g, device='cuda') * 0.6 + 0.7)   # positive: IS is defined
    D0 = Dt * (torch.rand((K, F), generator=g, device='cuda') + 0.5)
    mask = (torch.rand((N, F), generator=g, device='cuda') >= 0.2).float()
    Ym = Y * mask
    del xt
    lib, h = _arrays.lib_handle(Y)
    cases = [('kl', _hip.LIK_KL, None, False), ('kl+mask', _hip.LIK_KL, None, True)]
    for beta in (0.0, 0.5, 1.5, 0.7):   # 0.7: the general exp2 / log2 epilogue (0, 0.5, 1.5 have closed forms)
        cases += [('beta=%g' % beta, _hip.LIK_BETA, beta, False), ('beta=%g+mask' % beta, _hip.LIK_BETA, beta, True)]
    result = {}
    for name, lik, beta, masked in cases:
        y, m = (Ym, mask) if masked else (Y, None)
        D = D0.clone()
        _arrays.l2_normalize_(D, strict=True)
        x = torch.ones((N, K), device='cuda')
        it = ctypes.c_int(0)

        def run(n):
            if lik == _hip.LIK_BETA:
                _hip.check(h, lib.dcp_set_nmf_beta(h, beta), 'dcp_set_nmf_beta')
            _hip.check(h, lib.dcp_nmf_mu_f32(h, _arrays.ptr(y), _arrays.ptr(m), _arrays.ptr(x),
                                             _arrays.ptr(D), N, F, K, lik, ctypes.c_float(0.0), n + 1,
                                             ctypes.byref(it), None, None), 'nmf')
        run(3)
        samples = []
        for _ in range(a.runs):
            torch.cuda.synchronize()
            e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
            e0.record()
            run(a.steps)
            e1.record()
            torch.cuda.synchronize()
            samples.append(e0.elapsed_time(e1) / a.steps)
        ms = statistics.median(samples)
        # algorithmic flops: KL 2 (+1 masked) 2NFK products per half step and the forward; beta 3 per half step
        nprod = 6 if lik == _hip.LIK_BETA else (6 if masked else 4)
        flops = nprod * 2.0 * N * F * K
        finite = bool(torch.isfinite(D).all()) and bool(torch.isfinite(x).all())
        result[name] = {'ms_per_iter': round(ms, 4), 'samples': [round(s, 4) for s in samples],
                        'tflops': round(flops / ms / 1e9, 1), 'finite': finite}
        print('%-14s %dx%d k=%d: %.3f ms/iter (median of %d)  %.1f TFLOP/s algorithmic  finite=%s'
              % (name, N, F, K, ms, a.runs, flops / ms / 1e9, finite))
    kl = result['kl']['ms_per_iter']
    is0 = result['beta=0']['ms_per_iter']
    ratios = {'beta0_over_kl': round(is0 / kl, 3),
              'beta0.5_over_beta0': round(result['beta=0.5']['ms_per_iter'] / is0, 3),
              'beta1.5_over_beta0': round(result['beta=1.5']['ms_per_iter'] / is0, 3),
              'beta0.7_over_beta0': round(result['beta=0.7']['ms_per_iter'] / is0, 3)}
    print(json.dumps({'shape': [N, F, K], 'steps': a.steps, 'runs': a.runs, 'cases': result, 'ratios': ratios}))


if __name__ == '__main__':
    main()
