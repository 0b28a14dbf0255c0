#!/usr/bin/env python3
"""em-hals (method='em-hals', dcp_nmf_emhals_*) against the masked multiplicative update (dcp_nmf_mu_* with a
mask, l2) on one planted non-negative problem with missing entries, default float32 65536 x 4096, k = 256, a
binary mask with 30 % of the entries missing, both started from x = ones and the same D:

  * ms per iteration of em-hals with the mask, of unmasked HALS (dcp_nmf_hals_*, the iteration em-hals adds the
    imputing product to) and of masked MU: a warm-up, then --steps iterations between two events, --runs runs
    with the three variants alternating run by run, the median of each;
  * the masked relative residual |(Y - xD) o M| / |Y o M| after every iteration (the loops' resid_trace, a
    separate run), the iterations em-hals needs to reach what masked MU reaches after --iters iterations, the
    wall time that takes at the measured ms per iteration, and the relative error on the hidden entries.

Prints one line per measurement and a JSON summary line.
    python tools/nmf_emhals_vs_mu.py [--rows 65536] [--f 4096] [--k 256] [--missing 0.3] [--steps 20] [--runs 5]
                                     [--iters 200]"""
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
    ap.add_argument('--missing', type=float, default=0.3)
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

    def half_sparse(shape):
        return (torch.rand(shape, generator=g, device='cuda', dtype=dt) *
                (torch.rand(shape, generator=g, device='cuda') < 0.5))

    x0 = half_sparse((N, K))
    D0 = half_sparse((K, F))
    Y = x0 @ D0 + 0.01 * torch.rand((N, F), generator=g, device='cuda', dtype=dt)
    del x0, D0
    Dstart = torch.rand((K, F), generator=g, device='cuda', dtype=dt) + 0.1
    _arrays.l2_normalize_(Dstart, strict=True)
    M = (torch.rand((N, F), generator=g, device='cuda') >= a.missing).to(dt)
    ymnorm = float(torch.linalg.vector_norm((Y * M).double()))
    lib, h = _arrays.lib_handle(Y)
    it = ctypes.c_int(0)

    def call(method, x, D, n, trace=None):
        if method == 'em-hals':
            rc = getattr(lib, 'dcp_nmf_emhals_' + sfx)(h, _arrays.ptr(Y), _arrays.ptr(M), _arrays.ptr(x),
                                                        _arrays.ptr(D), N, F, K, ctype(0.0), n + 1, ctypes.byref(it),
                                                        None, trace)
        elif method == 'hals':
            rc = getattr(lib, 'dcp_nmf_hals_' + sfx)(h, _arrays.ptr(Y), _arrays.ptr(x), _arrays.ptr(D), N, F, K,
                                                      ctype(0.0), n + 1, ctypes.byref(it), None, trace)
        else:
            rc = getattr(lib, 'dcp_nmf_mu_' + sfx)(h, _arrays.ptr(Y), _arrays.ptr(M), _arrays.ptr(x), _arrays.ptr(D),
                                                    N, F, K, _hip.LIK_L2, ctype(0.0), n + 1, ctypes.byref(it), None,
                                                    trace)
        _hip.check(h, rc, method)

    methods = ('em-hals', 'hals', 'masked-mu')
    state, samples = {}, {m: [] for m in methods}
    for m in methods:
        state[m] = (torch.ones((N, K), device='cuda', dtype=dt), Dstart.clone())
        call(m, state[m][0], state[m][1], 3)   # warm-up (workspace, code objects)
    for _ in range(a.runs):                    # the variants alternate run by run
        for m in methods:
            x, D = state[m]
            torch.cuda.synchronize()
            e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
            e0.record()
            call(m, x, D, a.steps)
            e1.record()
            torch.cuda.synchronize()
            samples[m].append(e0.elapsed_time(e1) / a.steps)
    del state
    timing = {}
    for m in methods:
        ms = statistics.median(samples[m])
        timing[m] = {'ms_per_iter': round(ms, 4), 'samples': [round(s, 4) for s in samples[m]],
                     'spread_pct': round(100.0 * (max(samples[m]) - min(samples[m])) / ms, 2)}
        print('%-9s %dx%d k=%d %s: %.4f ms/iter (median of %d, spread %.1f %%)'
              % (m, N, F, K, a.dtype, ms, a.runs, timing[m]['spread_pct']))

    conv = {}
    hidden = 1.0 - M
    yhnorm = float(torch.linalg.vector_norm((Y * hidden).double()))
    for m in ('masked-mu', 'em-hals'):
        x = torch.ones((N, K), device='cuda', dtype=dt)
        D = Dstart.clone()
        trace = (ctype * (a.iters + 1))()
        call(m, x, D, a.iters, trace)
        rel = [float(trace[i]) / ymnorm for i in range(a.iters)]
        hid = float(torch.linalg.vector_norm(((Y - x @ D) * hidden).double())) / max(yhnorm, 1e-300)
        conv[m] = {'rel_resid': rel, 'hidden_rel_err': hid}
        print('%-9s masked rel. residual after 1/10/%d iterations: %.3e %.3e %.3e; hidden-entry rel. error %.3e'
              % (m, a.iters, rel[0], rel[min(9, a.iters - 1)], rel[-1], hid))
    target = conv['masked-mu']['rel_resid'][-1]
    summary = {}
    for m in ('masked-mu', 'em-hals'):
        n = next((i + 1 for i, v in enumerate(conv[m]['rel_resid']) if v <= target), None)
        ms = timing[m]['ms_per_iter']
        summary[m] = {'ms_per_iter': ms, 'iters_to_target': n, 'ms_to_target': None if n is None else round(n * ms, 2),
                      'final_rel_resid': conv[m]['rel_resid'][-1], 'hidden_rel_err': conv[m]['hidden_rel_err']}
        print('%-9s reaches masked rel. residual %.4e after %s iterations = %s ms'
              % (m, target, n, 'n/a' if n is None else '%.1f' % (n * ms)))
    r_mu = round(timing['em-hals']['ms_per_iter'] / timing['masked-mu']['ms_per_iter'], 3)
    r_hals = round(timing['em-hals']['ms_per_iter'] / timing['hals']['ms_per_iter'], 3)
    print('em-hals / masked mu time per iteration: %.3f; em-hals / unmasked hals: %.3f' % (r_mu, r_hals))
    print(json.dumps({'shape': [N, F, K], 'dtype': a.dtype, 'missing': a.missing, 'steps': a.steps, 'runs': a.runs,
                      'iters': a.iters, 'target_rel_resid': target, 'summary': summary,
                      'emhals_over_masked_mu_per_iter': r_mu, 'emhals_over_hals_per_iter': r_hals,
                      'timing': timing}))


if __name__ == '__main__':
    main()
