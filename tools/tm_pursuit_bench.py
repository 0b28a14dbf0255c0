#!/usr/bin/env python3
"""Convolutional matching pursuit (dcp_tm_pursuit_*) at the documented template shape, against the coder a
template_matching user had before it (dcp_tm_lasso_*, acc_ista, lasso_iter = 10), at
    float32 and complex64    N = 2048, T = 8, S = 64, stride 1, 'SAME'    B = 16 and B = 1024
with n_nonzero_coefs = 1, 16 and 128.  The time of a greedy step is the difference of the 128- and the 16-step
calls over 112; "prepare" is the 16-step call less 16 such steps (row norms, lag correlations, y A^H, start-up of the
greedy kernel).  Event-timed, median of --runs runs after one warm-up run, one process.  y holds 160 planted events
per signal plus noise, so no signal stops before 128 steps.  Prints one line per figure and a JSON summary line.
    python tools/tm_pursuit_bench.py [--runs 5] [--small]"""
import argparse
import ctypes
import json
import os
import statistics
import sys

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))

import torch  # noqa: E402
from decomp_amd import _arrays, _hip, lasso, template_matching as tm  # noqa: E402


def timed(fn, runs):
    samples = []
    for r in range(runs + 1):       # run 0: warm-up
        torch.cuda.synchronize()
        e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        e0.record()
        fn()
        e1.record()
        torch.cuda.synchronize()
        if r > 0:
            samples.append(e0.elapsed_time(e1))
    return statistics.median(samples), samples


def problem(B, N, T, S, cplx, gen, events=160):
    def randn(*s):
        r = torch.randn(s, generator=gen, device='cuda')
        return torch.complex(r, torch.randn(s, generator=gen, device='cuda')) if cplx else r
    D = randn(T, S)
    _arrays.l2_normalize_(D, strict=True)
    C = tm._coef_size(S, N, 1, 'SAME')
    x0 = torch.zeros((B, T * C), device='cuda', dtype=D.dtype)
    cols = torch.randint(0, T * C, (B, events), generator=gen, device='cuda')
    x0.scatter_(1, cols, (1.0 + torch.rand((B, events), generator=gen, device='cuda')).to(D.dtype))
    Y = tm.predict(x0.reshape(B, T, C), D, N, 1, 'SAME')      # (set-up only: the timed calls are the library's)
    Y += 0.05 * Y.abs().mean() * randn(B, N)
    return Y.contiguous(), D.contiguous(), C


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument('--runs', type=int, default=5)
    ap.add_argument('--small', action='store_true', help='B / 8 (a quick look)')
    a = ap.parse_args()
    lib, h = _arrays.lib_handle(torch.empty(1, device='cuda'))
    gen = torch.Generator(device='cuda')
    gen.manual_seed(1)
    out = {}
    N, T, S = 2048, 8, 64
    for sfx, cplx in (('f32', False), ('c64', True)):
        for B in (16, 1024):
            if a.small:
                B = max(B // 8, 1)
            Y, D, C = problem(B, N, T, S, cplx, gen)
            X = torch.empty((B, T, C), device='cuda', dtype=Y.dtype)
            it = ctypes.c_int(0)
            tag = '%s_B%d' % (sfx, B)
            ms = {}
            for n in (1, 16, 128):
                def pursuit():
                    _hip.check(h, getattr(lib, 'dcp_tm_pursuit_' + sfx)(h, _arrays.ptr(Y), _arrays.ptr(D),
                                                                        _arrays.ptr(X), B, T, S, N, 1, 1, n, -1.0, 0,
                                                                        ctypes.byref(it)), 'dcp_tm_pursuit')
                ms[n], sm = timed(pursuit, a.runs)
                out['%s/n%d/pursuit_ms' % (tag, n)] = round(ms[n], 4)
                print('%-12s n = %3d  pursuit %9.4f ms (spread %.1f %%)   steps %d'
                      % (tag, n, ms[n], 100 * (max(sm) - min(sm)) / ms[n], it.value))
            step_us = 1000.0 * (ms[128] - ms[16]) / 112.0
            prepare = ms[16] - 16 * step_us / 1000.0
            out[tag + '/step_us'] = round(step_us, 3)
            out[tag + '/prepare_ms'] = round(prepare, 4)

            def ista():
                X.zero_()
                _hip.check(h, getattr(lib, 'dcp_tm_lasso_' + sfx)(h, _arrays.ptr(Y), _arrays.ptr(D), _arrays.ptr(X), B,
                                                                  T, S, N, 1, 1, 0.02, 1e-5, 10,
                                                                  lasso._METHOD_CODE['acc_ista'], 0, ctypes.byref(it)),
                           'dcp_tm_lasso')
            ms_l, _ = timed(ista, a.runs)
            out[tag + '/lasso_acc_ista10_ms'] = round(ms_l, 4)
            print('%-12s greedy step %8.3f us   prepare %8.4f ms   acc_ista x 10 %9.4f ms   pursuit(16) / acc_ista %.3f'
                  % (tag, step_us, prepare, ms_l, ms[16] / ms_l))
            del Y, D, X
            torch.cuda.empty_cache()
    print(json.dumps({'runs': a.runs, 'small': a.small, 'figures': out}))


if __name__ == '__main__':
    main()
