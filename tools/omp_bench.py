#!/usr/bin/env python3
"""Orthogonal matching pursuit (dcp_omp_*): the whole solve, the greedy kernel alone (dcp_omp_gram_*), the y.A^H
product it follows (dcp_gemm_*, form NT) and the dictionary step with 'omp' against the one with ista x 10, at
    float32    N = 8192 and 65536, F = 4096, K = 512, s = 8, 16, 32   (the dictionary steps at s = 16)
    complex64  8192 x 8192, K = 512, s = 16
Event-timed, median of --runs runs after one warm-up run, one process.  y = x0 A + noise with 16 atoms per row, so
no row stops before s steps.  Prints one line per figure and a JSON summary line.
    python tools/omp_bench.py [--runs 5] [--small]"""
import argparse
import ctypes
import json
import os
import statistics
import sys

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))

import torch  # noqa: E402
from decomp_amd import _arrays, _hip  # noqa: E402


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


def problem(N, F, K, cplx, gen):
    def randn(*s):
        r = torch.randn(s, generator=gen, device='cuda')
        return torch.complex(r, torch.randn(s, generator=gen, device='cuda')) if cplx else r
    A = randn(K, F)
    _arrays.l2_normalize_(A, strict=True)
    x0 = torch.zeros((N, K), device='cuda', dtype=A.dtype)
    cols = torch.randint(0, K, (N, 16), generator=gen, device='cuda')
    x0.scatter_(1, cols, (1.0 + torch.rand((N, 16), generator=gen, device='cuda')).to(A.dtype))
    Y = x0 @ A                      # (set-up only: the timed calls are the library's)
    Y += 0.05 * Y.abs().mean() * randn(N, F)
    return Y.contiguous(), A


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument('--runs', type=int, default=5)
    ap.add_argument('--small', action='store_true', help='N / 8 (a quick look)')
    a = ap.parse_args()
    lib, h = _arrays.lib_handle(torch.empty(1, device='cuda'))
    gen = torch.Generator(device='cuda')
    gen.manual_seed(1)
    out = {}
    shapes = [('f32', False, 8192, 4096, 512, (8, 16, 32)), ('f32', False, 65536, 4096, 512, (8, 16, 32)),
              ('c64', True, 8192, 8192, 512, (16,))]
    for sfx, cplx, N, F, K, sparsities in shapes:
        if a.small:
            N //= 8
        Y, A = problem(N, F, K, cplx, gen)
        X = torch.empty((N, K), device='cuda', dtype=Y.dtype)
        alpha0 = torch.empty((N, K), device='cuda', dtype=Y.dtype)
        G = torch.empty((K, K), device='cuda', dtype=Y.dtype)
        it = ctypes.c_int(0)
        gemm = getattr(lib, 'dcp_gemm_' + sfx)
        tag = '%s_%dx%dk%d' % (sfx, N, F, K)

        def product():
            _hip.check(h, gemm(h, 0, _arrays.ptr(Y), _arrays.ptr(A), _arrays.ptr(alpha0), N, K, F, 1, 0), 'gemm')
        ms, _ = timed(product, a.runs)
        out[tag + '/product_yAh_ms'] = round(ms, 4)
        print('%-28s y.A^H product            %9.4f ms' % (tag, ms))
        _hip.check(h, gemm(h, 0, _arrays.ptr(A), _arrays.ptr(A), _arrays.ptr(G), K, K, F, 1, 0), 'gemm')
        for s in sparsities:
            def whole():
                _hip.check(h, getattr(lib, 'dcp_omp_' + sfx)(h, _arrays.ptr(Y), _arrays.ptr(A), _arrays.ptr(X), N, F,
                                                             K, s, -1.0, ctypes.byref(it)), 'dcp_omp')

            def greedy():
                _hip.check(h, getattr(lib, 'dcp_omp_gram_' + sfx)(h, _arrays.ptr(alpha0), _arrays.ptr(G), None,
                                                                  _arrays.ptr(X), N, K, s, -1.0, ctypes.byref(it)),
                           'dcp_omp_gram')
            ms_w, _ = timed(whole, a.runs)
            ms_g, sm = timed(greedy, a.runs)
            out['%s/s%d/omp_ms' % (tag, s)] = round(ms_w, 4)
            out['%s/s%d/greedy_ms' % (tag, s)] = round(ms_g, 4)
            print('%-28s s = %2d  whole solve %9.4f ms   greedy kernel %9.4f ms (spread %.1f %%)   steps %d'
                  % (tag, s, ms_w, ms_g, 100 * (max(sm) - min(sm)) / ms_g, it.value))
        # the dictionary step on these rows as one minibatch: ista x 10 against omp, s = 16
        D = A.clone()
        Dn = torch.empty_like(D)
        md, lit = ctypes.c_double(0), ctypes.c_int(0)
        step = getattr(lib, 'dcp_dict_step_' + sfx)

        def dict_step(code, iters, alpha):
            x = torch.ones((N, K), device='cuda', dtype=Y.dtype)
            SA = torch.zeros((K, K), device='cuda', dtype=Y.dtype)
            SB = torch.zeros((K, F), device='cuda', dtype=Y.dtype)

            def run():
                _hip.check(h, step(h, _arrays.ptr(Y), _arrays.ptr(x), _arrays.ptr(D), _arrays.ptr(Dn), _arrays.ptr(SA),
                                   _arrays.ptr(SB), N, F, K, 0.0, alpha, code, iters, -1.0 if code == _hip.LASSO_OMP
                                   else 1e-5, ctypes.byref(md), ctypes.byref(lit)), 'dcp_dict_step')
            return timed(run, a.runs)[0]
        ms_i = dict_step(_hip.LASSO_ISTA, 10, 0.02)
        ms_o = dict_step(_hip.LASSO_OMP, 16, 0.0)
        out[tag + '/dict_step_ista10_ms'] = round(ms_i, 4)
        out[tag + '/dict_step_omp16_ms'] = round(ms_o, 4)
        out[tag + '/dict_step_ratio'] = round(ms_o / ms_i, 4)
        print('%-28s dictionary step: ista x 10 %9.4f ms   omp (s = 16) %9.4f ms   ratio %.3f'
              % (tag, ms_i, ms_o, ms_o / ms_i))
        del Y, A, X, alpha0, G, D, Dn
        torch.cuda.empty_cache()
    print(json.dumps({'runs': a.runs, 'small': a.small, 'figures': out}))


if __name__ == '__main__':
    main()
