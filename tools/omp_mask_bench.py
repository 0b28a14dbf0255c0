#!/usr/bin/env python3
"""Masked orthogonal matching pursuit (dcp_omp_mask_*, a mask row of its own for every data row) at
    float32    65536 x 4096, K = 512, s = 16
    complex64  8192 x 8192,  K = 512, s = 16
with 30 % of the entries missing.  For each: the whole solve; the share of it spent in the s products
alpha = (m o r) A^H and the share spent in the step kernel (the library's own event pairs, dcp_profile_*, in a
separate profiled run of the same call); the ratio of the step kernel to its step's product; the unmasked dcp_omp_*
on the same arrays; and the masked solve with an all-ones mask against the unmasked one.
Event-timed, median of --runs runs after one warm-up run, one process.  y = x0 A + noise with 16 atoms per row, so
no row stops before s steps.  Prints one line per figure and a JSON summary line.
    python tools/omp_mask_bench.py [--runs 5] [--small] [--sparsity 16]"""
import argparse
import ctypes
import json
import os
import sys

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))

import torch  # noqa: E402
from decomp_amd import _arrays, _hip  # noqa: E402
from omp_bench import problem, timed  # noqa: E402

PROF_PRODUCTS, PROF_STEP, PROF_REST = 0, 2, 8      # DCP_PROF_GRAM, DCP_PROF_XUPDATE, DCP_PROF_MISC


def profiled(lib, h, fn):
    """One run of fn with the library's event pairs on: ms under each of the three labels."""
    _hip.check(h, lib.dcp_profile_enable(h, 1), 'dcp_profile_enable')
    _hip.check(h, lib.dcp_profile_reset(h), 'dcp_profile_reset')
    fn()
    out = {}
    for label in (PROF_PRODUCTS, PROF_STEP, PROF_REST):
        ms, cnt = ctypes.c_double(0), ctypes.c_int64(0)
        _hip.check(h, lib.dcp_profile_read(h, label, ctypes.byref(ms), ctypes.byref(cnt)), 'dcp_profile_read')
        out[label] = ms.value
    _hip.check(h, lib.dcp_profile_enable(h, 0), 'dcp_profile_enable')
    return out


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument('--runs', type=int, default=5)
    ap.add_argument('--small', action='store_true', help='N / 8 (a quick look)')
    ap.add_argument('--sparsity', type=int, default=16, help='s (how the step kernel grows with it: 4, 32)')
    a = ap.parse_args()
    lib, h = _arrays.lib_handle(torch.empty(1, device='cuda'))
    gen = torch.Generator(device='cuda')
    gen.manual_seed(1)
    out = {}
    s = a.sparsity
    for sfx, cplx, N, F, K in [('f32', False, 65536, 4096, 512), ('c64', True, 8192, 8192, 512)]:
        if a.small:
            N //= 8
        Y, A = problem(N, F, K, cplx, gen)
        M = (torch.rand((N, F), generator=gen, device='cuda') < 0.7).to(torch.float32)
        X = torch.empty((N, K), device='cuda', dtype=Y.dtype)
        it = ctypes.c_int(0)
        tag = '%s_%dx%dk%d_s%d' % (sfx, N, F, K, s)

        def masked(mask=M):
            _hip.check(h, getattr(lib, 'dcp_omp_mask_' + sfx)(h, _arrays.ptr(Y), _arrays.ptr(mask), 2, _arrays.ptr(A),
                                                              _arrays.ptr(X), N, F, K, s, -1.0, 0, ctypes.byref(it)),
                       'dcp_omp_mask')

        def unmasked():
            _hip.check(h, getattr(lib, 'dcp_omp_' + sfx)(h, _arrays.ptr(Y), _arrays.ptr(A), _arrays.ptr(X), N, F, K, s,
                                                         -1.0, ctypes.byref(it)), 'dcp_omp')
        ms_m, sm = timed(masked, a.runs)
        steps = it.value
        prof = profiled(lib, h, masked)
        total = sum(prof.values())
        ms_u, _ = timed(unmasked, a.runs)
        M.fill_(1.0)
        ms_1, _ = timed(masked, a.runs)
        fig = {'masked_ms': ms_m, 'products_share': prof[PROF_PRODUCTS] / total, 'step_kernel_share': prof[PROF_STEP] / total,
               'products_ms_profiled': prof[PROF_PRODUCTS], 'step_kernel_ms_profiled': prof[PROF_STEP],
               'rest_ms_profiled': prof[PROF_REST], 'step_to_product': prof[PROF_STEP] / prof[PROF_PRODUCTS],
               'unmasked_ms': ms_u, 'ones_mask_ms': ms_1, 'ones_mask_to_unmasked': ms_1 / ms_u}
        for k, v in fig.items():
            out[tag + '/' + k] = round(v, 4)
        print('%-26s masked solve %9.3f ms (spread %.1f %%, steps %d)   products %.1f %%   step kernel %.1f %%   '
              'step kernel / product %.2f' % (tag, ms_m, 100 * (max(sm) - min(sm)) / ms_m, steps,
                                              100 * fig['products_share'], 100 * fig['step_kernel_share'],
                                              fig['step_to_product']))
        print('%-26s unmasked dcp_omp %9.3f ms   all-ones mask %9.3f ms   ratio %.2f'
              % (tag, ms_u, ms_1, ms_1 / ms_u))
        del Y, A, X, M
        torch.cuda.empty_cache()
    print(json.dumps({'runs': a.runs, 'small': a.small, 'sparsity': s, 'figures': out}))


if __name__ == '__main__':
    main()
