#!/usr/bin/env python3
"""Masked approximate K-SVD (dcp_ksvd_mask_step_*, dcp_ksvd_mask_sweep_*): milliseconds per iteration, split into
coder, residual and atom sweep, at
    float32    65536 x 4096, K = 512, s = 16
    float32    65536 x 4096, K = 256, s = 8
    complex64   8192 x 8192, K = 512, s = 16
with 30 % of the entries missing (a 0 / 1 mask row of its own for every data row).  Event-timed around the library
calls (their host synchronisations included), median of --runs runs after one warm-up run, one process.
y = x0 A + noise with 16 atoms per row, so no row stops before s steps.
    whole step        dcp_ksvd_mask_step_*
    coder             dcp_omp_mask_* on the same operands
    residual + lists  dcp_ksvd_mask_sweep_* on X = 0: the list build, the copy of D, R = Y - X D, max|dD|; no atom runs
    atoms             dcp_ksvd_mask_sweep_* on the coder's X, minus the line above; with bytes / s from the model
                      sum_k |I_k| F (3 sizeof(T) + 2 sizeof(real)) (two reads and one write of every support row of
                      R, two reads of the same rows of M) against the 6.29 TB/s copy rate
    all-ones mask     the same supports, M = 1: the masked atoms against the unmasked atoms of dcp_ksvd_sweep_* (timed
                      here, the way tools/ksvd_bench.py times them), in the same session
Prints one line per figure and a JSON summary line.
    python tools/ksvd_mask_bench.py [--runs 5] [--small]"""
import argparse
import ctypes
import json
import os
import sys

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))

import torch  # noqa: E402
from decomp_amd import _arrays, _hip  # noqa: E402
from ksvd_bench import COPY_RATE, timed  # noqa: E402
from omp_bench import problem  # noqa: E402


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument('--runs', type=int, default=5)
    ap.add_argument('--small', action='store_true', help='N / 8 (a quick look)')
    a = ap.parse_args()
    lib, h = _arrays.lib_handle(torch.empty(1, device='cuda'))
    gen = torch.Generator(device='cuda')
    gen.manual_seed(1)
    out = {}
    for sfx, cplx, N, F, K, s in [('f32', False, 65536, 4096, 512, 16), ('f32', False, 65536, 4096, 256, 8),
                                  ('c64', True, 8192, 8192, 512, 16)]:
        if a.small:
            N //= 8
        Y, D0 = problem(N, F, K, cplx, gen)
        M = (torch.rand((N, F), generator=gen, device='cuda') < 0.7).to(torch.float32)
        ones = torch.ones_like(M)
        X0 = torch.empty((N, K), device='cuda', dtype=Y.dtype)
        it, md = ctypes.c_int(0), ctypes.c_double(0)
        tag = '%s_%dx%dk%ds%d' % (sfx, N, F, K, s)

        def omp(Dc, Xc):
            _hip.check(h, getattr(lib, 'dcp_omp_mask_' + sfx)(h, _arrays.ptr(Y), _arrays.ptr(M), 2, _arrays.ptr(Dc),
                                                              _arrays.ptr(Xc), N, F, K, s, -1.0, 0, ctypes.byref(it)),
                       'dcp_omp_mask')

        def sweep(Dc, Xc, mask=M):
            _hip.check(h, getattr(lib, 'dcp_ksvd_mask_sweep_' + sfx)(h, _arrays.ptr(Y), _arrays.ptr(mask), 2,
                                                                     _arrays.ptr(Xc), _arrays.ptr(Dc), N, F, K, s,
                                                                     ctypes.byref(md)), 'dcp_ksvd_mask_sweep')

        def unmasked_sweep(Dc, Xc):
            _hip.check(h, getattr(lib, 'dcp_ksvd_sweep_' + sfx)(h, _arrays.ptr(Y), _arrays.ptr(Xc), _arrays.ptr(Dc), N,
                                                                F, K, s, ctypes.byref(md)), 'dcp_ksvd_sweep')

        def step(Dc, Xc):
            _hip.check(h, getattr(lib, 'dcp_ksvd_mask_step_' + sfx)(h, _arrays.ptr(Y), _arrays.ptr(M), 2,
                                                                    _arrays.ptr(Xc), _arrays.ptr(Dc), N, F, K, s, -1.0,
                                                                    0, ctypes.byref(md), ctypes.byref(it)),
                       'dcp_ksvd_mask_step')
        omp(D0, X0)
        nnz = int(torch.count_nonzero(X0))
        counts = torch.count_nonzero(X0, dim=0)
        D, X = D0.clone(), X0.clone()

        def restore():
            D.copy_(D0)
            X.copy_(X0)

        def zero():
            D.copy_(D0)
            X.zero_()

        ms_step = timed(restore, lambda: step(D, X), a.runs)
        ms_omp = timed(restore, lambda: omp(D, X), a.runs)
        ms_fixed = timed(zero, lambda: sweep(D, X), a.runs)
        ms_atoms = timed(restore, lambda: sweep(D, X), a.runs) - ms_fixed
        ms_atoms_ones = timed(restore, lambda: sweep(D, X, ones), a.runs) - ms_fixed
        ms_fixed_u = timed(zero, lambda: unmasked_sweep(D, X), a.runs)
        ms_atoms_u = timed(restore, lambda: unmasked_sweep(D, X), a.runs) - ms_fixed_u
        esz, rsz = Y.element_size(), M.element_size()
        model_bytes = float(nnz) * F * (3 * esz + 2 * rsz)
        model_bytes_u = 3.0 * nnz * F * esz
        rate, rate_u = model_bytes / (ms_atoms * 1e-3), model_bytes_u / (ms_atoms_u * 1e-3)
        out[tag] = {'step_ms': round(ms_step, 4), 'coder_ms': round(ms_omp, 4),
                    'residual_and_lists_ms': round(ms_fixed, 4), 'atoms_ms': round(ms_atoms, 4),
                    'atoms_model_TBps': round(rate / 1e12, 4), 'atoms_share_of_copy_rate': round(rate / COPY_RATE, 4),
                    'atoms_ones_mask_ms': round(ms_atoms_ones, 4), 'unmasked_atoms_ms': round(ms_atoms_u, 4),
                    'unmasked_atoms_model_TBps': round(rate_u / 1e12, 4),
                    'ones_mask_to_unmasked': round(ms_atoms_ones / ms_atoms_u, 4),
                    'byte_model_ratio': round(model_bytes / model_bytes_u, 4),
                    'nnz': nnz, 'support_min': int(counts.min()), 'support_max': int(counts.max())}
        print('%-26s step %9.3f ms = coder %9.3f + residual and lists %8.3f + atoms %9.3f (sum %9.3f)'
              % (tag, ms_step, ms_omp, ms_fixed, ms_atoms, ms_omp + ms_fixed + ms_atoms))
        print('%-26s atoms: %d support rows (per atom %d .. %d), model %.3f GB -> %.3f TB/s = %.1f %% of the copy rate'
              % (tag, nnz, int(counts.min()), int(counts.max()), model_bytes / 1e9, rate / 1e12,
                 100 * rate / COPY_RATE))
        print('%-26s all-ones mask: masked atoms %9.3f ms, unmasked atoms %9.3f ms (%.3f TB/s): ratio %.2f, byte '
              'model %.2f' % (tag, ms_atoms_ones, ms_atoms_u, rate_u / 1e12, ms_atoms_ones / ms_atoms_u,
                              model_bytes / model_bytes_u))
        del Y, D0, X0, D, X, M, ones
        torch.cuda.empty_cache()
    print(json.dumps({'runs': a.runs, 'small': a.small, 'figures': out}))


if __name__ == '__main__':
    main()
