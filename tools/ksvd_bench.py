#!/usr/bin/env python3
"""Approximate K-SVD (dcp_ksvd_step_*, dcp_ksvd_sweep_*): milliseconds per iteration, split into coder, residual and
atom sweep, at
    float32    65536 x 4096, K = 512, s = 16     (the float32 dictionary-step shape of BASELINE)
    float32    65536 x 4096, K = 256, s = 8
Event-timed around the library calls (their host synchronisations included), median of --runs runs after one warm-up
run, one process.  y = x0 A + noise with 16 atoms per row, so no row stops before s steps.
    whole step        dcp_ksvd_step_*
    coder             dcp_omp_* on the same operands
    residual + lists  dcp_ksvd_sweep_* on X = 0: the list build, the copy of D, R = Y - X D, max|dD|; no atom runs
    atoms             dcp_ksvd_sweep_* on the coder's X, minus the line above; with bytes / s from the model
                      3 sum_k |I_k| F sizeof(T) (two reads and one write of every support row of R) against the
                      6.29 TB/s copy rate
    atoms, F = 64     the same supports on the first 64 channels: what is left of the sweep when the bytes are taken
                      away (launches and the latency of 3 K dependent kernels), as a share of the sweep
Prints one line per figure and a JSON summary line.
    python tools/ksvd_bench.py [--runs 5] [--small]"""
import argparse
import ctypes
import json
import os
import statistics
import sys

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))

import torch  # noqa: E402
from decomp_amd import _arrays, _hip  # noqa: E402
from omp_bench import problem  # noqa: E402

COPY_RATE = 6.29e12     # bytes / s, the measured device copy rate


def timed(prepare, fn, runs):
    samples = []
    for r in range(runs + 1):       # run 0: warm-up
        prepare()
        torch.cuda.synchronize()
        e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        e0.record()
        fn()
        e1.record()
        torch.cuda.synchronize()
        if r > 0:
            samples.append(e0.elapsed_time(e1))
    return statistics.median(samples)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument('--runs', type=int, default=5)
    ap.add_argument('--small', action='store_true', help='N / 8 (a quick look)')
    a = ap.parse_args()
    lib, h = _arrays.lib_handle(torch.empty(1, device='cuda'))
    gen = torch.Generator(device='cuda')
    gen.manual_seed(1)
    out = {}
    for N, F, K, s in [(65536, 4096, 512, 16), (65536, 4096, 256, 8)]:
        if a.small:
            N //= 8
        Y, D0 = problem(N, F, K, False, gen)
        X0 = torch.empty((N, K), device='cuda', dtype=Y.dtype)
        it, md = ctypes.c_int(0), ctypes.c_double(0)
        tag = 'f32_%dx%dk%ds%d' % (N, F, K, s)

        def omp(Yc, Dc, Xc):
            n, f = Yc.shape
            _hip.check(h, lib.dcp_omp_f32(h, _arrays.ptr(Yc), _arrays.ptr(Dc), _arrays.ptr(Xc), n, f, K, s, -1.0,
                                          ctypes.byref(it)), 'dcp_omp')

        def sweep(Yc, Dc, Xc):
            n, f = Yc.shape
            _hip.check(h, lib.dcp_ksvd_sweep_f32(h, _arrays.ptr(Yc), _arrays.ptr(Xc), _arrays.ptr(Dc), n, f, K, s,
                                                 ctypes.byref(md)), 'dcp_ksvd_sweep')

        def step(Yc, Dc, Xc):
            n, f = Yc.shape
            _hip.check(h, lib.dcp_ksvd_step_f32(h, _arrays.ptr(Yc), _arrays.ptr(Xc), _arrays.ptr(Dc), n, f, K, s, -1.0,
                                                ctypes.byref(md), ctypes.byref(it)), 'dcp_ksvd_step')
        omp(Y, D0, X0)
        nnz = int(torch.count_nonzero(X0))
        counts = torch.count_nonzero(X0, dim=0)
        D, X = D0.clone(), X0.clone()

        def restore():
            D.copy_(D0)
            X.copy_(X0)

        ms_step = timed(restore, lambda: step(Y, D, X), a.runs)
        ms_omp = timed(restore, lambda: omp(Y, D, X), a.runs)
        ms_fixed = timed(lambda: (D.copy_(D0), X.zero_()), lambda: sweep(Y, D, X), a.runs)
        ms_sweep = timed(restore, lambda: sweep(Y, D, X), a.runs)
        ms_atoms = ms_sweep - ms_fixed
        model_bytes = 3.0 * nnz * F * Y.element_size()
        rate = model_bytes / (ms_atoms * 1e-3)
        # the same supports on 64 channels
        Y64, D64_0 = Y[:, :64].contiguous(), D0[:, :64].contiguous()
        D64 = D64_0.clone()
        ms_fixed64 = timed(lambda: (D64.copy_(D64_0), X.zero_()), lambda: sweep(Y64, D64, X), a.runs)
        ms_sweep64 = timed(lambda: (D64.copy_(D64_0), X.copy_(X0)), lambda: sweep(Y64, D64, X), a.runs)
        ms_atoms64 = ms_sweep64 - ms_fixed64
        out[tag] = {'step_ms': round(ms_step, 4), 'coder_ms': round(ms_omp, 4),
                    'residual_and_lists_ms': round(ms_fixed, 4), 'atoms_ms': round(ms_atoms, 4),
                    'atoms_model_TBps': round(rate / 1e12, 4), 'atoms_share_of_copy_rate': round(rate / COPY_RATE, 4),
                    'atoms_F64_ms': round(ms_atoms64, 4), 'fixed_share_of_atoms': round(ms_atoms64 / ms_atoms, 4),
                    'nnz': nnz, 'support_min': int(counts.min()), 'support_max': int(counts.max())}
        print('%-26s step %9.3f ms = coder %9.3f + residual and lists %8.3f + atoms %9.3f (sum %9.3f)'
              % (tag, ms_step, ms_omp, ms_fixed, ms_atoms, ms_omp + ms_fixed + ms_atoms))
        print('%-26s atoms: %d support rows (per atom %d .. %d), model %.3f GB -> %.3f TB/s = %.1f %% of the copy '
              'rate; on 64 channels %.3f ms = %.1f %% of the sweep is launches and kernel latency'
              % (tag, nnz, int(counts.min()), int(counts.max()), model_bytes / 1e9, rate / 1e12,
                 100 * rate / COPY_RATE, ms_atoms64, 100 * ms_atoms64 / ms_atoms))
        del Y, D0, X0, D, X, Y64, D64_0, D64
        torch.cuda.empty_cache()
    print(json.dumps({'runs': a.runs, 'small': a.small, 'figures': out}))


if __name__ == '__main__':
    main()
