#!/usr/bin/env python3
"""Orthogonal convolutional pursuit (dcp_tm_omp_*) at the documented template shape, against plain matching pursuit
(dcp_tm_pursuit_*) at the same number of steps and against the orthogonal coder a user had before it (omp.solve on the
dense operator of _temp2mat), at
    float32 and complex64    N = 2048, T = 8, S = 64, stride 1, 'SAME'    B = 16 and B = 1024
with n_nonzero_coefs = 1, 16 and the cap (64 real, 32 complex).  A step re-fits the whole cluster of overlapping events,
so its time grows with the support: the time per step is given over steps 2 .. 16, (t16 - t1) / 15, and over steps
17 .. cap, (tcap - t16) / (cap - 16); "prepare" is the one-step call (row norms, lag correlations, y A^H, start-up of
the greedy kernel and its first step).  Event-timed, median of --runs runs after one warm-up run, one process.  y
holds 160 planted events per signal plus noise -- every event overlaps others, one cluster -- so no signal stops before
the cap.  The dense coder is left out (null) where its
workspace -- the operator, its Gram matrix and the 64 split-K slabs of that -- exceeds --dense-gib or cannot be had.
Prints one line per figure and a JSON summary line.
    python tools/tm_omp_bench.py [--runs 5] [--small] [--dense-gib 80]"""
import argparse
import ctypes
import json
import os
import sys

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))

import torch  # noqa: E402
from decomp_amd import _arrays, _hip, omp, template_matching as tm  # noqa: E402
from tm_pursuit_bench import problem, timed  # noqa: E402


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument('--runs', type=int, default=5)
    ap.add_argument('--small', action='store_true', help='B / 8 (a quick look)')
    ap.add_argument('--dense-gib', type=float, default=80.0,
                    help='run omp.solve on the dense operator where its workspace stays below this (0: never)')
    a = ap.parse_args()
    lib, h = _arrays.lib_handle(torch.empty(1, device='cuda'))
    gen = torch.Generator(device='cuda')
    gen.manual_seed(1)
    out = {}
    N, T, S = 2048, 8, 64
    for sfx, cplx in (('f32', False), ('c64', True)):
        cap = omp.CAP_COMPLEX if cplx else omp.CAP_REAL
        for B in (16, 1024):
            if a.small:
                B = max(B // 8, 1)
            Y, D, C = problem(B, N, T, S, cplx, gen)
            X = torch.empty((B, T, C), device='cuda', dtype=Y.dtype)
            it = ctypes.c_int(0)
            tag = '%s_B%d' % (sfx, B)
            ms, ms_mp = {}, {}
            for n in (1, 16, cap):
                def coder():
                    _hip.check(h, getattr(lib, 'dcp_tm_omp_' + sfx)(h, _arrays.ptr(Y), _arrays.ptr(D), _arrays.ptr(X), B,
                                                                    T, S, N, 1, 1, n, -1.0, ctypes.byref(it)),
                               'dcp_tm_omp')

                def pursuit():
                    _hip.check(h, getattr(lib, 'dcp_tm_pursuit_' + sfx)(h, _arrays.ptr(Y), _arrays.ptr(D),
                                                                        _arrays.ptr(X), B, T, S, N, 1, 1, n, -1.0, 0,
                                                                        ctypes.byref(it)), 'dcp_tm_pursuit')
                ms_mp[n], _ = timed(pursuit, a.runs)
                ms[n], sm = timed(coder, a.runs)
                out['%s/n%d/omp_ms' % (tag, n)] = round(ms[n], 4)
                out['%s/n%d/pursuit_ms' % (tag, n)] = round(ms_mp[n], 4)
                out['%s/n%d/omp_over_pursuit' % (tag, n)] = round(ms[n] / ms_mp[n], 3)
                print('%-12s n = %3d  orthogonal %9.4f ms (spread %.1f %%)   pursuit %9.4f ms   ratio %.2f   support %d'
                      % (tag, n, ms[n], 100 * (max(sm) - min(sm)) / ms[n], ms_mp[n], ms[n] / ms_mp[n], it.value))
            step_lo = 1000.0 * (ms[16] - ms[1]) / 15.0
            step_hi = 1000.0 * (ms[cap] - ms[16]) / (cap - 16.0)
            out[tag + '/step_us_2_16'] = round(step_lo, 3)
            out[tag + '/step_us_17_cap'] = round(step_hi, 3)
            out[tag + '/prepare_ms'] = round(ms[1], 4)
            line = '%-12s prepare %8.4f ms   step %7.3f us (2 .. 16), %7.3f us (17 .. %d)' % (tag, ms[1], step_lo, step_hi,
                                                                                             cap)
            out.update(('%s/n%d/dense_omp_ms' % (tag, n), None) for n in (16, cap))
            for n in (16, cap):
                key = '%s/n%d/dense_omp_ms' % (tag, n)
                need = (66.0 * (T * C) ** 2 + (T * C) * (N + B)) * Y.element_size() / 2.0 ** 30
                if need > a.dense_gib:
                    line += '   dense omp.solve: left out (%.0f GiB)' % need
                    break
                try:
                    A = tm._temp2mat(D, N, 1, 'SAME').reshape(T * C, N)
                    ms_d, _ = timed(lambda: omp.solve(Y, A, n_nonzero_coefs=n), a.runs)
                    out[key] = round(ms_d, 4)
                    out['%s/n%d/omp_over_dense' % (tag, n)] = round(ms[n] / ms_d, 4)
                    line += '   dense omp.solve(%d) %9.3f ms (ratio %.4f)' % (n, ms_d, ms[n] / ms_d)
                except RuntimeError as e:      # the dense workspace cannot be had
                    line += '   dense omp.solve(%d): %s' % (n, str(e).splitlines()[0][:60])
                    break
                finally:
                    A = None
            print(line)
            del Y, D, X
            torch.cuda.empty_cache()
    print(json.dumps({'runs': a.runs, 'small': a.small, 'figures': out}))


if __name__ == '__main__':
    main()
