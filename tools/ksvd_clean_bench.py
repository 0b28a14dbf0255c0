#!/usr/bin/env python3
"""K-SVD with replacement of unused and duplicate atoms (dcp_ksvd_clean_step_*, dcp_ksvd_clean_*): milliseconds per
iteration with and without the cleaning pass, float32, at
    65536 x 4096, K = 512, s = 16        65536 x 4096, K = 256, s = 8
without a mask and with 30 % of the entries missing (a 0 / 1 mask row of its own for every data row).  Event-timed
around the library calls (their host synchronisations included; the replacement kernels a clean step leaves in flight
are inside the interval), median of --runs runs after one warm-up run, one process.  The start is the planted
dictionary whose last n atoms are copies of its first n: the coder never picks a copy (ties go to the lower index), so
exactly n atoms are unused after the sweep and marked, n = 0, 8 and K / 8.
    plain step        dcp_ksvd_step_* / dcp_ksvd_mask_step_* on that start: the iteration of replace_atoms=False
    marking only      dcp_ksvd_clean_step_* with stop_tol = +inf: the recount, the Gram product and the marking ride
                      along, nothing is replaced
    clean step        dcp_ksvd_clean_step_* with stop_tol = 0: energies, selection and replacement of the n atoms too
    pass alone        dcp_ksvd_clean_* on the (X, D) a plain step leaves: R = Y - X D again (not part of a step), the
                      marking and the replacement; with n = 0 it is the residual product and the marking alone, so
                      the difference to it is energies + selection + replacement, and `no threshold` (max_coherence
                      0) drops the Gram product and the coherence walk
Prints one line per figure and a JSON summary line.
    python tools/ksvd_clean_bench.py [--runs 5] [--small]"""
import argparse
import ctypes
import json
import math
import os
import sys

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))

import torch  # noqa: E402
from decomp_amd import _arrays, _hip  # noqa: E402
from ksvd_bench import timed  # noqa: E402
from omp_bench import problem  # noqa: E402

MU = 0.99


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument('--runs', type=int, default=5)
    ap.add_argument('--small', action='store_true', help='N / 8 (a quick look)')
    a = ap.parse_args()
    lib, h = _arrays.lib_handle(torch.empty(1, device='cuda'))
    gen = torch.Generator(device='cuda')
    gen.manual_seed(1)
    out = {}
    sfx = 'f32'
    for N, F, K, s in [(65536, 4096, 512, 16), (65536, 4096, 256, 8)]:
        if a.small:
            N //= 8
        Y, A = problem(N, F, K, False, gen)
        for masked in (False, True):
            M = (torch.rand((N, F), generator=gen, device='cuda') < 0.7).to(torch.float32) if masked else None
            ndim = 2 if masked else 0
            X = torch.empty((N, K), device='cuda', dtype=Y.dtype)
            D = torch.empty_like(A)
            it, nm, nr, md = ctypes.c_int(0), ctypes.c_int(0), ctypes.c_int(0), ctypes.c_double(0)
            tag = '%s_%dx%dk%ds%d%s' % (sfx, N, F, K, s, '_masked' if masked else '')

            def plain_step():
                if masked:
                    rc = getattr(lib, 'dcp_ksvd_mask_step_' + sfx)(h, _arrays.ptr(Y), _arrays.ptr(M), 2, _arrays.ptr(X),
                                                                  _arrays.ptr(D), N, F, K, s, -1.0, 0, ctypes.byref(md),
                                                                  ctypes.byref(it))
                else:
                    rc = getattr(lib, 'dcp_ksvd_step_' + sfx)(h, _arrays.ptr(Y), _arrays.ptr(X), _arrays.ptr(D), N, F,
                                                             K, s, -1.0, ctypes.byref(md), ctypes.byref(it))
                _hip.check(h, rc, 'plain step')

            def clean_step(stop, mu=MU):
                rc = getattr(lib, 'dcp_ksvd_clean_step_' + sfx)(h, _arrays.ptr(Y), _arrays.ptr(M), ndim, _arrays.ptr(X),
                                                               _arrays.ptr(D), N, F, K, s, -1.0, 0, ctypes.byref(md),
                                                               ctypes.byref(it), mu, stop, ctypes.byref(nm))
                _hip.check(h, rc, 'clean step')

            def pass_alone(mu=MU):
                rc = getattr(lib, 'dcp_ksvd_clean_' + sfx)(h, _arrays.ptr(Y), _arrays.ptr(M), ndim, _arrays.ptr(X),
                                                          _arrays.ptr(D), N, F, K, mu, ctypes.byref(nm),
                                                          ctypes.byref(nr))
                _hip.check(h, rc, 'pass alone')

            fig = {}
            for n in (0, 8, K // 8):
                D0 = A.clone()
                if n:
                    D0[K - n:] = D0[:n]

                def start():
                    D.copy_(D0)
                ms_plain = timed(start, plain_step, a.runs)
                ms_mark = timed(start, lambda: clean_step(math.inf), a.runs)
                n_marked = nm.value
                ms_clean = timed(start, lambda: clean_step(0.0), a.runs)
                assert nm.value == n_marked, (nm.value, n_marked)
                start()
                plain_step()
                X1, D1 = X.clone(), D.clone()

                def swept():
                    X.copy_(X1)
                    D.copy_(D1)
                ms_alone = timed(swept, pass_alone, a.runs)
                replaced = nr.value
                ms_alone_nomu = timed(swept, lambda: pass_alone(0.0), a.runs)
                fig['marked_%d' % n] = {'marked': n_marked, 'replaced': replaced, 'plain_step_ms': round(ms_plain, 4),
                                        'marking_only_step_ms': round(ms_mark, 4),
                                        'clean_step_ms': round(ms_clean, 4),
                                        'clean_step_over_plain': round(ms_clean / ms_plain, 5),
                                        'pass_alone_ms': round(ms_alone, 4),
                                        'pass_alone_no_threshold_ms': round(ms_alone_nomu, 4)}
                print('%-34s %3d marked: plain step %9.3f ms, marking only %9.3f, clean step %9.3f (%+.2f %%); pass '
                      'alone %8.3f ms, without threshold %8.3f'
                      % (tag, n_marked, ms_plain, ms_mark, ms_clean, 100 * (ms_clean / ms_plain - 1), ms_alone,
                         ms_alone_nomu))
                del X1, D1, D0
            base = fig['marked_0']['pass_alone_ms']
            for n in (8, K // 8):
                extra = fig['marked_%d' % n]['pass_alone_ms'] - base
                fig['marked_%d' % n]['energies_selection_replacement_ms'] = round(extra, 4)
                print('%-34s %3d marked: energies + selection + replacement %8.3f ms (pass alone minus the pass with '
                      'nothing marked, %.3f ms: residual product, recount, Gram product, marking)'
                      % (tag, n, extra, base))
            out[tag] = fig
            del X, D, M
            torch.cuda.empty_cache()
        del Y, A
        torch.cuda.empty_cache()
    print(json.dumps({'runs': a.runs, 'small': a.small, 'figures': out}))


if __name__ == '__main__':
    main()
