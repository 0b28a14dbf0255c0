#!/usr/bin/env python3
"""Template learning with greedy codes -- template_matching.solve(alpha=0, lasso_method='omp', lasso_iter=16) -- at the
documented template shape,
    float32 and complex64    N = 2048, T = 8, S = 64, stride 1, 'SAME'    B = 16 and B = 1024
and the parts of one outer iteration, all in one process: the coder (dcp_tm_omp_*, 16 events per signal), the
dictionary step on event lists (dcp_tm_dstep_events_*, max_events = 16) and the dense dictionary step (dcp_tm_dstep_*)
on the same x, the two timed in turn, run after run.  Event-timed, median of --runs runs after one warm-up run; the
outer iteration is a host clock around solve(maxiter = --iters + 1, tol = 0), which ends in a synchronisation, over
--iters.  In a pass of its own, with the library's profile brackets on, the share of the dense step that its two
partial-sum kernels take (tm_stats_core_kernel, tm_stats_yx_kernel: what the event lists replace) and the share of
the event step that their replacements take (compaction included).  y holds 160 planted events per signal plus noise.
Both steps give the same bits (asserted here on D, XXt and yX).  Prints one line per figure and a JSON summary line.
    python tools/tm_learn_bench.py [--runs 7] [--iters 10] [--small]"""
import argparse
import ctypes
import json
import os
import statistics
import sys
import time

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))

import torch  # noqa: E402
from decomp_amd import _arrays, _hip, template_matching as tm  # noqa: E402
from tm_pursuit_bench import problem, timed  # noqa: E402

N, T, S, EVENTS = 2048, 8, 64, 16
PROF_STATS, PROF_MISC = 4, 8          # DCP_PROF_STATS (all statistics kernels), DCP_PROF_MISC (the partial sums alone)


def _bits(t):
    t = torch.view_as_real(t) if t.is_complex() else t
    return t.contiguous().view(torch.int32)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument('--runs', type=int, default=7)
    ap.add_argument('--iters', type=int, default=10)
    ap.add_argument('--small', action='store_true', help='B / 8 (a quick look)')
    a = ap.parse_args()
    lib, h = _arrays.lib_handle(torch.empty(1, device='cuda'))
    gen = torch.Generator(device='cuda')
    gen.manual_seed(1)
    out = {}
    for sfx, cplx in (('f32', False), ('c64', True)):
        for B in (16, 1024):
            if a.small:
                B = max(B // 8, 1)
            Y, D, C = problem(B, N, T, S, cplx, gen)
            X = torch.empty((B, T, C), device='cuda', dtype=Y.dtype)
            XXt = torch.empty((T * S, T * S), device='cuda', dtype=Y.dtype)
            yX = torch.empty((T * S,), device='cuda', dtype=Y.dtype)
            Dw = D.clone()
            it = ctypes.c_int(0)
            tag = '%s_B%d' % (sfx, B)

            def coder():
                _hip.check(h, getattr(lib, 'dcp_tm_omp_' + sfx)(h, _arrays.ptr(Y), _arrays.ptr(D), _arrays.ptr(X), B, T,
                                                                S, N, 1, 1, EVENTS, -1.0, ctypes.byref(it)),
                           'dcp_tm_omp')

            def events():
                tm._dstep_events(Y, X, Dw, XXt, yX, 1, 'SAME', 0, EVENTS)

            def dense():
                tm._dstep(Y, X, Dw, XXt, yX, 1, 'SAME', 0)

            def fresh(step):          # (the step updates D in place: every run starts from the same D)
                Dw.copy_(D)
                step()
                return Dw.clone(), XXt.clone(), yX.clone()
            ms_c, _ = timed(coder, a.runs)
            nnz = int((X != 0).sum(dim=(1, 2)).max())
            same = all(torch.equal(_bits(u), _bits(v)) for u, v in zip(fresh(events), fresh(dense)))
            assert same, 'the event step and the dense step differ'
            # the two steps in turn, run after run: a drift of the machine meets both
            s_e, s_d = [], []
            for r in range(a.runs + 1):
                for step, dst in ((events, s_e), (dense, s_d)):
                    Dw.copy_(D)
                    torch.cuda.synchronize()
                    e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
                    e0.record()
                    step()
                    e1.record()
                    torch.cuda.synchronize()
                    if r > 0:
                        dst.append(e0.elapsed_time(e1))
            ms_e, ms_d = statistics.median(s_e), statistics.median(s_d)
            # the share of the partial sums, from the library's own brackets, in a pass of its own
            share = {}
            for name, step in (('events', events), ('dense', dense)):
                lib.dcp_profile_enable(h, 1)
                lib.dcp_profile_reset(h)
                for _ in range(a.runs):
                    Dw.copy_(D)
                    step()
                part, allst, cnt = ctypes.c_double(0), ctypes.c_double(0), ctypes.c_int64(0)
                _hip.check(h, lib.dcp_profile_read(h, PROF_MISC, ctypes.byref(part), ctypes.byref(cnt)), 'profile')
                _hip.check(h, lib.dcp_profile_read(h, PROF_STATS, ctypes.byref(allst), ctypes.byref(cnt)), 'profile')
                lib.dcp_profile_enable(h, 0)
                share[name] = (part.value / a.runs, allst.value / a.runs)

            def outer():
                tm.solve(Y, D, 0, maxiter=a.iters + 1, tol=0, lasso_method='omp', lasso_iter=EVENTS, lasso_tol=None)
            outer()
            walls = []
            for _ in range(3):
                torch.cuda.synchronize()
                t0 = time.perf_counter()
                outer()
                torch.cuda.synchronize()
                walls.append(1e3 * (time.perf_counter() - t0) / a.iters)
            ms_o = statistics.median(walls)
            out[tag + '/coder_ms'] = round(ms_c, 4)
            out[tag + '/dstep_events_ms'] = round(ms_e, 4)
            out[tag + '/dstep_dense_ms'] = round(ms_d, 4)
            out[tag + '/events_over_dense'] = round(ms_e / ms_d, 4)
            out[tag + '/outer_iteration_ms'] = round(ms_o, 4)
            out[tag + '/dense_partials_ms'] = round(share['dense'][0], 4)
            out[tag + '/dense_stats_ms'] = round(share['dense'][1], 4)
            out[tag + '/dense_partials_share'] = round(share['dense'][0] / ms_d, 4)
            out[tag + '/events_partials_ms'] = round(share['events'][0], 4)
            out[tag + '/events_stats_ms'] = round(share['events'][1], 4)
            out[tag + '/max_events_in_a_signal'] = nnz
            print('%-10s outer iteration %9.4f ms   coder %9.4f ms   D step: events %8.4f ms (spread %.0f %%), dense '
                  '%9.4f ms (spread %.0f %%), ratio %.4f' % (tag, ms_o, ms_c, ms_e, 100 * (max(s_e) - min(s_e)) / ms_e,
                                                             ms_d, 100 * (max(s_d) - min(s_d)) / ms_d, ms_e / ms_d))
            print('%-10s partial sums: dense %9.4f ms of %9.4f ms of statistics (%.1f %% of the dense step); events '
                  '%8.4f ms of %8.4f ms' % (tag, share['dense'][0], share['dense'][1], 100 * share['dense'][0] / ms_d,
                                            share['events'][0], share['events'][1]))
            del Y, D, X, XXt, yX, Dw
            torch.cuda.empty_cache()
    print(json.dumps({'runs': a.runs, 'iters': a.iters, 'small': a.small, 'figures': out}))


if __name__ == '__main__':
    main()
