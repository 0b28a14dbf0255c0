#!/usr/bin/env python3
"""Learning multichannel templates -- template_matching.solve(alpha=0, lasso_method='omp', lasso_iter=16) with
D [T, Ch, S] -- at the documented template shape,
    float32 and complex64    N = 2048, T = 8, S = 64, stride 1, 'VALID'    Ch = 4 and 32    B = 16 and B = 1024
and the parts of one outer iteration, all in one process: the coder (dcp_tm_mc_omp_*, 16 events per signal) and the
dictionary step (dcp_tm_mc_dstep_events_*, max_events = 16), event-timed, median of --runs runs after one warm-up run;
in a pass of its own, with the library's profile brackets on, the step's split into its partial sums (compaction,
tm_events_core_kernel, tm_events_yx_kernel: DCP_PROF_MISC), the rest of the statistics (batch sums, edge terms,
assembly: DCP_PROF_STATS less the former) and the update with the read-back (the remainder).  The outer iteration is a
host clock around solve(maxiter = --iters + 1, tol = 0), which ends in a synchronisation, over --iters.
The baseline is the only route to the same templates without the multichannel step: the one-channel solve on the
channel-interleaved signal (y'[n Ch + ch], D'[t, k Ch + ch], stride Ch, 'VALID'), whose XXt is [(T Ch S)^2].
--route interleaved times that route alone and uses nothing but the 2-D solve, so the same file runs on a tree without
the multichannel step.  yx_floor_us is the time tm_events_yx_kernel's traffic (every event reads Ch S samples of y,
every (signal, template) row writes Ch S partial sums) would take at --copy-tbps (6.29: the measured float4 copy rate
of the device); its kernel time comes from a kernel trace.  y holds 160 planted events per signal plus noise.
Prints one line per figure and a JSON summary line.
    python tools/tm_mc_learn_bench.py [--runs 7] [--iters 5] [--route mc|interleaved|both] [--only TAG] [--small]"""
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
from tm_multichannel_bench import problem, timed  # noqa: E402

N, T, S, EVENTS = 2048, 8, 64, 16
PROF_STATS, PROF_MISC = 4, 8          # DCP_PROF_STATS (all statistics kernels), DCP_PROF_MISC (the partial sums alone)


def wall_per_iteration(fn, iters, repeats=3):
    fn()
    walls = []
    for _ in range(repeats):
        torch.cuda.synchronize()
        t0 = time.perf_counter()
        fn()
        torch.cuda.synchronize()
        walls.append(1e3 * (time.perf_counter() - t0) / iters)
    return statistics.median(walls), walls


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument('--runs', type=int, default=7)
    ap.add_argument('--iters', type=int, default=5)
    ap.add_argument('--route', choices=('mc', 'interleaved', 'both'), default='both')
    ap.add_argument('--only', default=None, help='one shape, e.g. f32_Ch32_B1024')
    ap.add_argument('--small', action='store_true', help='B / 8 (a quick look)')
    ap.add_argument('--copy-tbps', type=float, default=6.29, help='copy rate of the device')
    a = ap.parse_args()
    lib, h = _arrays.lib_handle(torch.empty(1, device='cuda'))
    gen = torch.Generator(device='cuda')
    gen.manual_seed(1)
    out = {}
    slower = []
    for sfx, cplx in (('f32', False), ('c64', True)):
        for Ch in (4, 32):
            for B in (16, 1024):
                tag = '%s_Ch%d_B%d' % (sfx, Ch, B)
                if a.small:
                    B = max(B // 8, 1)
                Y, D, C = problem(B, N, T, Ch, S, cplx, gen)      # (drawn for every shape: --only sees the same data)
                if a.only not in (None, tag):
                    continue
                kw = dict(maxiter=a.iters + 1, tol=0, lasso_method='omp', lasso_iter=EVENTS, lasso_tol=None)
                if a.route in ('mc', 'both'):
                    X = torch.empty((B, T, C), device='cuda', dtype=Y.dtype)
                    XXt = torch.empty((T * S, T * S), device='cuda', dtype=Y.dtype)
                    yX = torch.empty((T * Ch * S,), device='cuda', dtype=Y.dtype)
                    Dw = D.clone()
                    it = ctypes.c_int(0)

                    def coder():
                        _hip.check(h, getattr(lib, 'dcp_tm_mc_omp_' + sfx)(
                            h, _arrays.ptr(Y), _arrays.ptr(D), _arrays.ptr(X), B, T, Ch, S, N, 1, 0, EVENTS, -1.0,
                            ctypes.byref(it)), 'dcp_tm_mc_omp')

                    def step():          # (the step updates D in place: every run starts from the same D)
                        Dw.copy_(D)
                        tm._dstep_events(Y, X, Dw, XXt, yX, 1, 'VALID', 0, EVENTS)
                    ms_c, _ = timed(coder, a.runs)
                    nnz = int((X != 0).sum(dim=(1, 2)).max())
                    ms_s, s_s = timed(step, a.runs)
                    lib.dcp_profile_enable(h, 1)
                    lib.dcp_profile_reset(h)
                    for _ in range(a.runs):
                        step()
                    part, allst, cnt = ctypes.c_double(0), ctypes.c_double(0), ctypes.c_int64(0)
                    _hip.check(h, lib.dcp_profile_read(h, PROF_MISC, ctypes.byref(part), ctypes.byref(cnt)), 'profile')
                    _hip.check(h, lib.dcp_profile_read(h, PROF_STATS, ctypes.byref(allst), ctypes.byref(cnt)), 'profile')
                    lib.dcp_profile_enable(h, 0)
                    ms_p, ms_st = part.value / a.runs, allst.value / a.runs
                    ms_o, w_o = wall_per_iteration(lambda: tm.solve(Y, D, 0, stride=1, padding='VALID', **kw), a.iters)
                    item = Y.element_size()
                    yx_bytes = (B * EVENTS + B * T) * Ch * S * item
                    out[tag + '/outer_iteration_ms'] = round(ms_o, 4)
                    out[tag + '/coder_ms'] = round(ms_c, 4)
                    out[tag + '/dstep_ms'] = round(ms_s, 4)
                    out[tag + '/dstep_partials_ms'] = round(ms_p, 4)
                    out[tag + '/dstep_stats_ms'] = round(ms_st, 4)
                    out[tag + '/yx_bytes'] = yx_bytes
                    out[tag + '/yx_floor_us'] = round(yx_bytes / (a.copy_tbps * 1e12) * 1e6, 3)
                    out[tag + '/max_events_in_a_signal'] = nnz
                    print('%-16s outer iteration %9.4f ms (spread %.0f %%)   coder %9.4f ms   D step %8.4f ms (spread '
                          '%.0f %%): partial sums %7.4f, other statistics %7.4f, update and read-back %7.4f   yX floor '
                          '%.2f us' % (tag, ms_o, 100 * (max(w_o) - min(w_o)) / ms_o, ms_c, ms_s,
                                       100 * (max(s_s) - min(s_s)) / ms_s, ms_p, ms_st - ms_p, ms_s - ms_st,
                                       out[tag + '/yx_floor_us']))
                    del X, XXt, yX, Dw
                if a.route in ('interleaved', 'both'):
                    Yi = Y.transpose(1, 2).reshape(B, N * Ch).contiguous()
                    Di = D.transpose(1, 2).reshape(T, S * Ch).contiguous()
                    ms_i, w_i = wall_per_iteration(lambda: tm.solve(Yi, Di, 0, stride=Ch, padding='VALID', **kw),
                                                   a.iters, repeats=2)
                    out[tag + '/interleaved_outer_iteration_ms'] = round(ms_i, 4)
                    print('%-16s interleaved route: outer iteration %9.4f ms (spread %.0f %%), XXt of %.2f GiB'
                          % (tag, ms_i, 100 * (max(w_i) - min(w_i)) / ms_i,
                             (T * Ch * S) ** 2 * Y.element_size() / 2.0 ** 30))
                    if a.route == 'both' and ms_o > ms_i:
                        slower.append(tag)
                    del Yi, Di
                del Y, D
                torch.cuda.empty_cache()
    print(json.dumps({'runs': a.runs, 'iters': a.iters, 'route': a.route, 'small': a.small,
                      'slower_than_interleaved': slower, 'figures': out}))
    return 1 if slower else 0


if __name__ == '__main__':
    sys.exit(main())
