#!/usr/bin/env python3
"""Matching pursuit on multichannel templates (dcp_tm_mc_pursuit_*) at the documented template shape, against the only
route to the same code before it: dcp_tm_pursuit_* on the channel-interleaved signal (y'[n Ch + ch], D'[t, k Ch + ch],
stride Ch, 'VALID'), at
    float32 and complex64    N = 2048, T = 8, S = 64, stride 1, 'VALID'    Ch = 4 and 32    B = 16 and B = 1024
with n_nonzero_coefs = 16 (and 128 for the time of a step: the difference of the 128- and the 16-step calls over
112; "prepare" is the 16-step call less 16 such steps).  The correlation kernel alone is read from the library's
profile brackets (DCP_PROF_XUPDATE) in a run of its own; from it the achieved flop rate (2 B T C Ch S, complex: x 4)
as a fraction of the fp32 vector rate (--peak-tflops, 157.3: 256 CUs x 128 lanes x 2 flop x 2.4 GHz), and its time
relative to Ch x the one-channel pass (tm_corr_store_kernel) on channel 0 of the same data.  Event-timed, median of
--runs runs after one warm-up run, one process.  y holds 160 planted events per signal plus noise, so no signal stops
before 128 steps.  Prints one line per figure and a JSON summary line.
    python tools/tm_multichannel_bench.py [--runs 5] [--small]"""
import argparse
import ctypes
import json
import os
import statistics
import sys

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))

import torch  # noqa: E402
from decomp_amd import _arrays, _hip, template_matching as tm  # noqa: E402

PROF_XUPDATE = 2


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


def corr_ms(lib, h, fn, runs):
    """Median time of the correlation pass inside fn(), from the library's profile brackets."""
    samples = []
    _hip.check(h, lib.dcp_profile_select(h, 1 << PROF_XUPDATE), 'dcp_profile_select')
    _hip.check(h, lib.dcp_profile_enable(h, 1), 'dcp_profile_enable')
    for r in range(runs + 1):
        _hip.check(h, lib.dcp_profile_reset(h), 'dcp_profile_reset')
        fn()
        ms, cnt = ctypes.c_double(0.0), ctypes.c_int64(0)
        _hip.check(h, lib.dcp_profile_read(h, PROF_XUPDATE, ctypes.byref(ms), ctypes.byref(cnt)), 'dcp_profile_read')
        assert cnt.value == 1
        if r > 0:
            samples.append(ms.value)
    _hip.check(h, lib.dcp_profile_enable(h, 0), 'dcp_profile_enable')
    _hip.check(h, lib.dcp_profile_select(h, 0xffffffff), 'dcp_profile_select')
    return statistics.median(samples)


def problem(B, N, T, Ch, S, cplx, gen, events=160):
    def randn(*s):
        r = torch.randn(s, generator=gen, device='cuda')
        return torch.complex(r, torch.randn(s, generator=gen, device='cuda')) if cplx else r
    D = randn(T, Ch, S)
    D /= D.reshape(T, -1).norm(dim=1)[:, None, None]
    C = tm._coef_size(S, N, 1, 'VALID')
    x0 = torch.zeros((B, T * C), device='cuda', dtype=D.dtype)
    cols = torch.randint(0, T * C, (B, events), generator=gen, device='cuda')
    x0.scatter_(1, cols, (1.0 + torch.rand((B, events), generator=gen, device='cuda')).to(D.dtype))
    Y = tm.predict(x0.reshape(B, T, C), D, N, 1, 'VALID')     # (set-up only: the timed calls are the library's)
    Y += 0.05 * Y.abs().mean() * randn(B, Ch, N)
    return Y.contiguous(), D.contiguous(), C


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument('--runs', type=int, default=5)
    ap.add_argument('--small', action='store_true', help='B / 8 (a quick look)')
    ap.add_argument('--peak-tflops', type=float, default=157.3, help='fp32 vector rate of the device')
    a = ap.parse_args()
    lib, h = _arrays.lib_handle(torch.empty(1, device='cuda'))
    gen = torch.Generator(device='cuda')
    gen.manual_seed(1)
    out = {}
    N, T, S = 2048, 8, 64
    slower = []
    for sfx, cplx in (('f32', False), ('c64', True)):
        for Ch in (4, 32):
            for B in (16, 1024):
                if a.small:
                    B = max(B // 8, 1)
                Y, D, C = problem(B, N, T, Ch, S, cplx, gen)
                Yi = Y.transpose(1, 2).reshape(B, N * Ch).contiguous()       # the interleaved route's operands
                Di = D.transpose(1, 2).reshape(T, S * Ch).contiguous()
                Y0, D0 = Y[:, 0].contiguous(), D[:, 0].contiguous()          # one channel of the same data
                X = torch.empty((B, T, C), device='cuda', dtype=Y.dtype)
                Xi = torch.empty((B, T, C), device='cuda', dtype=Y.dtype)
                it = ctypes.c_int(0)
                tag = '%s_Ch%d_B%d' % (sfx, Ch, B)

                def mc(n):
                    _hip.check(h, getattr(lib, 'dcp_tm_mc_pursuit_' + sfx)(
                        h, _arrays.ptr(Y), _arrays.ptr(D), _arrays.ptr(X), B, T, Ch, S, N, 1, 0, n, -1.0, 0,
                        ctypes.byref(it)), 'dcp_tm_mc_pursuit')

                def interleaved(n):
                    _hip.check(h, getattr(lib, 'dcp_tm_pursuit_' + sfx)(
                        h, _arrays.ptr(Yi), _arrays.ptr(Di), _arrays.ptr(Xi), B, T, S * Ch, N * Ch, Ch, 0, n, -1.0, 0,
                        ctypes.byref(it)), 'dcp_tm_pursuit')

                def one_channel(n):
                    _hip.check(h, getattr(lib, 'dcp_tm_pursuit_' + sfx)(
                        h, _arrays.ptr(Y0), _arrays.ptr(D0), _arrays.ptr(Xi), B, T, S, N, 1, 0, n, -1.0, 0,
                        ctypes.byref(it)), 'dcp_tm_pursuit')

                ms = {}
                for n in (16, 128):
                    ms[n], sm = timed(lambda: mc(n), a.runs)
                    out['%s/n%d/mc_ms' % (tag, n)] = round(ms[n], 4)
                ms_i, _ = timed(lambda: interleaved(16), a.runs)
                mc(16)
                same = bool(torch.equal(X != 0, Xi != 0))
                step_us = 1000.0 * (ms[128] - ms[16]) / 112.0
                prepare = ms[16] - 16 * step_us / 1000.0
                c_mc = corr_ms(lib, h, lambda: mc(16), a.runs)
                c_il = corr_ms(lib, h, lambda: interleaved(16), a.runs)
                c_one = corr_ms(lib, h, lambda: one_channel(16), a.runs)
                flop = 2.0 * B * T * C * Ch * S * (4 if cplx else 1)
                frac = flop / (c_mc * 1e-3) / (a.peak_tflops * 1e12)
                out[tag + '/interleaved_n16_ms'] = round(ms_i, 4)
                out[tag + '/step_us'] = round(step_us, 3)
                out[tag + '/prepare_ms'] = round(prepare, 4)
                out[tag + '/corr_ms'] = round(c_mc, 4)
                out[tag + '/corr_interleaved_ms'] = round(c_il, 4)
                out[tag + '/corr_one_channel_ms'] = round(c_one, 4)
                out[tag + '/corr_fp32_fraction'] = round(frac, 4)
                out[tag + '/corr_over_ch_one_channel'] = round(c_mc / (Ch * c_one), 4)
                if ms[16] > ms_i:
                    slower.append(tag)
                print('%-16s mc(16) %9.4f ms   interleaved(16) %9.4f ms   ratio %.3f   step %8.3f us   prepare %8.4f ms'
                      % (tag, ms[16], ms_i, ms[16] / ms_i, step_us, prepare))
                print('%-16s corr %9.4f ms (interleaved %9.4f, one channel %9.4f)   %.1f %% of the fp32 vector rate   '
                      'corr / (Ch x one channel) %.3f   same support as interleaved: %s'
                      % (tag, c_mc, c_il, c_one, 100 * frac, c_mc / (Ch * c_one), same))
                del Y, D, X, Xi, Yi, Di, Y0, D0
                torch.cuda.empty_cache()
    print(json.dumps({'runs': a.runs, 'small': a.small, 'slower_than_interleaved': slower, 'figures': out}))
    return 1 if slower else 0


if __name__ == '__main__':
    sys.exit(main())
