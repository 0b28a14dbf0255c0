#!/usr/bin/env python3
"""The Gram-form LASSO on multichannel templates (dcp_tm_mc_lasso_*) at the documented template shape, against the only
route to the same codes before it: dcp_tm_lasso_* (residual form) on the channel-interleaved signal (y'[n Ch + ch],
D'[t, k Ch + ch], stride Ch, 'VALID'), at
    float32 and complex64    N = 2048, T = 8, S = 64, stride 1, 'VALID'    Ch = 4 and 32    B = 16 and B = 1024
with acc_ista, 10 iterations, tol = 0.  The time of an iteration is the difference of the 30- and the 10-iteration
calls over 20 (it includes the two further stop checks of the longer call); "prepare" is the 10-iteration call less 10
such iterations: the correlation pass over y, the lag correlations, the Gershgorin bound, the taps, the edge table.
From the iteration time, the step kernel's flop rate (2 B T C T (2 dh + 1), complex: x 4) as a fraction of the fp32
vector rate (--peak-tflops, 157.3: 256 CUs x 128 lanes x 2 flop x 2.4 GHz).  At Ch = 32 the same call with 'SAME' shows
what the edge table and the coefficients that read it cost.  Event-timed, median of --runs runs after one warm-up run,
one process.  Prints one line per figure and a JSON summary line; exits 1 if an iteration at Ch = 32 is not faster
than the interleaved route's.
    python tools/tm_basis_pursuit_bench.py [--runs 5] [--small]"""
import argparse
import ctypes
import json
import os
import statistics
import sys

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))

import torch  # noqa: E402
from decomp_amd import _arrays, _hip, template_matching as tm  # noqa: E402

ACC_ISTA = _hip.LASSO_ACC_ISTA


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
    return Y.contiguous(), D.contiguous()


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
    nd = 2 * (S - 1) + 1
    slower = []
    for sfx, cplx in (('f32', False), ('c64', True)):
        for Ch in (4, 32):
            for B in (16, 1024):
                if a.small:
                    B = max(B // 8, 1)
                Y, D = problem(B, N, T, Ch, S, cplx, gen)
                alpha = 0.5 / (Ch * N)      # threshold alpha Ch N / rho = 0.5 against events of amplitude 1 to 2
                Yi = Y.transpose(1, 2).reshape(B, N * Ch).contiguous()       # the interleaved route's operands
                Di = D.transpose(1, 2).reshape(T, S * Ch).contiguous()
                it = ctypes.c_int(0)
                tag = '%s_Ch%d_B%d' % (sfx, Ch, B)
                X = {pad: torch.empty((B, T, tm._coef_size(S, N, 1, pad)), device='cuda', dtype=Y.dtype)
                     for pad in ('VALID', 'SAME')}
                Xi = torch.empty_like(X['VALID'])

                def mc(n, pad='VALID'):
                    X[pad].zero_()
                    _hip.check(h, getattr(lib, 'dcp_tm_mc_lasso_' + sfx)(
                        h, _arrays.ptr(Y), _arrays.ptr(D), _arrays.ptr(X[pad]), B, T, Ch, S, N, 1,
                        0 if pad == 'VALID' else 1, alpha, 0.0, n, ACC_ISTA, 0, ctypes.byref(it)), 'dcp_tm_mc_lasso')

                def interleaved(n):
                    Xi.zero_()
                    _hip.check(h, getattr(lib, 'dcp_tm_lasso_' + sfx)(
                        h, _arrays.ptr(Yi), _arrays.ptr(Di), _arrays.ptr(Xi), B, T, S * Ch, N * Ch, Ch, 0, alpha, 0.0,
                        n, ACC_ISTA, 0, ctypes.byref(it)), 'dcp_tm_lasso')

                def figures(fn):
                    t10, t30 = timed(lambda: fn(10), a.runs), timed(lambda: fn(30), a.runs)
                    it_us = 1000.0 * (t30 - t10) / 20.0
                    return t10, it_us, t10 - 10 * it_us / 1000.0

                m10, m_it, m_prep = figures(mc)
                i10, i_it, i_prep = figures(interleaved)
                mc(10)
                interleaved(10)
                scale = float(Xi.abs().max())
                diff = float((X['VALID'] - Xi).abs().max()) / scale
                nz = float((Xi != 0).float().mean())
                C = X['VALID'].shape[-1]
                flop = 2.0 * B * T * C * T * nd * (4 if cplx else 1)
                frac = flop / (m_it * 1e-6) / (a.peak_tflops * 1e12)
                for k, v in (('mc_ms', m10), ('mc_iteration_us', m_it), ('mc_prepare_ms', m_prep),
                             ('interleaved_ms', i10), ('interleaved_iteration_us', i_it),
                             ('interleaved_prepare_ms', i_prep), ('step_fp32_fraction', frac),
                             ('difference_to_interleaved', diff), ('nonzero_share', nz)):
                    out['%s/%s' % (tag, k)] = round(v, 6)
                print('%-16s call(10) %9.4f ms (interleaved %9.4f, ratio %.3f)   iteration %8.2f us (interleaved %8.2f, '
                      'ratio %.3f)   prepare %8.4f ms (interleaved %8.4f)'
                      % (tag, m10, i10, m10 / i10, m_it, i_it, m_it / i_it, m_prep, i_prep))
                print('%-16s step kernel %.1f %% of the fp32 vector rate   max |x - x_interleaved| / max |x| %.2g   '
                      'non-zero %.1f %%' % (tag, 100 * frac, diff, 100 * nz))
                if Ch == 32:
                    if m_it >= i_it:
                        slower.append(tag)
                    s10, s_it, s_prep = figures(lambda n: mc(n, 'SAME'))
                    for k, v in (('same_ms', s10), ('same_iteration_us', s_it), ('same_prepare_ms', s_prep)):
                        out['%s/%s' % (tag, k)] = round(v, 6)
                    print("%-16s 'SAME': call(10) %9.4f ms   iteration %8.2f us   prepare %8.4f ms   (over 'VALID': "
                          'call %.3f, iteration %.3f)' % (tag, s10, s_it, s_prep, s10 / m10, s_it / m_it))
                del Y, D, X, Xi, Yi, Di
                torch.cuda.empty_cache()
    print(json.dumps({'runs': a.runs, 'small': a.small, 'iteration_not_faster_at_Ch32': slower, 'figures': out}))
    return 1 if slower else 0


if __name__ == '__main__':
    sys.exit(main())
