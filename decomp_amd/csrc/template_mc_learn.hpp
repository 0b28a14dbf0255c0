// The dictionary step of template learning for multichannel templates D [T, Ch, S] (y [B, Ch, N], x [B, T, C]: one
// coefficient per event for all channels), on the event lists of template_events.hpp.
//
// x is shared by the channels, so the Gram statistic is the one-channel XXt [T S, T S]: the compaction,
// tm_events_core_kernel, the edge terms and the assembly run as they do for one channel.  Only yX gains the channel
// axis,
//   yxpart[((b T + t) Ch + ch) S + k] = sum_(events c of row (b, t) in window(k, 0)) x[b, t, c] y[b, ch, s c - Q + k],
// channel by channel the sum tm_events_yx_kernel forms (the same terms in ascending c, tm_stat_madd from +0), and the
// update of tm_dstep_around takes the product XXt D per channel and normalises a template over its Ch S entries.  At
// Ch = 1 every number is the one-channel step's, bit for bit.  No atomics, no waiting between workgroups; max_events
// decides the speed and never the result.
#pragma once

namespace dcp {

// One workgroup per row (b, t) and block of 256 of its Ch S cells (ch, k), k fastest over the lanes: an event is one
// coalesced read of y per channel, and a workgroup walks the event list once.
template <class T>
__global__ void __launch_bounds__(256) tm_mc_events_yx_kernel(const T* __restrict__ y, const T* __restrict__ x,
                                                              TmGeom g, long cap, const int* __restrict__ ev_c,
                                                              const int* __restrict__ ev_n, T* __restrict__ yxpart) {
    __shared__ int sc[kTmEvChunk];
    __shared__ T sv[kTmEvChunk];
    const long bt = blockIdx.x, b = bt / g.T;
    const long cells = g.Ch * g.S, q = blockIdx.y * 256L + threadIdx.x;
    const bool live = q < cells;
    const long ch = live ? q / g.S : 0, k = live ? q % g.S : 0;
    const T* yb = y + (b * g.Ch + ch) * g.N;
    long lo, hi;
    g.window(k, 0, &lo, &hi);
    T acc = zero_of<T>();
    tm_events_walk(x + bt * g.C, ev_c + bt * cap, (long)ev_n[bt], cap, g.C, sc, sv, [&](long c, T v) {
        if (live && c >= lo && c <= hi) acc = tm_stat_madd(acc, v, yb[g.s * c - g.Q + k]);
    });
    if (live) yxpart[bt * cells + q] = acc;
}

// tm_dstep_events for Y [B, Ch, N], D [T, Ch, S], yX [T Ch S] (g.Ch channels); XXt [T S, T S].
template <class T>
inline int tm_mc_dstep_events(dcp_handle* h, const T* Y, const T* X, T* D, T* XXt, T* yX, const TmGeom& g, int acc_it,
                              int64_t max_events, double* maxdiff) {
    const long blocks = (g.Ch * g.S + 255) / 256;
    if (blocks > 65535) return fail(h, DCP_ERR_INVALID, "multichannel D step: Ch S exceeds 65535 * 256");
    return tm_dstep_events_with<T>(h, X, D, XXt, yX, g, acc_it, max_events, maxdiff,
                                   [&](long cap, const int* ev_c, const int* ev_n, T* yxpart) {
        hipLaunchKernelGGL((tm_mc_events_yx_kernel<T>), dim3((unsigned)(g.B * g.T), (unsigned)blocks), dim3(256), 0,
                           h->stream, Y, X, g, cap, ev_c, ev_n, yxpart);
    });
}

}  // namespace dcp
