// The dictionary step of template learning for SPARSE codes: the statistics of x from per-row event lists.
//
// tm_stats_core_kernel and tm_stats_yx_kernel walk all C coefficients of a row per output cell.  The codes of the
// greedy coders (template_pursuit.hpp, template_omp.hpp) hold at most n_steps non-zeros per signal, so nearly every
// term they add is an exact zero.  Here the non-zeros of every row (b, t) of x are first compacted into a list of
// positions, in ascending c, and the two statistics are then summed over the listed positions only:
//   mpart[((b T + t) T + t') nd + (d + dh)] = sum_(events c of row (b, t) in core(d)) x[b, t, c] conj(x[b, t', c + d])
//   yxpart[((b T + t) Ch + ch) S + k]       = sum_(events c of row (b, t) in window(k, 0)) x[b, t, c] y[b, ch, s c - Q + k]
// with the right factors read from the dense x and y.  Everything after these partial sums (edge terms, assembly,
// the D update) is tm_dstep_around of template_impl.hpp, shared with the dense step.
//
// Multichannel templates D [T, Ch, S] (y [B, Ch, N], x [B, T, C]: one coefficient per event for all channels;
// TmGeom::Ch, 1 for D [T, S]).  x is shared by the channels, so the Gram statistic is the one-channel XXt [T S, T S]:
// the compaction, tm_events_core_kernel, the edge terms and the assembly do not see Ch.  Only yX gains the channel
// axis, channel by channel the same sum, and the update of tm_dstep_around takes the product XXt D per channel and
// normalises a template over its Ch S entries.
//
// The result equals the dense step's bit for bit: the terms are added in the same ascending order by the same
// tm_stat_madd (one spelling of the complex product, so that no two kernels fuse it differently), and a left-out term
// has the left factor 0, for which tm_stat_madd(acc, 0, v) == acc (the accumulator starts at +0 and so never is -0
// when a zero term meets it).  PRECONDITION: x and y are finite.  The dense kernels turn 0 * inf into NaN
// at a term that is left out here.
//
// max_events bounds the list of a row: cap = min(max_events, C) positions are stored, the count runs on past them.  A
// row that holds more (ev_n > cap) is walked over all its c by the same loop body, which skips the zeros, so
// max_events decides the speed and never the result; there is no error path and no extra synchronisation.  No
// atomics, no waiting between workgroups: two runs give the same bits.
#pragma once

namespace dcp {

constexpr int kTmEvChunk = 256;   // events staged in LDS at a time (= the workgroup size)

// -0.0 counts as zero
template <class T>
DCP_HD bool tm_nonzero(T v) {
    if constexpr (scalar_traits<T>::is_complex) return v.re != 0 || v.im != 0;
    else return v != 0;
}

// One wave per row (b, t), four rows per workgroup: C is walked in chunks of 64, a ballot gives every non-zero its
// place behind those of the lower lanes and of the chunks before, so the list ascends by construction.
//   ev_c[row cap + 0 .. min(ev_n, cap))  the first cap positions;   ev_n[row]  the count of all non-zeros
template <class T>
__global__ void __launch_bounds__(256) tm_events_compact_kernel(const T* __restrict__ x, long rows, long C, long cap,
                                                                int* __restrict__ ev_c, int* __restrict__ ev_n) {
    const int lane = threadIdx.x & 63;
    const long row = (long)blockIdx.x * 4 + (threadIdx.x >> 6);
    if (row >= rows) return;   // the whole wave; the kernel has no barrier
    const T* xr = x + row * C;
    int* out = ev_c + row * cap;
    long n = 0;
    for (long c0 = 0; c0 < C; c0 += 64) {
        const long c = c0 + lane;
        const bool nz = c < C && tm_nonzero(xr[c]);
        const unsigned long long m = __ballot(nz);
        const long pos = n + __popcll(m & ((1ull << lane) - 1ull));
        if (nz && pos < cap) out[pos] = (int)c;
        n += __popcll(m);
    }
    if (lane == 0) ev_n[row] = (int)n;
}

// The events (c, x[b, t, c]) of one row, in ascending c, kTmEvChunk at a time through LDS: every thread of the
// workgroup calls this (it has barriers), and gets f(c, v) for each event in order.  A row whose list overflowed
// (ev_n > cap) is walked over all its c instead; f is then not called at the zeros.
template <class T, class F>
__device__ __forceinline__ void tm_events_walk(const T* __restrict__ xa, const int* __restrict__ lst, long n_all,
                                               long cap, long C, int* sc, T* sv, F&& f) {
    const bool listed = n_all <= cap;
    const long nsrc = listed ? n_all : C;
    for (long e0 = 0; e0 < nsrc; e0 += kTmEvChunk) {
        __syncthreads();
        const long e = e0 + threadIdx.x;
        if (e < nsrc) {
            const long c = listed ? (long)lst[e] : e;
            sc[threadIdx.x] = (int)c;
            sv[threadIdx.x] = xa[c];
        }
        __syncthreads();
        const int m = nsrc - e0 < kTmEvChunk ? (int)(nsrc - e0) : kTmEvChunk;
        for (int i = 0; i < m; ++i) {
            const T v = sv[i];
            if (tm_nonzero(v)) f((long)sc[i], v);
        }
    }
}

// One workgroup per row (b, t); its T nd cells (t', d) go over the threads, 256 at a time.
template <class T>
__global__ void __launch_bounds__(256) tm_events_core_kernel(const T* __restrict__ x, TmGeom g, long cap,
                                                             const int* __restrict__ ev_c,
                                                             const int* __restrict__ ev_n, T* __restrict__ mpart) {
    __shared__ int sc[kTmEvChunk];
    __shared__ T sv[kTmEvChunk];
    const long bt = blockIdx.x, b = bt / g.T;
    const T* xa = x + bt * g.C;
    const long nd = g.nd(), cells = g.T * nd;
    const long n_all = ev_n[bt];
    for (long q0 = 0; q0 < cells; q0 += 256) {
        const long q = q0 + threadIdx.x;
        const bool live = q < cells;
        const long tp = live ? q / nd : 0, d = (live ? q % nd : 0) - g.dh;
        long cl, ch, ul, uh;
        g.core(d, &cl, &ch, &ul, &uh);
        const T* xb = x + (b * g.T + tp) * g.C;
        T acc = zero_of<T>();
        tm_events_walk(xa, ev_c + bt * cap, n_all, cap, g.C, sc, sv, [&](long c, T v) {
            if (live && c >= cl && c <= ch) acc = tm_stat_madd(acc, v, conj_of(xb[c + d]));
        });
        if (live) mpart[bt * cells + q] = acc;
    }
}

// One workgroup per row (b, t) and block of 256 of its Ch S cells (ch, k), k fastest over the lanes: an event is one
// coalesced read of y per channel, and a workgroup walks the event list once.  grid (B T, ceil(Ch S / 256)).
template <class T>
__global__ void __launch_bounds__(256) tm_events_yx_kernel(const T* __restrict__ y, const T* __restrict__ x, TmGeom g,
                                                           long cap, const int* __restrict__ ev_c,
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

// tm_dstep with the two partial sums taken from event lists of at most max_events positions per row of X, for
// Y [B, Ch, N], D [T, Ch, S], yX [T Ch S] (g.Ch channels; 1: Y [B, N], D [T, S]); XXt [T S, T S].  Both
// dcp_tm_dstep_events_* and dcp_tm_mc_dstep_events_* are this function after their geometry.
template <class T>
inline int tm_dstep_events(dcp_handle* h, const T* Y, const T* X, T* D, T* XXt, T* yX, const TmGeom& g, int acc_it,
                           int64_t max_events, double* maxdiff) {
    if (!Y || !X || !D || !XXt || !yX || !maxdiff) return fail(h, DCP_ERR_INVALID, "null pointer");
    if (acc_it < 0) return fail(h, DCP_ERR_INVALID, "acc_it must be >= 0");
    if (max_events < 1) return fail(h, DCP_ERR_INVALID, "max_events must be >= 1");
    hipStream_t st = h->stream;
    const long hmax = tm_hmax(g), rows = g.B * g.T, blocks = (g.Ch * g.S + 255) / 256;
    const long cap = max_events < (int64_t)g.C ? (long)max_events : g.C;
    if (blocks > 65535) return fail(h, DCP_ERR_INVALID, "multichannel D step: Ch S exceeds 65535 * 256");
    if (rows > 0x7fffffffL) return fail(h, DCP_ERR_INVALID, "event D step: B T exceeds 2^31 - 1");
    TmDstepWs<T> w;
    int *ev_c = nullptr, *ev_n = nullptr;   // the position lists take no more room than X: cap <= C 32-bit words a row
    DCP_TRY(ws_lay_out(h, [&](WsLayout& a) {
        tm_dstep_layout(a, w, g, hmax);
        a.take(ev_c, rows * cap);
        a.take(ev_n, rows);
    }));
    return tm_dstep_around<T>(h, w, X, D, XXt, yX, g, hmax, acc_it, maxdiff, [&]() -> int {
        hipLaunchKernelGGL((tm_events_compact_kernel<T>), dim3((unsigned)((rows + 3) / 4)), dim3(256), 0, st, X, rows,
                           g.C, cap, ev_c, ev_n);
        DCP_LAUNCH_OK(h, hipGetLastError());
        hipLaunchKernelGGL((tm_events_core_kernel<T>), dim3((unsigned)rows), dim3(256), 0, st, X, g, cap,
                           (const int*)ev_c, (const int*)ev_n, w.mpart);
        DCP_LAUNCH_OK(h, hipGetLastError());
        hipLaunchKernelGGL((tm_events_yx_kernel<T>), dim3((unsigned)rows, (unsigned)blocks), dim3(256), 0, st, Y, X, g,
                           cap, (const int*)ev_c, (const int*)ev_n, w.yxpart);
        DCP_LAUNCH_OK(h, hipGetLastError());
        return DCP_OK;
    });
}

template <class T>
inline int tm_dstep_events_api(dcp_handle* h, const T* Y, const T* X, T* D, T* XXt, T* yX, const TmShape& sh,
                               int acc_it, int64_t max_events, double* maxdiff) {
    TmGeom g;
    DCP_TRY(tm_geom_api(h, sh, g));
    return tm_dstep_events<T>(h, Y, X, D, XXt, yX, g, acc_it, max_events, maxdiff);
}

}  // namespace dcp
