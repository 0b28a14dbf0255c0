// Convolutional matching pursuit on the template operator (template_matching.pursuit, dcp_tm_pursuit_*).
// Included from template_impl.hpp, whose geometry, lag correlations and correlation pass it uses.
//
// Per signal y [N], independent of the others, with A[(t, c), n] = D[t, n - s c + Q], rho2[t, c] = sum_n |A[(t, c), n]|^2
// over the taps inside [0, N), r = y, E = |y|^2, x = 0, at most n_steps times:
//   1. tol given and E <= tol: stop
//   2. alpha[t, c] = sum_n r[n] conj(A[(t, c), n]);  score = |alpha|^2 / rho2 over the atoms with rho2 > 0 (positive:
//      alpha^2 / rho2 over the atoms with alpha > 0); i* = the LOWEST flat index t C + c attaining the maximum;
//      maximum not > 0 (or NaN): stop
//   3. a = alpha* / rho2*;  x[i*] += a;  E -= score*;  r -= a A*
// Matching pursuit, not OMP: no re-fit on the support, an atom may be taken again (its coefficient accumulates).
//
// r is never formed.  alpha is kept up to date in Gram form: taking (t*, c*) changes only the atoms within dh of c*,
//   alpha[t', c'] -= a G,   G = sum_n A*[n] conj(A[(t', c'), n]) = Corr[t*, t', s (c* - c')]
// when every tap of the taken atom lies inside the signal (the `inside` rule of tm_gram_colsum_kernel), else the
// explicit sum over the overlap inside [0, N).
//
// Kernels.  Prepare: rho2 (tm_pursuit_rho2_kernel), Corr (tm_lagcorr_kernel), alpha0 = y A^H for all (b, t, c)
// (tm_corr_store_kernel: the correlation pass of the LASSO with a store-only epilogue; the dcp_tm_mc_* entries:
// tm_mc_corr_kernel of template_multichannel.hpp).  Then tm_pursuit_kernel: one
// 1024-thread workgroup (16 waves) per signal, the steps of a signal sequential, the signals concurrent; no waiting
// between workgroups, no float atomics (one integer max per signal for the step count), the loop bounded by n_steps.
// A step is a chain of dependent latencies, not of work, hence the wide workgroup: every phase is one pass.
//   arg-max     never rescans alpha.  A table holds, for every SEGMENT (a fixed run of kTmPursuitSeg = 64 flat
//               indices, one per lane), its best atom: (score, index) and that atom's alpha and rho2.  A step reduces
//               the table (each thread its entries, a 6-step butterfly per wave, the 16 wave results through LDS),
//               updates T (2 dh + 1) correlations and re-reduces only the segments those lie in: at most
//               T (ceil(2 dh / 64) + 1).  Ties go to the lower index at every level (lane, wave, segment, table):
//               the comparison is greedy_better of greedy.hpp throughout.
//   per step    3 workgroup barriers (table result | alpha update | segment refresh), T (2 dh + 1) multiply-adds
//               (one per thread up to 1024), <= T (ceil(2 dh / 64) + 1) segment reductions shared by 16 waves,
//               ceil(nseg / 1024) table entries per thread, 1 global read-modify-write of x by one thread.  The global
//               reads on the chain: Corr (update) and rho2 (refresh), one round trip each.
//   tiers       LDS:    T C <= kTmPursuitLdsBytes / sizeof(T) (36864 float, 18432 double / complex64, 9216
//                       complex128): alpha [T C] and the table live in LDS, at most 144 KiB + 9 KiB of the CU's
//                       160 KiB -- one resident workgroup per CU at the largest sizes, which is what a batch of
//                       B >= 256 signals wants on 256 CUs; smaller problems ask for less and share a CU.
//               global: above: alpha is updated in place in the alpha0 workspace [B, T C], the table in a
//                       per-signal workspace; both stay in L2 between steps.
//   x           written straight to global memory (zeroed by the kernel: the caller's X is written entirely).
// Every value a signal's workgroup computes depends on that signal, D and the geometry alone, in a fixed order:
// results are bitwise reproducible and bitwise independent of the rest of the batch.
//
// The pieces orthogonal pursuit (template_omp.hpp) runs on as well are defined here once: the prepare launches, the
// segment table with its `excluded` lanes, the table's best atom, |y|^2, the window of an atom, the Gram entry and the
// launch of a tier.
//
// Multichannel templates (D [T, Ch, S], y [B, Ch, N], one coefficient per event for all channels; dcp_tm_mc_*): a step
// reads y only through alpha0, rho2, Corr, the explicit overlap sum and |y|^2, so TmGeom::Ch (1 everywhere else) adds a
// channel loop to the last four (rho2 and Corr: tm_row_norm2 and tm_lagcorr_kernel of template_impl.hpp), each run once
// at Ch = 1, and tm_pursuit_prepare(mc) takes alpha0 from the correlation pass of template_multichannel.hpp.
#pragma once
#include "greedy.hpp"

namespace dcp {

constexpr int kTmPursuitSeg = 64;                     // flat indices per table entry: one per lane
constexpr int kTmPursuitThreads = 1024;
constexpr int kTmPursuitWaves = kTmPursuitThreads / 64;
constexpr size_t kTmPursuitLdsBytes = 144 * 1024;     // the LDS image of alpha in the LDS tier

// a segment's best atom
template <class T>
struct TmBest {
    T a;                 // its correlation
    real_t<T> s, r2;     // its score and rho2
    int i;               // its flat index
};

// the largest T C whose alpha is kept in LDS
template <class T>
constexpr long tm_pursuit_lds_atoms() { return (long)(kTmPursuitLdsBytes / sizeof(T)); }

inline long tm_pursuit_nseg(long K) { return (K + kTmPursuitSeg - 1) / kTmPursuitSeg; }

// LDS tier carve: alpha [K] (T), the table [nseg]
template <class T>
inline size_t tm_pursuit_lds_bytes(long K) {
    const size_t a = ((size_t)K * sizeof(T) + 15) & ~size_t(15);
    return a + (size_t)tm_pursuit_nseg(K) * sizeof(TmBest<T>);
}

// rho2[t, c] = |A_(t,c)|^2 over its taps inside [0, N) (not rho^2 of tm_rownorm_kernel: the square of a rounded
// root is not the sum); clears *it_zero
template <class T>
__global__ void __launch_bounds__(256) tm_pursuit_rho2_kernel(const T* __restrict__ D, TmGeom g,
                                                              real_t<T>* __restrict__ rho2, int* __restrict__ it_zero) {
    if (blockIdx.x == 0 && threadIdx.x == 0) *it_zero = 0;
    for (long i = blockIdx.x * 256L + threadIdx.x; i < g.T * g.C; i += (long)gridDim.x * 256L)
        rho2[i] = tm_row_norm2(D, g, i / g.C, i % g.C);
}

// alpha0[b, t, c] = (y A^H)[b, t, c]: tm_corr_step_kernel's pass with a store-only epilogue (same grid)
template <class T>
__global__ void __launch_bounds__(256) tm_corr_store_kernel(const T* __restrict__ y, const T* __restrict__ D, TmGeom g,
                                                            int lds_ok, T* __restrict__ alpha0) {
    const long t = blockIdx.y, b = blockIdx.z;
    const long c = (long)blockIdx.x * 256 + threadIdx.x;
    const T acc = tm_corr_tile(y, D, g, lds_ok, t, b, c);
    if (c < g.C) alpha0[(b * g.T + t) * g.C + c] = acc;
}

// |alpha|^2 / rho2 of an atom that may be taken, else -1 (rho2 = 0, positive and alpha <= 0, or a NaN: never wins)
template <class T>
__device__ __forceinline__ real_t<T> tm_pursuit_score(T a, real_t<T> rho2, int positive) {
    typedef real_t<T> R;
    bool ok = rho2 > R(0);
    if constexpr (!scalar_traits<T>::is_complex) ok = ok && (!positive || a > R(0));
    const R sc = abs2(a) / (ok ? rho2 : R(1));
    return (ok && sc >= R(0)) ? sc : R(-1);
}

// tab[seg] <- the best atom of flat indices [64 seg, 64 seg + 64) & [0, K) whose lane is not `excluded`; the whole wave
// calls it
template <class T>
__device__ __forceinline__ void tm_pursuit_segment(const T* al, const real_t<T>* __restrict__ rho2, int K, int seg,
                                                   int positive, bool excluded, TmBest<T>* tab) {
    typedef real_t<T> R;
    const int lane = threadIdx.x & 63;
    const int i = seg * kTmPursuitSeg + lane;
    const int ic = i < K ? i : K - 1;
    const T a = al[ic];
    const R r2 = rho2[ic];
    R sc = tm_pursuit_score(a, r2, positive);
    if (i >= K || excluded) sc = R(-1);
    int bi = i;
    greedy_wave_best(sc, bi);
    const int wl = bi - seg * kTmPursuitSeg;   // the winner's lane
    const T wa = lane_get(a, wl);
    const R wr = lane_get(r2, wl);
    if (lane == 0) tab[seg] = TmBest<T>{wa, sc, wr, bi};
}

// The table's best (score, index), the same in every thread: each thread its entries, the butterfly per wave, the
// wave results through shS / shI [kTmPursuitWaves].  One workgroup barrier, inside.
template <class T>
__device__ __forceinline__ void tm_pursuit_table_best(const TmBest<T>* tab, int nseg, real_t<T>* shS, int* shI,
                                                      real_t<T>& bs, int& bi) {
    const int tid = threadIdx.x;
    bs = real_t<T>(-1);
    bi = 0x7fffffff;
    for (int j = tid; j < nseg; j += kTmPursuitThreads) greedy_better(bs, bi, tab[j].s, tab[j].i);
    greedy_wave_best(bs, bi);
    if ((tid & 63) == 0) {
        shS[tid >> 6] = bs;
        shI[tid >> 6] = bi;
    }
    __syncthreads();
    bs = shS[0];
    bi = shI[0];
#pragma unroll
    for (int w = 1; w < kTmPursuitWaves; ++w) greedy_better(bs, bi, shS[w], shI[w]);
}

// |y|^2 in every thread, a fixed-order sum (shS [kTmPursuitWaves], *shE: LDS)
template <class T>
__device__ __forceinline__ real_t<T> tm_pursuit_ynorm2(const T* __restrict__ y, long N, real_t<T>* shS, real_t<T>* shE) {
    real_t<T> acc = 0;
    for (long n = threadIdx.x; n < N; n += kTmPursuitThreads) acc += abs2(y[n]);
    const real_t<T> tot = block_sum_256<kTmPursuitWaves>(acc, shS);
    if (threadIdx.x == 0) *shE = tot;
    __syncthreads();
    return *shE;
}

// [ca, cb]: the c' of the atoms within dh of c, the only ones an atom at c overlaps
__device__ __forceinline__ void tm_pursuit_window(const TmGeom& g, int c, int& ca, int& cb) {
    const int C = (int)g.C;
    ca = c - g.dh > 0 ? (int)(c - g.dh) : 0;
    cb = c + g.dh < C - 1 ? (int)(c + g.dh) : C - 1;
}

// every tap of an atom at c lies inside the signal
__device__ __forceinline__ bool tm_pursuit_inside(const TmGeom& g, int c) {
    const long bj = g.s * c - g.Q;   // first sample of its taps
    return bj >= 0 && bj + g.S - 1 <= g.N - 1;
}

// acc + a conj(b) with the rounding of every product fixed: a * conj(b) as one rounded product and one fused
// multiply-add per part, then the sum.  The compiler's own contraction of a complex multiply-add depends on the
// surrounding code (which product it fuses changes the bits), and every caller of tm_pursuit_gram must form the same
// ones.  Which product is rounded is what both kernels had before they shared this sum, kept so that their results
// stay what they were: in the real part it is a.re b.re in c64 and a.im b.im in c128.
DCP_HD float  tm_madd_conj(float acc, float a, float b)    { return fmaf(a, b, acc); }
DCP_HD double tm_madd_conj(double acc, double a, double b) { return fma(a, b, acc); }
DCP_HD c64 tm_madd_conj(c64 acc, c64 a, c64 b) {
    return c64{acc.re + fmaf(a.im, b.im, a.re * b.re), acc.im + fmaf(a.im, b.re, -(a.re * b.im))};
}
DCP_HD c128 tm_madd_conj(c128 acc, c128 a, c128 b) {
    return c128{acc.re + fma(a.re, b.re, a.im * b.im), acc.im + fma(a.im, b.re, -(a.re * b.im))};
}

// G[(t, c), (tp, cp)] = A_(t,c) . A_(tp,cp)^H over the samples inside [0, N): Corr when atom (t, c) lies inside the
// signal (inside = tm_pursuit_inside(g, c), hoisted by the caller), else the explicit sum, over the g.Ch channels of
// D [T, Ch, S] (ch ascending, k ascending inside); an exact zero when the atoms do not overlap
template <class T>
__device__ __forceinline__ T tm_pursuit_gram(const T* __restrict__ D, const T* __restrict__ corr, const TmGeom& g, int t,
                                             int c, bool inside, int tp, int cp) {
    const long m = g.s * ((long)c - cp);   // sum_k D[t, k] conj(D[tp, k + m])
    if (m > g.S - 1 || m < -(g.S - 1)) return zero_of<T>();
    if (inside) return corr[((long)t * g.T + tp) * (2 * g.S - 1) + m + g.S - 1];
    const long bj = g.s * c - g.Q;
    long k0 = m < 0 ? -m : 0, k1 = m > 0 ? g.S - 1 - m : g.S - 1;
    if (k0 < -bj) k0 = -bj;
    if (k1 > g.N - 1 - bj) k1 = g.N - 1 - bj;
    T G = zero_of<T>();
    for (long ch = 0; ch < g.Ch; ++ch) {
        const long dt = (t * g.Ch + ch) * g.S, dp = (tp * g.Ch + ch) * g.S + m;
        for (long k = k0; k <= k1; ++k) G = tm_madd_conj(G, D[dt + k], D[dp + k]);
    }
    return G;
}

// grid: B workgroups of kTmPursuitThreads threads.  alpha0 [B, K] (K = T C < 2^31): read, and in the global tier
// updated in place; ws_tab [B, nseg]: the table of the global tier (unused in the LDS tier, whose dynamic LDS is
// tm_pursuit_lds_bytes(K)).  X [B, K] is written entirely.  *it_max (zero on entry) receives the largest step count.
template <class T, bool LDS>
__global__ void __launch_bounds__(kTmPursuitThreads) tm_pursuit_kernel(const T* __restrict__ Y, const T* __restrict__ D,
                                                                       const T* __restrict__ corr,
                                                                       const real_t<T>* __restrict__ rho2, T* alpha0,
                                                                       TmBest<T>* ws_tab, T* X, TmGeom g, long n_steps,
                                                                       real_t<T> tol, int positive,
                                                                       int* __restrict__ it_max) {
    typedef real_t<T> R;
    constexpr int NT = kTmPursuitThreads, NW = kTmPursuitWaves;
    extern __shared__ __attribute__((aligned(16))) char tm_smem[];
    __shared__ R shS[NW];
    __shared__ int shI[NW];
    __shared__ R shE;
    const int tid = threadIdx.x, wave = tid >> 6;
    const long b = blockIdx.x;
    const int C = (int)g.C, Tn = (int)g.T, K = Tn * C, nseg = (K + kTmPursuitSeg - 1) / kTmPursuitSeg;
    T* al;
    TmBest<T>* tab;
    if constexpr (LDS) {
        al = reinterpret_cast<T*>(tm_smem);
        tab = reinterpret_cast<TmBest<T>*>(tm_smem + (((size_t)K * sizeof(T) + 15) & ~size_t(15)));
        for (int i = tid; i < K; i += NT) al[i] = alpha0[b * K + i];
    } else {
        al = alpha0 + b * K;
        tab = ws_tab + b * nseg;
    }
    T* x = X + b * K;
    for (int i = tid; i < K; i += NT) x[i] = zero_of<T>();
    R E = tm_pursuit_ynorm2(Y + b * g.Ch * g.N, g.Ch * g.N, shS, &shE);
    for (int seg = wave; seg < nseg; seg += NW) tm_pursuit_segment(al, rho2, K, seg, positive, false, tab);
    __syncthreads();

    const bool use_tol = tol >= R(0);
    int steps = 0;
    for (long it = 0; it < n_steps; ++it) {
        if (use_tol && E <= tol) break;
        R bs;
        int bi;
        tm_pursuit_table_best(tab, nseg, shS, shI, bs, bi);
        if (!(bs > R(0))) break;
        // ---- take it (its alpha and rho2 came along in the table) ----
        const T a = div_real(tab[bi / kTmPursuitSeg].a, tab[bi / kTmPursuitSeg].r2);
        const int ts = bi / C, cs = bi - ts * C;
        E -= bs;
        ++steps;
        // ---- alpha -= a G over the atoms within dh of c* ----
        const bool inside = tm_pursuit_inside(g, cs);
        int ca, cb;
        tm_pursuit_window(g, cs, ca, cb);
        const int nc = cb - ca + 1, total = Tn * nc;
        const int dq = NT / nc, dr = NT - dq * nc;       // q += NT moves (t', c' - ca) by (dq, dr), with a carry
        int tp = tid / nc, off = tid - tp * nc;
        for (int q = tid; q < total; q += NT) {
            const int cp = ca + off;
            const int i = tp * C + cp;
            al[i] = fmsub(al[i], a, tm_pursuit_gram(D, corr, g, ts, cs, inside, tp, cp));
            tp += dq;
            off += dr;
            if (off >= nc) {
                off -= nc;
                ++tp;
            }
        }
        __syncthreads();
        if (tid == NT - 1) x[bi] = add(x[bi], a);        // (the last wave has the fewest segments to refresh)
        // ---- refresh the segments the update touched: template t' wrote [t' C + ca, t' C + cb] ----
        const int nsp = (nc + kTmPursuitSeg - 2) / kTmPursuitSeg + 1;   // the most segments a run of nc can touch
        for (int j = wave; j < Tn * nsp; j += NW) {
            const int tq = j / nsp, p = j - tq * nsp;
            const int f0 = (tq * C + ca) / kTmPursuitSeg, f1 = (tq * C + cb) / kTmPursuitSeg;
            // the previous template's last segment is refreshed as that template's
            const bool dup = p == 0 && tq > 0 && ((tq - 1) * C + cb) / kTmPursuitSeg == f0;
            if (f0 + p <= f1 && !dup) tm_pursuit_segment(al, rho2, K, f0 + p, positive, false, tab);
        }
        __syncthreads();
    }
    if (tid == 0 && steps > 0) atomicMax(it_max, steps);
}

// The prepare launches of the greedy coders: rho2 [K], the lag correlations corr [T, T, 2 S - 1], alpha0 = y A^H
// [B, K]; clears *it_dev.  D is [T, g.Ch, S] and y [B, g.Ch, N].  mc (the dcp_tm_mc_* entries, for every Ch, 1
// included) takes alpha0 from tm_mc_corr_kernel, else (g.Ch == 1) from tm_corr_store_kernel: the one place that chooses.
template <class T>
inline int tm_pursuit_prepare(dcp_handle* h, const T* Y, const T* D, const TmGeom& g, real_t<T>* rho2, T* corr,
                              T* alpha0, int* it_dev, bool mc) {
    hipStream_t st = h->stream;
    const long K = g.T * g.C;
    hipLaunchKernelGGL((tm_pursuit_rho2_kernel<T>), dim3(tm_grid(K)), dim3(256), 0, st, D, g, rho2, it_dev);
    DCP_LAUNCH_OK(h, hipGetLastError());
    hipLaunchKernelGGL((tm_lagcorr_kernel<T>), dim3(g.T * g.T), dim3(256), 0, st, D, g, corr);
    DCP_LAUNCH_OK(h, hipGetLastError());
    if (mc) return tm_mc_corr_pass<T>(h, Y, D, g, alpha0);
    {   // alpha0, the batch in slices of at most 65535 signals (the grid's z extent)
        ProfScope ps(h, DCP_PROF_XUPDATE);
        const long span = 255 * g.s + g.S;
        size_t bytes = (size_t)(g.S + span) * sizeof(T);
        const int lds_ok = bytes <= kTmLdsBytes;
        if (!lds_ok) bytes = 0;
        for (long b0 = 0; b0 < g.B; b0 += 65535) {
            TmGeom gs = g;
            gs.B = g.B - b0 < 65535 ? g.B - b0 : 65535;
            hipLaunchKernelGGL((tm_corr_store_kernel<T>), dim3((g.C + 255) / 256, g.T, gs.B), dim3(256), bytes, st,
                               Y + b0 * g.N, D, gs, lds_ok, alpha0 + b0 * K);
            DCP_LAUNCH_OK(h, hipGetLastError());
        }
    }
    return DCP_OK;
}

// One workgroup per signal on the chosen tier: KernLds with `bytes` of dynamic LDS (above 64 KiB the kernel's limit is
// raised first, once per instantiation and device, to `most`: what its largest problem asks for), else KernGlobal.
template <auto KernLds, auto KernGlobal, class... Args>
inline hipError_t tm_pursuit_launch(hipStream_t st, long B, bool lds, size_t bytes, size_t most, Args... args) {
    if (lds && bytes > 65536) {
        static DynLdsRaised raised;   // per instantiation
        std::atomic<bool>& done = raised.on_current_device();
        if (!done) {
            const hipError_t e = hipFuncSetAttribute(reinterpret_cast<const void*>(KernLds),
                                                     hipFuncAttributeMaxDynamicSharedMemorySize, (int)most);
            if (e != hipSuccess) return e;
            done = true;
        }
    }
    if (lds) hipLaunchKernelGGL(KernLds, dim3(B), dim3(kTmPursuitThreads), bytes, st, args...);
    else hipLaunchKernelGGL(KernGlobal, dim3(B), dim3(kTmPursuitThreads), bytes, st, args...);
    return hipGetLastError();
}

// Y [B, N], D [T, S] (mc: Y [B, Ch, N], D [T, Ch, S]) -> X [B, T, C]; *it_out = the largest number of steps a signal
// took.  Synchronises the stream.
template <class T>
inline int tm_pursuit_solve(dcp_handle* h, const T* Y, const T* D, T* X, const TmGeom& g, int64_t n_steps, double tol,
                            int positive, int* it_out, bool mc) {
    typedef real_t<T> R;
    hipStream_t st = h->stream;
    const long K = g.T * g.C, nseg = tm_pursuit_nseg(K);
    const bool lds = K <= tm_pursuit_lds_atoms<T>();
    R* rho2 = nullptr;
    T* corr = nullptr;     // lag correlations
    T* alpha0 = nullptr;   // y A^H; the global tier's alpha
    TmBest<T>* tab = nullptr;   // the global tier's table
    int* it_dev = nullptr;
    DCP_TRY(ws_lay_out(h, [&](WsLayout& a) {
        a.take(rho2, K);
        a.take(corr, g.T * g.T * (2 * g.S - 1));
        a.take(alpha0, g.B * K);
        a.take(tab, lds ? 0 : g.B * nseg);
        a.take(it_dev, 4);
    }));
    DCP_TRY(tm_pursuit_prepare<T>(h, Y, D, g, rho2, corr, alpha0, it_dev, mc));
    const R t = tol >= 0.0 ? (R)tol : R(-1);
    DCP_LAUNCH_OK(h, (tm_pursuit_launch<&tm_pursuit_kernel<T, true>, &tm_pursuit_kernel<T, false>>(
                         st, g.B, lds, lds ? tm_pursuit_lds_bytes<T>(K) : 0,
                         tm_pursuit_lds_bytes<T>(tm_pursuit_lds_atoms<T>()), Y, D, (const T*)corr, (const R*)rho2, alpha0,
                         tab, X, g, (long)n_steps, t, positive, it_dev)));
    return read_scalar(h, (const int*)it_dev, it_out);
}

// dcp_tm_pursuit_* and dcp_tm_mc_pursuit_*
template <class T>
inline int tm_pursuit_api(dcp_handle* h, const T* Y, const T* D, T* X, const TmShape& sh, int64_t n_steps, double tol,
                          int positive, int* it_out) {
    TmGeom g;
    DCP_TRY(tm_geom_api(h, sh, g));
    if (!Y || !D || !X || !it_out) return fail(h, DCP_ERR_INVALID, "null pointer");
    const int64_t K = (int64_t)g.T * g.C;
    if (K > 0x7fffff00LL) return fail(h, DCP_ERR_INVALID, "pursuit: T C exceeds 2^31 - 257");
    if (n_steps < 1 || n_steps > K) return fail(h, DCP_ERR_INVALID, "pursuit: n_steps must be in [1, T C]");
    if (tol != tol) return fail(h, DCP_ERR_INVALID, "pursuit: tol is NaN");
    if (positive && scalar_traits<T>::is_complex)
        return fail(h, DCP_ERR_INVALID, "pursuit: positive needs a real dtype");
    return tm_pursuit_solve<T>(h, Y, D, X, g, n_steps, tol, positive, it_out, sh.mc);
}

}  // namespace dcp
