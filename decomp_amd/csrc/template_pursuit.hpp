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
// (tm_corr_store_kernel: the correlation pass of the LASSO with a store-only epilogue).  Then tm_pursuit_kernel: one
// 1024-thread workgroup (16 waves) per signal, the steps of a signal sequential, the signals concurrent; no waiting
// between workgroups, no float atomics (one integer max per signal for the step count), the loop bounded by n_steps.
// A step is a chain of dependent latencies, not of work, hence the wide workgroup: every phase is one pass.
//   arg-max     never rescans alpha.  A table holds, for every SEGMENT (a fixed run of kTmPursuitSeg = 64 flat
//               indices, one per lane), its best atom: (score, index) and that atom's alpha and rho2.  A step reduces
//               the table (each thread its entries, a 6-step butterfly per wave, the 16 wave results through LDS),
//               updates T (2 dh + 1) correlations and re-reduces only the segments those lie in: at most
//               T (ceil(2 dh / 64) + 1).  Ties go to the lower index at every level (lane, wave, segment, table):
//               the comparison is (score, -index) throughout.
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
#pragma once

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

// (s, i) <- the better of (s, i) and (s2, i2): the larger score, the lower index on a tie
template <class R>
__device__ __forceinline__ void tm_pursuit_better(R& s, int& i, R s2, int i2) {
    if (s2 > s || (s2 == s && i2 < i)) {
        s = s2;
        i = i2;
    }
}

// the best (score, index) over the wave, the same in every lane (the order is total: a butterfly is enough)
template <class R>
__device__ __forceinline__ void tm_pursuit_wave_best(R& s, int& i) {
#pragma unroll
    for (int m = 32; m >= 1; m >>= 1) {
        const R s2 = lane_xor(s, m);
        const int i2 = lane_xor(i, m);
        tm_pursuit_better(s, i, s2, i2);
    }
}

// tab[seg] <- the best atom of flat indices [64 seg, 64 seg + 64) & [0, K); the whole wave calls it
template <class T>
__device__ __forceinline__ void tm_pursuit_segment(const T* al, const real_t<T>* __restrict__ rho2, int K, int seg,
                                                   int positive, TmBest<T>* tab) {
    typedef real_t<T> R;
    const int lane = threadIdx.x & 63;
    const int i = seg * kTmPursuitSeg + lane;
    const int ic = i < K ? i : K - 1;
    const T a = al[ic];
    const R r2 = rho2[ic];
    R sc = tm_pursuit_score(a, r2, positive);
    if (i >= K) sc = R(-1);
    int bi = i;
    tm_pursuit_wave_best(sc, bi);
    const int wl = bi - seg * kTmPursuitSeg;   // the winner's lane
    const T wa = lane_get(a, wl);
    const R wr = lane_get(r2, wl);
    if (lane == 0) tab[seg] = TmBest<T>{wa, sc, wr, bi};
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
    const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
    const long b = blockIdx.x;
    const int C = (int)g.C, Tn = (int)g.T, K = Tn * C, nseg = (K + kTmPursuitSeg - 1) / kTmPursuitSeg;
    const long W = 2 * g.S - 1;
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
    R E;
    {   // |y|^2, a fixed-order sum
        R acc = 0;
        for (long n = tid; n < g.N; n += NT) acc += abs2(Y[b * g.N + n]);
        const R tot = block_sum_256<NW>(acc, shS);
        if (tid == 0) shE = tot;
        __syncthreads();
        E = shE;
    }
    for (int seg = wave; seg < nseg; seg += NW) tm_pursuit_segment(al, rho2, K, seg, positive, tab);
    __syncthreads();

    const bool use_tol = tol >= R(0);
    int steps = 0;
    for (long it = 0; it < n_steps; ++it) {
        if (use_tol && E <= tol) break;
        // ---- the table's best atom ----
        R bs = R(-1);
        int bi = 0x7fffffff;
        for (int j = tid; j < nseg; j += NT) tm_pursuit_better(bs, bi, tab[j].s, tab[j].i);
        tm_pursuit_wave_best(bs, bi);
        if (lane == 0) {
            shS[wave] = bs;
            shI[wave] = bi;
        }
        __syncthreads();
        bs = shS[0];
        bi = shI[0];
#pragma unroll
        for (int w = 1; w < NW; ++w) tm_pursuit_better(bs, bi, shS[w], shI[w]);
        if (!(bs > R(0))) break;
        // ---- take it (its alpha and rho2 came along in the table) ----
        const T a = div_real(tab[bi / kTmPursuitSeg].a, tab[bi / kTmPursuitSeg].r2);
        const int ts = bi / C, cs = bi - ts * C;
        E -= bs;
        ++steps;
        // ---- alpha -= a G over the atoms within dh of c* ----
        const long bj = g.s * cs - g.Q;                  // first sample of the taken atom's taps
        const bool inside = bj >= 0 && bj + g.S - 1 <= g.N - 1;
        const int ca = cs - g.dh > 0 ? (int)(cs - g.dh) : 0;
        const int cb = cs + g.dh < C - 1 ? (int)(cs + g.dh) : C - 1;
        const int nc = cb - ca + 1, total = Tn * nc;
        const int dq = NT / nc, dr = NT - dq * nc;       // q += NT moves (t', c' - ca) by (dq, dr), with a carry
        int tp = tid / nc, off = tid - tp * nc;
        for (int q = tid; q < total; q += NT) {
            const int cp = ca + off;
            const long m = g.s * (cs - cp);              // G = sum_k D[t*, k] conj(D[t', k + m]) over n inside
            T G;
            if (inside) {
                G = corr[((long)ts * Tn + tp) * W + m + g.S - 1];
            } else {
                long k0 = m < 0 ? -m : 0, k1 = m > 0 ? g.S - 1 - m : g.S - 1;
                if (k0 < -bj) k0 = -bj;
                if (k1 > g.N - 1 - bj) k1 = g.N - 1 - bj;
                G = zero_of<T>();
                for (long k = k0; k <= k1; ++k) G = madd(G, D[ts * g.S + k], conj_of(D[tp * g.S + k + m]));
            }
            const int i = tp * C + cp;
            al[i] = fmsub(al[i], a, G);
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
            if (f0 + p <= f1 && !dup) tm_pursuit_segment(al, rho2, K, f0 + p, positive, tab);
        }
        __syncthreads();
    }
    if (tid == 0 && steps > 0) atomicMax(it_max, steps);
}

// The prepare launches of the greedy coders: rho2 [K], the lag correlations corr [T, T, 2 S - 1], alpha0 = y A^H
// [B, K]; clears *it_dev
template <class T>
inline int tm_pursuit_prepare(dcp_handle* h, const T* Y, const T* D, const TmGeom& g, real_t<T>* rho2, T* corr,
                              T* alpha0, int* it_dev) {
    hipStream_t st = h->stream;
    const long K = g.T * g.C;
    hipLaunchKernelGGL((tm_pursuit_rho2_kernel<T>), dim3(tm_grid(K)), dim3(256), 0, st, D, g, rho2, it_dev);
    DCP_LAUNCH_OK(h, hipGetLastError());
    hipLaunchKernelGGL((tm_lagcorr_kernel<T>), dim3(g.T * g.T), dim3(256), 0, st, D, g, corr);
    DCP_LAUNCH_OK(h, hipGetLastError());
    {   // alpha0, the batch in slices of at most 65535 signals (the grid's z extent)
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

// Y [B, N], D [T, S] -> X [B, T, C]; *it_out = the largest number of steps a signal took.  Synchronises the stream.
template <class T>
inline int tm_pursuit_solve(dcp_handle* h, const T* Y, const T* D, T* X, const TmGeom& g, int64_t n_steps, double tol,
                            int positive, int* it_out) {
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
    DCP_TRY(tm_pursuit_prepare<T>(h, Y, D, g, rho2, corr, alpha0, it_dev));
    const R t = tol >= 0.0 ? (R)tol : R(-1);
    if (lds) {
        const size_t bytes = tm_pursuit_lds_bytes<T>(K);
        if (bytes > 65536) {
            static DynLdsRaised raised;   // per instantiation
            std::atomic<bool>& done = raised.on_current_device();
            if (!done) {
                DCP_LAUNCH_OK(h, hipFuncSetAttribute(reinterpret_cast<const void*>(&tm_pursuit_kernel<T, true>),
                                                     hipFuncAttributeMaxDynamicSharedMemorySize,
                                                     (int)tm_pursuit_lds_bytes<T>(tm_pursuit_lds_atoms<T>())));
                done = true;
            }
        }
        hipLaunchKernelGGL((tm_pursuit_kernel<T, true>), dim3(g.B), dim3(kTmPursuitThreads), bytes, st, Y, D,
                           (const T*)corr, (const R*)rho2, alpha0, tab, X, g, (long)n_steps, t, positive, it_dev);
    } else {
        hipLaunchKernelGGL((tm_pursuit_kernel<T, false>), dim3(g.B), dim3(kTmPursuitThreads), 0, st, Y, D,
                           (const T*)corr, (const R*)rho2, alpha0, tab, X, g, (long)n_steps, t, positive, it_dev);
    }
    DCP_LAUNCH_OK(h, hipGetLastError());
    return read_scalar(h, (const int*)it_dev, it_out);
}

template <class T>
inline int tm_pursuit_api(dcp_handle* h, const T* Y, const T* D, T* X, const TmGeom& g, int64_t n_steps, double tol,
                          int positive, int* it_out) {
    if (!Y || !D || !X || !it_out) return fail(h, DCP_ERR_INVALID, "null pointer");
    const int64_t K = (int64_t)g.T * g.C;
    if (K > 0x7fffff00LL) return fail(h, DCP_ERR_INVALID, "pursuit: T C exceeds 2^31 - 257");
    if (n_steps < 1 || n_steps > K) return fail(h, DCP_ERR_INVALID, "pursuit: n_steps must be in [1, T C]");
    if (tol != tol) return fail(h, DCP_ERR_INVALID, "pursuit: tol is NaN");
    if (positive && scalar_traits<T>::is_complex)
        return fail(h, DCP_ERR_INVALID, "pursuit: positive needs a real dtype");
    return tm_pursuit_solve<T>(h, Y, D, X, g, n_steps, tol, positive, it_out);
}

}  // namespace dcp
