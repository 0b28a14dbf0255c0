// Multichannel templates for the greedy coders (template_matching.pursuit / orthogonal_pursuit / predict with a 3-D D,
// dcp_tm_mc_*): the correlation pass and predict.  Included from template_impl.hpp before template_pursuit.hpp, whose
// prepare step calls tm_mc_corr_pass.
//
// Model: y[b, ch, n] ~ sum_(t, c) x[b, t, c] D[t, ch, n - s c + Q]: the atom of (t, c) is the spatio-temporal waveform
// A[(t, c), (ch, n)] = D[t, ch, n - s c + Q], one coefficient for all Ch channels.  The geometry (C, Q, dh, the flat
// index t C + c) is that of one channel.  The step kernels are in Gram form and read y only through
//   alpha0[b, t, c]  = sum_ch sum_k y[b, ch, s c - Q + k] conj(D[t, ch, k])
//   rho2[t, c]       = sum_ch sum_k |D[t, ch, k]|^2                         over the taps inside [0, N)
//   Corr[t, t', m]   = sum_ch sum_k D[t, ch, k] conj(D[t', ch, k + m])
// and |y_b|^2 over the Ch N samples of a signal, so each gains a sum over the channels (TmGeom::Ch) and nothing else
// in a step changes.  Every sum runs ch ascending, k ascending inside.  rho2 and Corr come from the kernels every
// coder uses (tm_pursuit_rho2_kernel, tm_lagcorr_kernel: their channel loop runs once at Ch = 1); alpha0 is the kernel
// here, for every Ch the dcp_tm_mc_* entries are given, 1 included.  It is not tm_corr_store_kernel with a channel
// loop: in the complex dtypes the two fuse different products of the multiply-add (tm_mc_madd below against madd), so
// their bits differ and the entry point decides which one runs.
//
// tm_mc_corr_kernel (alpha0, the dominant cost: 2 B T C Ch S flop).  A 256-thread workgroup owns 256 consecutive c of
// one signal and a block of TB templates; a thread holds TB accumulators.  The channels go in passes of CP: a pass
// stages the windows of CP channels of y in LDS (span 255 s + S samples each, zeros outside [0, N)), then every thread
// walks ch and k and reads a sample from LDS ONCE for all TB templates.  The taps are read from D with indices that
// are the same in the whole workgroup (template block, channel, k), so they are wave-uniform operands of the
// multiply-adds and cost no LDS read: ds_read_b32 delivers 128 B/clk/CU, a quarter of the fp32 multiply-add rate, which
// bounds a kernel with one LDS read per multiply-add (the one-template pass) and is removed by the template block.
// The sum of a coefficient is tm_mc_madd over ch ascending, k = 0 .. S - 1 ascending (a sample outside the signal is an
// exact zero: acc + 0 d = acc), whatever TB, CP, the template's place in its block, or the batch.  A ragged last
// template block computes its missing templates as copies of the last one and does not store them; the last channel
// pass is shorter; c >= C is computed on zeros or stale LDS inside the staged image and not stored.  CP = 0 (one
// channel's window does not fit the LDS budget): the same loop reads y from global memory, guarded.
#pragma once

namespace dcp {

constexpr int kTmMcMaxChannelsPerPass = 8;   // more adds LDS, not reuse: a pass's barrier is already amortised over 8 S
constexpr int kTmMcPredictChannels = 4;      // channels a predict workgroup accumulates per staged coefficient tile

// templates per thread of tm_mc_corr_kernel: 8 accumulator registers' worth in the 4-byte dtypes
template <class T>
constexpr int tm_mc_template_block() {
    return scalar_traits<T>::is_complex ? (sizeof(real_t<T>) == 4 ? 4 : 2) : (sizeof(T) == 4 ? 8 : 4);
}

// channels staged per pass (0: no LDS)
template <class T>
inline int tm_mc_channels_per_pass(int64_t S, int64_t stride) {
    if (S < 1 || stride < 1 || S > 0x7fffffffLL || stride > 0x7fffffffLL) return 0;
    const int64_t span = 255 * stride + S;
    const int64_t fit = (int64_t)(kTmLdsBytes / sizeof(T)) / span;
    return (int)(fit < kTmMcMaxChannelsPerPass ? fit : kTmMcMaxChannelsPerPass);
}

// acc + y conj(d), the one spelling of the correlation pass: every product fused, the real-part product first
DCP_HD float  tm_mc_madd(float acc, float y, float d)    { return fmaf(y, d, acc); }
DCP_HD double tm_mc_madd(double acc, double y, double d) { return fma(y, d, acc); }
DCP_HD c64 tm_mc_madd(c64 acc, c64 y, c64 d) {
    return c64{fmaf(y.im, d.im, fmaf(y.re, d.re, acc.re)), fmaf(-y.re, d.im, fmaf(y.im, d.re, acc.im))};
}
DCP_HD c128 tm_mc_madd(c128 acc, c128 y, c128 d) {
    return c128{fma(y.im, d.im, fma(y.re, d.re, acc.re)), fma(-y.re, d.im, fma(y.im, d.re, acc.im))};
}

// The accumulation loop of the correlation kernels, for the workgroup of tm_mc_corr_kernel's grid: acc[j] = the sum of
// coefficient (t0 + j, c0 + tid) over the g.Ch channels and g.S taps, the samples taken from ld(ch, n), 0 <= n < g.N
// (y [Ch, N] of a signal there; the Gram-form LASSO step of template_mc_lasso.hpp runs the same loop on the scaled
// iterate).  The whole workgroup calls it (the staging has barriers).
template <class T, int TB, bool LDS, class Load>
__device__ __forceinline__ void tm_mc_corr_accumulate(const Load& ld, const T* __restrict__ D, const TmGeom& g, int CP,
                                                      long t0, T (&acc)[TB]) {
    extern __shared__ __attribute__((aligned(16))) char tm_smem[];
    T* sY = reinterpret_cast<T*>(tm_smem);
    const int tid = threadIdx.x;
    const long c0 = (long)blockIdx.x * 256;
    const long span = 255 * g.s + g.S;
    const long nlo = g.s * c0 - g.Q;   // the sample of sY[0]; this thread's taps start at sY[off]
    const long off = g.s * tid;
    const T* Dt[TB];                   // workgroup-uniform: the taps are scalar operands
#pragma unroll
    for (int j = 0; j < TB; ++j) Dt[j] = D + (t0 + j < g.T ? t0 + j : g.T - 1) * g.Ch * g.S;
#pragma unroll
    for (int j = 0; j < TB; ++j) acc[j] = zero_of<T>();
    const long step = LDS ? CP : g.Ch;
    for (long p0 = 0; p0 < g.Ch; p0 += step) {
        const long np = g.Ch - p0 < step ? g.Ch - p0 : step;
        if constexpr (LDS) {
            __syncthreads();
            for (long q = 0; q < np; ++q) {
                for (long m = tid; m < span; m += 256) {
                    const long n = nlo + m;
                    sY[q * span + m] = (n >= 0 && n < g.N) ? ld(p0 + q, n) : zero_of<T>();
                }
            }
            __syncthreads();
        }
        for (long q = 0; q < np; ++q) {
            const long dch = (p0 + q) * g.S;
            const T* w = sY + q * span + off;
#pragma unroll 8
            for (long k = 0; k < g.S; ++k) {
                T v;
                if constexpr (LDS) {
                    v = w[k];
                } else {
                    const long n = nlo + off + k;
                    v = (n >= 0 && n < g.N) ? ld(p0 + q, n) : zero_of<T>();
                }
#pragma unroll
                for (int j = 0; j < TB; ++j) acc[j] = tm_mc_madd(acc[j], v, Dt[j][dch + k]);
            }
        }
    }
}

// sample n of channel ch of one signal y [Ch, N]
template <class T>
struct TmMcSignal {
    const T* yb;
    long N;
    __device__ __forceinline__ T operator()(long ch, long n) const { return yb[ch * N + n]; }
};

// grid (ceil(C / 256), ceil(T / TB), B <= 65535); dynamic LDS CP (255 s + S) sizeof(T) when LDS.  y [B, Ch, N],
// D [T, Ch, S] -> alpha0 [B, T, C]
template <class T, int TB, bool LDS>
__global__ void __launch_bounds__(256) tm_mc_corr_kernel(const T* __restrict__ y, const T* __restrict__ D, TmGeom g,
                                                         int CP, T* __restrict__ alpha0) {
    const long b = blockIdx.z, t0 = (long)blockIdx.y * TB;
    const long c = (long)blockIdx.x * 256 + threadIdx.x;
    T acc[TB];
    tm_mc_corr_accumulate<T, TB, LDS>(TmMcSignal<T>{y + b * g.Ch * g.N, g.N}, D, g, CP, t0, acc);
    if (c >= g.C) return;
#pragma unroll
    for (int j = 0; j < TB; ++j)
        if (t0 + j < g.T) alpha0[(b * g.T + t0 + j) * g.C + c] = acc[j];
}

// alpha0 [B, T C] of the dcp_tm_mc_* coders, the batch in slices of at most 65535 signals (the grid's z extent).  With
// dcp_profile_* on, the pass is timed under DCP_PROF_XUPDATE (as the one-channel pass is).
template <class T>
inline int tm_mc_corr_pass(dcp_handle* h, const T* Y, const T* D, const TmGeom& g, T* alpha0) {
    hipStream_t st = h->stream;
    constexpr int TB = tm_mc_template_block<T>();
    const long K = g.T * g.C;
    int CP = tm_mc_channels_per_pass<T>(g.S, g.s);
    if (CP > g.Ch) CP = (int)g.Ch;
    const size_t bytes = (size_t)CP * (size_t)(255 * g.s + g.S) * sizeof(T);
    ProfScope ps(h, DCP_PROF_XUPDATE);
    for (long b0 = 0; b0 < g.B; b0 += 65535) {
        const long nb = g.B - b0 < 65535 ? g.B - b0 : 65535;
        const dim3 grid((g.C + 255) / 256, (g.T + TB - 1) / TB, nb);
        const T* ys = Y + b0 * g.Ch * g.N;
        T* as = alpha0 + b0 * K;
        if (CP > 0) hipLaunchKernelGGL((tm_mc_corr_kernel<T, TB, true>), grid, dim3(256), bytes, st, ys, D, g, CP, as);
        else hipLaunchKernelGGL((tm_mc_corr_kernel<T, TB, false>), grid, dim3(256), 0, st, ys, D, g, 0, as);
        DCP_LAUNCH_OK(h, hipGetLastError());
    }
    return DCP_OK;
}

// out[b, ch, n] = sum_t sum_c x[b, t, c] D[t, ch, n - s c + Q]: tm_residual_kernel's staging, the coefficients of a tile
// staged once per template and read once for the kTmMcPredictChannels channels of the workgroup (a ragged last group
// computes copies of the last channel and does not store them).  grid (ceil(N / 256), ceil(Ch / 4), B <= 65535).
template <class T, bool LDS>
__global__ void __launch_bounds__(256) tm_mc_predict_kernel(const T* __restrict__ x, const T* __restrict__ D, TmGeom g,
                                                            T* __restrict__ out) {
    constexpr int CB = kTmMcPredictChannels;
    extern __shared__ __attribute__((aligned(16))) char tm_smem[];
    T* sD = reinterpret_cast<T*>(tm_smem);   // [CB][S]
    T* sU = sD + CB * g.S;
    const long b = blockIdx.z, ch0 = (long)blockIdx.y * CB;
    const long n0 = (long)blockIdx.x * 256, n = n0 + threadIdx.x;
    const long n1 = (n0 + 255 < g.N - 1) ? n0 + 255 : g.N - 1;
    const long clo = g.c_first(n0), chi = g.c_last(n1);
    long chj[CB];
#pragma unroll
    for (int j = 0; j < CB; ++j) chj[j] = ch0 + j < g.Ch ? ch0 + j : g.Ch - 1;
    T acc[CB];
#pragma unroll
    for (int j = 0; j < CB; ++j) acc[j] = zero_of<T>();
    for (long t = 0; t < g.T; ++t) {
        const T* xrow = x + (b * g.T + t) * g.C;
        if constexpr (LDS) {
            __syncthreads();
#pragma unroll
            for (int j = 0; j < CB; ++j)
                for (long k = threadIdx.x; k < g.S; k += 256) sD[j * g.S + k] = D[(t * g.Ch + chj[j]) * g.S + k];
            for (long c = clo + threadIdx.x; c <= chi; c += 256) sU[c - clo] = xrow[c];
            __syncthreads();
        }
        if (n < g.N) {
            const long c1 = g.c_last(n);
            for (long c = g.c_first(n); c <= c1; ++c) {
                const long k = n - g.s * c + g.Q;
                const T u = LDS ? sU[c - clo] : xrow[c];
#pragma unroll
                for (int j = 0; j < CB; ++j)
                    acc[j] = madd(acc[j], u, LDS ? sD[j * g.S + k] : D[(t * g.Ch + chj[j]) * g.S + k]);
            }
        }
    }
    if (n >= g.N) return;
#pragma unroll
    for (int j = 0; j < CB; ++j)
        if (ch0 + j < g.Ch) out[(b * g.Ch + ch0 + j) * g.N + n] = acc[j];
}

template <class T>
inline int tm_mc_predict(dcp_handle* h, const T* X, const T* D, const TmGeom& g, T* out) {
    constexpr int CB = kTmMcPredictChannels;
    const long span = (255 + g.S - 1) / g.s + 2;
    const size_t bytes = (size_t)(CB * g.S + span) * sizeof(T);
    const bool lds = bytes <= kTmLdsBytes;
    for (long b0 = 0; b0 < g.B; b0 += 65535) {
        const long nb = g.B - b0 < 65535 ? g.B - b0 : 65535;
        const dim3 grid((g.N + 255) / 256, (g.Ch + CB - 1) / CB, nb);
        const T* xs = X + b0 * g.T * g.C;
        T* os = out + b0 * g.Ch * g.N;
        if (lds) hipLaunchKernelGGL((tm_mc_predict_kernel<T, true>), grid, dim3(256), bytes, h->stream, xs, D, g, os);
        else hipLaunchKernelGGL((tm_mc_predict_kernel<T, false>), grid, dim3(256), 0, h->stream, xs, D, g, os);
        DCP_LAUNCH_OK(h, hipGetLastError());
    }
    return DCP_OK;
}

template <class T>
inline int tm_mc_predict_api(dcp_handle* h, const T* X, const T* D, const TmShape& sh, T* out) {
    TmGeom g;
    DCP_TRY(tm_geom_api(h, sh, g));
    if (!X || !D || !out) return fail(h, DCP_ERR_INVALID, "null pointer");
    return tm_mc_predict<T>(h, X, D, g, out);
}

}  // namespace dcp
