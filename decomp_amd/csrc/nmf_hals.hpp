// HALS for NMF with the squared loss (hierarchical alternating least squares, i.e. exact block coordinate
// descent on the columns of x and the atoms of D; Cichocki & Phan 2009, Gillis & Glineur 2012).
//
// The one new hot-path kernel is the non-negative coordinate sweep
//
//   sweep(V, C, G):  for k = 0 .. K-1 in order, with the current V (columns < k already updated)
//     if G[k,k] > 0:  V[:,k] = max(0, V[:,k] - (V G[:,k] - C[:,k]) / G[k,k])      (else V[:,k] unchanged)
//
// over R independent vectors V [R, K] (rows), C [R, K], symmetric G [K, K].  Two layouts of V and C:
// vector-major V[r*ld + k] (x and Y D^T) and coordinate-major V[k*ld + r] (D [K, F] and x^T Y, whose
// columns are the vectors: D is swept without a transpose in memory).
//
// One wave owns MT x 16 vectors and runs the whole sweep in one launch (the vectors are independent: no
// cross-wave traffic, no atomics, bitwise deterministic).  Its tile of V sits in LDS, [16 MT][Kp + 4]
// (Kp = K rounded up to 64; a row stride of 4 x odd words puts the 64 lanes of every access on 64
// distinct banks).  K is walked in blocks of 16 coordinates k0 .. k0+15:
//   T = V_cur G[:, blk]        on the matrix pipe (v_mfma_f32_16x16x4_f32 / v_mfma_f64_16x16x4_f64):
//                              A = 16 rows of the tile (LDS), B = G[:, blk] (L2); columns >= k0 still
//                              hold their old values, so T is V G[:,k] before this block's changes
//   16 sequential steps        each lane holds ONE coordinate of the block (the MFMA's C column) for
//                              4 of the rows (its C registers).  At step j the lane of coordinate j
//                              takes its new value v_j; dv_j = v_j - v_old is broadcast over the 16
//                              lanes of its rows (ds_swizzle) and every lane corrects its T by
//                              dv_j G[k0+j, k0+col] -- the in-block sum over i < j, pushed forward.
// Cost per vector: 2 K^2 flop on the matrix pipe, 16 K broadcast-and-FMA steps on the VALU.
//
// K too large for a 64 KiB tile: the same kernel keeps the tile in V_out itself (global memory, L1/L2).
#pragma once
#include <hip/hip_runtime.h>

#include "gemm_mfma_f64.hpp"   // f32x4 / f64x4
#include "kernels_small.hpp"

namespace dcp {

template <class T> struct hals_acc;
template <> struct hals_acc<float> {
    typedef f32x4 type;
    // C/D map of v_mfma_f32_16x16x4_f32: col = lane & 15, row = 4 (lane >> 4) + reg
    static __device__ __forceinline__ int row(int grp, int reg) { return 4 * grp + reg; }
    static __device__ __forceinline__ f32x4 mfma(float a, float b, f32x4 c) {
        return __builtin_amdgcn_mfma_f32_16x16x4f32(a, b, c, 0, 0, 0);
    }
};
template <> struct hals_acc<double> {
    typedef f64x4 type;
    // C/D map of v_mfma_f64_16x16x4_f64: col = lane & 15, row = (lane >> 4) + 4 reg
    static __device__ __forceinline__ int row(int grp, int reg) { return grp + 4 * reg; }
    static __device__ __forceinline__ f64x4 mfma(double a, double b, f64x4 c) {
        return __builtin_amdgcn_mfma_f64_16x16x4f64(a, b, c, 0, 0, 0);
    }
};

// v of lane (lane & ~15) | J, for every lane: ds_swizzle bit mode, and_mask 0x10 keeps the 16-lane group
// (bit 5 is kept by the 32-lane swizzle itself), or_mask J picks the lane.
template <int J>
__device__ __forceinline__ float bcast16(float v) {
    return __int_as_float(__builtin_amdgcn_ds_swizzle(__float_as_int(v), 0x10 | (J << 5)));
}
template <int J>
__device__ __forceinline__ double bcast16(double v) {
    const long long b = __double_as_longlong(v);
    const int lo = __builtin_amdgcn_ds_swizzle((int)(b & 0xffffffffLL), 0x10 | (J << 5));
    const int hi = __builtin_amdgcn_ds_swizzle((int)(b >> 32), 0x10 | (J << 5));
    return __longlong_as_double(((long long)hi << 32) | (unsigned int)lo);
}

// v where keep, else +0, by a bit mask: a select of a loaded value lets the compiler sink the load into a branch
// of its own (one branch and one wait for memory per load); the mask keeps the tile loads unconditional.
__device__ __forceinline__ float hals_mask(float v, bool keep) {
    return __int_as_float(__float_as_int(v) & -(int)keep);
}
__device__ __forceinline__ double hals_mask(double v, bool keep) {
    return __longlong_as_double(__double_as_longlong(v) & -(long long)keep);
}

constexpr int kHalsLdsBytes = 64 * 1024;   // the default dynamic LDS limit: two tiles per CU at least

__host__ __device__ inline int hals_kpad(int K) { return (K + 63) & ~63; }
template <class T>
inline size_t hals_lds_bytes(int K, int MT) { return (size_t)16 * MT * (hals_kpad(K) + 4) * sizeof(T); }

// steps J .. 15 of a block (J compile-time: the broadcast source and G[k0+J, .] are fixed per step)
template <class T, int MT, int J>
__device__ __forceinline__ void hals_steps(T (&t)[MT][4], const T (&vo)[MT][4], const T (&c)[MT][4],
                                           T (&vn)[MT][4], const T (&gk)[16], T inv, bool act, int col,
                                           int left) {
    if constexpr (J < 16) {
        if (J >= left) return;   // the last block of a K that is not a multiple of 16 (uniform)
#pragma unroll
        for (int m = 0; m < MT; ++m)
#pragma unroll
            for (int r = 0; r < 4; ++r) {
                const T u = vo[m][r] - (t[m][r] - c[m][r]) * inv;
                const T cand = act ? (u < T(0) ? T(0) : u) : vo[m][r];   // a NaN passes, as np.maximum
                const T dj = bcast16<J>(cand - vo[m][r]);
                t[m][r] += dj * gk[J];
                if (col == J) vn[m][r] = cand;
            }
        hals_steps<T, MT, J + 1>(t, vo, c, vn, gk, inv, act, col, left);
    }
}

// grid: one 64-thread workgroup per 16 MT vectors.  IN_LDS: the tile lives in dynamic LDS
// (hals_lds_bytes), else in V_out.  V_in may equal V_out.
template <class T, int MT, bool CM, bool IN_LDS>
__global__ void __launch_bounds__(64) nn_cd_sweep_kernel(const T* V_in, T* V_out, long ldv,
                                                         const T* __restrict__ C, long ldc,
                                                         const T* __restrict__ G, long ldg, int R, int K) {
    typedef hals_acc<T> A;
    typedef typename A::type acc_t;
    extern __shared__ __attribute__((aligned(16))) unsigned char hals_lds[];
    T* tile = reinterpret_cast<T*>(hals_lds);
    const int lane = threadIdx.x, col = lane & 15, grp = lane >> 4;
    const int Kp = hals_kpad(K), ldw = Kp + 4;
    const long r0 = (long)blockIdx.x * 16 * MT;
    auto vidx = [&](long r, long k) -> long { return CM ? k * ldv + r : r * ldv + k; };
    // the tile: local row rr (0 .. 16 MT - 1), coordinate k (0 .. Kp - 1); zero outside [R, K]
    auto wget = [&](int rr, int k) -> T {
        if constexpr (IN_LDS) return tile[rr * ldw + k];
        else {
            const long r = r0 + rr;
            return hals_mask(V_out[vidx(r < R ? r : R - 1, k < K ? k : K - 1)], r < R && k < K);
        }
    };
    auto wput = [&](int rr, int k, T v) {
        if constexpr (IN_LDS) tile[rr * ldw + k] = v;
        else if (r0 + rr < R) V_out[vidx(r0 + rr, k)] = v;
    };

    // ---- load the tile (rows >= R and coordinates >= K are zero: they contribute nothing) ----
    if constexpr (IN_LDS) {
        // element q of round i: vector-major, row i / (Kp/64) of the tile, 64 consecutive coordinates;
        // coordinate-major, 16 consecutive vectors x 4 coordinates.  Eight loads in flight per wait.
        const int per = CM ? Kp / 4 : Kp / 64;
        const int rounds = CM ? MT * per : 16 * MT * per;   // a multiple of 8
        for (int i0 = 0; i0 < rounds; i0 += 8) {
            T v[8];
            int rq[8], kq[8];
#pragma unroll
            for (int q = 0; q < 8; ++q) {
                const int i = i0 + q, a = i / per, b = i - a * per;
                rq[q] = CM ? 16 * a + col : a;
                kq[q] = CM ? 4 * b + grp : 64 * b + lane;
                const long r = r0 + rq[q];
                v[q] = hals_mask(V_in[vidx(r < R ? r : R - 1, kq[q] < K ? kq[q] : K - 1)], r < R && kq[q] < K);
            }
#pragma unroll
            for (int q = 0; q < 8; ++q)
                tile[rq[q] * ldw + kq[q]] = v[q];
        }
    } else if (V_in != V_out) {
        for (int m = 0; m < MT; ++m)
            for (int k = grp; k < K; k += 4) {
                const long r = r0 + 16 * m + col;
                if (r < R) V_out[vidx(r, k)] = V_in[vidx(r, k)];
            }
    }
    __syncthreads();

    for (int k0 = 0; k0 < K; k0 += 16) {
        const int kc = k0 + col;          // this lane's coordinate of the block (B / C column)
        const bool kc_ok = kc < K;
        const int kcl = kc_ok ? kc : K - 1;   // loads from clamped addresses, unconditional (no branch and
                                              // no wait per load); masked where needed after the product
        auto gload = [&](int ka) -> T { return G[(long)(ka < K ? ka : K - 1) * ldg + kcl]; };
        // the block's own loads first: their latency hides behind the product
        T gk[16];   // G[k0 + i, kc]; rows k0 + i >= K are never used (those steps do not run)
#pragma unroll
        for (int i = 0; i < 16; ++i) gk[i] = gload(k0 + i);
        const T gkk_raw = gload(kc);
        T c_raw[MT][4];
#pragma unroll
        for (int m = 0; m < MT; ++m)
#pragma unroll
            for (int r = 0; r < 4; ++r) {
                const long row = r0 + 16 * m + A::row(grp, r);
                const long rl = row < R ? row : R - 1;
                c_raw[m][r] = C[CM ? (long)kcl * ldc + rl : rl * ldc + kcl];
            }
        // ---- T = V_cur G[:, k0 .. k0+15], two accumulators per 16-row tile (MFMA latency 40 > issue 32).
        // B (G from L2) in chunks of 16 k-steps = 64 coordinates, the next chunk loaded while this one's
        // MFMAs issue (16 MT of them, >= 512 cycles: an L2 round trip).  B needs no mask: the tile is zero
        // at coordinates >= K, and the columns of lanes with kc >= K are never used.
        acc_t acc[MT][2];
#pragma unroll
        for (int m = 0; m < MT; ++m) acc[m][0] = acc[m][1] = acc_t{};
        T bc[16], bn[16];
#pragma unroll
        for (int j = 0; j < 16; ++j) bc[j] = gload(4 * j + grp);
        for (int kb = 0; kb < Kp; kb += 64) {   // Kp is a multiple of 64
            if (kb + 64 < Kp) {
#pragma unroll
                for (int j = 0; j < 16; ++j) bn[j] = gload(kb + 64 + 4 * j + grp);
            }
#pragma unroll
            for (int j = 0; j < 16; ++j) {
                const int ka = kb + 4 * j + grp;
#pragma unroll
                for (int m = 0; m < MT; ++m) acc[m][j & 1] = A::mfma(wget(16 * m + col, ka), bc[j], acc[m][j & 1]);
            }
#pragma unroll
            for (int j = 0; j < 16; ++j) bc[j] = bn[j];
        }
        T c[MT][4];
#pragma unroll
        for (int m = 0; m < MT; ++m)
#pragma unroll
            for (int r = 0; r < 4; ++r) c[m][r] = (kc_ok && r0 + 16 * m + A::row(grp, r) < R) ? c_raw[m][r] : T(0);
        const T gkk = kc_ok ? gkk_raw : T(0);
        // ---- the 16 sequential steps of the block ----
        const bool act = gkk > T(0);
        const T inv = act ? T(1) / gkk : T(0);
        T t[MT][4], vo[MT][4], vn[MT][4];
#pragma unroll
        for (int m = 0; m < MT; ++m)
#pragma unroll
            for (int r = 0; r < 4; ++r) {
                t[m][r] = acc[m][0][r] + acc[m][1][r];
                vo[m][r] = kc_ok ? wget(16 * m + A::row(grp, r), kc) : T(0);
                vn[m][r] = vo[m][r];
            }
        hals_steps<T, MT, 0>(t, vo, c, vn, gk, inv, act, col, K - k0);
        if (kc_ok) {
#pragma unroll
            for (int m = 0; m < MT; ++m)
#pragma unroll
                for (int r = 0; r < 4; ++r) wput(16 * m + A::row(grp, r), kc, vn[m][r]);
        }
        __syncthreads();   // the block's new values before the next block's product reads them
    }

    if constexpr (IN_LDS) {
        if (!CM) {
            for (int rr = 0; rr < 16 * MT; ++rr)
                if (r0 + rr < R)
                    for (int k = lane; k < K; k += 64) V_out[vidx(r0 + rr, k)] = tile[rr * ldw + k];
        } else {
            for (int m = 0; m < MT; ++m)
                for (int k = grp; k < K; k += 4) {
                    const int rr = 16 * m + col;
                    if (r0 + rr < R) V_out[vidx(r0 + rr, k)] = tile[rr * ldw + k];
                }
        }
    }
}

template <class T, int MT, bool CM, bool IN_LDS>
inline hipError_t launch_nn_cd_sweep_cfg(hipStream_t st, const T* V_in, T* V_out, long ldv, const T* C, long ldc,
                                         const T* G, long ldg, int R, int K) {
    const int grid = (R + 16 * MT - 1) / (16 * MT);
    const size_t lds = IN_LDS ? hals_lds_bytes<T>(K, MT) : 0;
    hipLaunchKernelGGL((nn_cd_sweep_kernel<T, MT, CM, IN_LDS>), dim3(grid), dim3(64), lds, st, V_in, V_out, ldv, C,
                       ldc, G, ldg, R, K);
    return hipGetLastError();
}

// One sweep.  Two 16-row tiles per wave (one B load feeds two MFMAs) when there are rows enough for
// >= 1024 waves and the tile fits; one otherwise; the global-memory tile past 64 KiB.
template <class T, bool CM>
inline hipError_t launch_nn_cd_sweep(hipStream_t st, const T* V_in, T* V_out, long ldv, const T* C, long ldc,
                                     const T* G, long ldg, int R, int K) {
    if (R >= 32 * 1024 && hals_lds_bytes<T>(K, 2) <= (size_t)kHalsLdsBytes)
        return launch_nn_cd_sweep_cfg<T, 2, CM, true>(st, V_in, V_out, ldv, C, ldc, G, ldg, R, K);
    if (hals_lds_bytes<T>(K, 1) <= (size_t)kHalsLdsBytes)
        return launch_nn_cd_sweep_cfg<T, 1, CM, true>(st, V_in, V_out, ldv, C, ldc, G, ldg, R, K);
    return launch_nn_cd_sweep_cfg<T, 1, CM, false>(st, V_in, V_out, ldv, C, ldc, G, ldg, R, K);
}

// ---- the normalisation of one HALS iteration ----------------------------------------------------
// n_k = ||U_k||_2.  n_k > 0: D_new[k] = U_k / n_k, nrm[k] = n_k;  n_k = 0: D_new[k] = U_k (= 0), nrm[k] = 1.
// max|ref - D_new| goes to *gmax (zero on entry; *gmax_zero is cleared for the next iteration) and, by the
// last-arriving workgroup, to the pinned host word the loop polls (publish_max).
template <class T>
__global__ void __launch_bounds__(256) hals_normalize_kernel(const T* __restrict__ U, long F,
                                                             const T* __restrict__ ref, T* __restrict__ out,
                                                             T* __restrict__ nrm, T* __restrict__ gmax,
                                                             T* __restrict__ gmax_zero,
                                                             unsigned int* __restrict__ ticket,
                                                             T* __restrict__ host_out) {
    __shared__ T sh[4];
    __shared__ T s_nrm;
    const long row = blockIdx.x;
    const T* u = U + row * F;
    T acc = 0;
    for (long j = threadIdx.x; j < F; j += 256) acc += u[j] * u[j];
    const T tot = block_sum_256(acc, sh);
    if (threadIdx.x == 0) {
        const T n = sqrt(tot);
        s_nrm = n;
        nrm[row] = n > T(0) ? n : T(1);
    }
    __syncthreads();
    const T n = s_nrm;
    const bool scale = n > T(0);
    T md = 0;
    for (long j = threadIdx.x; j < F; j += 256) {
        const T o = scale ? u[j] / n : u[j];
        const T d = fabs(ref[row * F + j] - o);
        md = max_np(d, md);
        out[row * F + j] = o;
    }
    const T m = block_max_256(md, sh);
    if (threadIdx.x == 0) {
        if (gmax_zero != nullptr && row == 0) *gmax_zero = T(0);
        publish_max(m, gmax, ticket, host_out, true);
    }
}

// x[:, k] *= nrm[k]  (nrm = 1 where the atom was zero: x unchanged bit for bit)
template <class T>
__global__ void __launch_bounds__(256) hals_rescale_kernel(T* __restrict__ X, long n, int K,
                                                           const T* __restrict__ nrm) {
    for (long i = blockIdx.x * 256L + threadIdx.x; i < n; i += (long)gridDim.x * 256L) X[i] *= nrm[i % K];
}

}  // namespace dcp
