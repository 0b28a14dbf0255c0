// Approximate K-SVD (Rubinstein, Zibulevsky & Elad 2008): the dictionary update that goes with the OMP coder of
// omp.hpp,
//
//   min |Y - X D|^2  s.t.  |x_i|_0 <= s, |d_k| = 1        Y [N, F], X [N, K], D [K, F] (atoms are rows)
//
// One iteration: X = omp(Y, D, s) (omp_solve, unchanged); R = Y - X D once, on the GEMM cores (EpiSubFrom); then
// the atom sweep, for k = 0 .. K-1 in order, with I = {i : X[i, k] != 0} in ascending row order, fixed for the
// whole sweep (the lists are built once, before atom 0):
//   I empty: atom k is left as it is (the sweep replaces no atom; the cleaning pass of ksvd_clean.hpp may, after it)
//   g = X[I, k], d = D[k]:   u  = g^H R[I, :] + |g|^2 d       (= g^H E for E = R[I, :] + g d; E is never formed)
//                            d' = u / |u|, or d where !(|u| > 0) (a NaN keeps d)
//                            g' = R[I, :] d'^H + g (d . d'^H)
//                            R[I, :] += g d - g' d';  X[I, k] = g';  D[k] = d'
// so R = Y - X D throughout, and no step of the sweep increases |R|^2.
//
// Kernels.  Order between atoms is stream order; nothing waits on another workgroup.  No float atomics: every sum has
// a fixed order that depends on the sizes alone (not on the grid or the CU count), so results are bitwise
// reproducible.
//   lists   a CSC-style index of X: rows are cut into blocks of kKsvdRowBlock; ksvd_count_kernel counts, per block
//           and column, the non-zeros (thread = column: coalesced in k) and the non-zeros per row (ballots);
//           ksvd_scan_kernel turns the per-block counts into per-block offsets inside the column,
//           ksvd_offsets_kernel the column totals into column offsets; ksvd_fill_kernel walks the same blocks again
//           and writes every column's rows in ascending order.  No atomics except one integer max (the row count).
//   pass 1  u: the support is cut into chunks of kKsvdChunk rows; workgroup (chunk, column tile) sums
//           conj(g_i) R[i, :] over the chunk's rows into part[chunk, :] (each wave a quarter of the chunk in list
//           order, the four sums added in wave order) and leaves |g|^2 of the chunk
//   finish  a workgroup per 256 columns: u = sum of the partials in chunk order + |g|^2 d, and its tile's share of
//           |u|^2, d . u^H and |d|^2 (d is read from the copy of D taken at the start of the sweep, which also
//           serves max|D_new - D_old|)
//   pass 2  one wave per support row: |u| and d . d'^H from the tile shares (in tile order), d' = u / |u| formed
//           where it is used; reads the row once (16-byte loads where the rows are 16-byte aligned) and keeps it in
//           the wave's LDS slice while the butterfly forms g', then applies the rank-2 correction and writes the row
//           once.  Rows too long for the slice (F sizeof(T) > kKsvdLdsBytes) are read a second time instead.  The
//           waves also write D[k] = d', a slice each.
// Each atom makes two reads and one write of its support rows of R: 3 sum_k |I_k| F sizeof(T) bytes per sweep.
//
// The sweep for data with holes (every inner product weighted per row, and its own monotonicity argument) is stated
// in ksvd_mask.hpp, which holds its three kernels.  The host path below is one for both: the atom loop launches the
// three kernels of this file or those three, and the coder of a step is OmpCoder (omp_mask.hpp) for mask = none, 1-D
// or 2-D.
//
// The replacement of unused and duplicate atoms after a sweep (dcp_ksvd_clean_step_*, dcp_ksvd_clean_*) is stated in
// ksvd_clean.hpp, which holds its kernels, its workspace and its entry; the step below runs it on request.
#pragma once
#include <hip/hip_runtime.h>

#include <cstdint>

#include "omp_mask.hpp"

namespace dcp {

constexpr int kKsvdChunk = 128;        // support rows per pass-1 partial
constexpr int kKsvdRowBlock = 256;     // rows per block of the list build
constexpr int kKsvdLdsBytes = 65536;   // LDS of one pass-2 workgroup: its waves' row slices
constexpr int kKsvdMdParts = 64;       // workgroups (and partial maxima) of max|D_new - D_old|

template <class T, int V>
struct alignas(V > 1 ? 16 : alignof(T)) KsvdPack {
    T v[V];
};
// elements per 16-byte access
template <class T>
constexpr int ksvd_vec() { return sizeof(T) >= 16 ? 1 : 16 / (int)sizeof(T); }

__device__ __forceinline__ bool ksvd_nz(float a)  { return a != 0.0f; }
__device__ __forceinline__ bool ksvd_nz(double a) { return a != 0.0; }
template <class R>
__device__ __forceinline__ bool ksvd_nz(cx<R> a) { return a.re != R(0) || a.im != R(0); }

template <class T>
__device__ __forceinline__ T ksvd_div(T a, real_t<T> s) {   // a true division, as the reference's u / |u|
    if constexpr (scalar_traits<T>::is_complex) return T{a.re / s, a.im / s};
    else return a / s;
}

// one element of the new atom: d' = u / |u|, or d where !(|u| > 0)
template <class T, int V>
__device__ __forceinline__ T ksvd_new_atom(bool keep_d, const KsvdPack<T, V>& d, const KsvdPack<T, V>& u, int q,
                                           real_t<T> nrm) {
    return keep_d ? d.v[q] : ksvd_div(u.v[q], nrm);
}

// ---- the support lists ---------------------------------------------------------------------------
// meta[0] (zero on entry) <- the largest number of non-zeros in a row; blockcnt[b, k] <- non-zeros of column k in
// rows [b RB, (b + 1) RB).  grid: ceil(N / RB) workgroups of 256.
template <class T>
__global__ void __launch_bounds__(256) ksvd_count_kernel(const T* __restrict__ X, int N, int K,
                                                         int* __restrict__ blockcnt, int* __restrict__ meta) {
    __shared__ int rowcnt[kKsvdRowBlock];
    const int tid = threadIdx.x, lane = tid & 63;
    const long r0 = (long)blockIdx.x * kKsvdRowBlock;
    const int nr = (int)((N - r0) < kKsvdRowBlock ? (N - r0) : kKsvdRowBlock);
    for (int r = tid; r < kKsvdRowBlock; r += 256) rowcnt[r] = 0;
    __syncthreads();
    for (int k0 = 0; k0 < K; k0 += 256) {
        const int k = k0 + tid;
        const bool live = k < K;
        const T* col = X + r0 * K + (live ? k : K - 1);
        int c = 0;
        for (int r = 0; r < nr; ++r) {
            const bool nz = live && ksvd_nz(col[(long)r * K]);
            c += (int)nz;
            const unsigned long long b = __ballot(nz);
            if (lane == 0 && b != 0ull) atomicAdd(&rowcnt[r], __popcll(b));
        }
        if (live) blockcnt[(long)blockIdx.x * K + k] = c;
    }
    __syncthreads();
    int m = 0;
    for (int r = tid; r < nr; r += 256) m = rowcnt[r] > m ? rowcnt[r] : m;
#pragma unroll
    for (int o = 32; o > 0; o >>= 1) {
        const int w = lane_down(m, o);
        m = w > m ? w : m;
    }
    if (lane == 0 && m > 0) atomicMax(&meta[0], m);
}

// blockoff[b, k] <- sum_{b' < b} blockcnt[b', k]; cnt[k] <- the column total.  thread = column.
__global__ void __launch_bounds__(256) ksvd_scan_kernel(const int* __restrict__ blockcnt, int nb, int K,
                                                        int* __restrict__ blockoff, int* __restrict__ cnt) {
    const int k = blockIdx.x * 256 + threadIdx.x;
    if (k >= K) return;
    int run = 0;
#pragma unroll 8
    for (int b = 0; b < nb; ++b) {
        blockoff[(long)b * K + k] = run;
        run += blockcnt[(long)b * K + k];
    }
    cnt[k] = run;
}

// off[k] = sum_{k' < k} cnt[k'], off[K] = the total.  One workgroup of 256.
__global__ void __launch_bounds__(256) ksvd_offsets_kernel(const int* __restrict__ cnt, int K,
                                                           long long* __restrict__ off) {
    __shared__ long long seg_sum[256];
    const int tid = threadIdx.x;
    const int seg = (K + 255) / 256;
    const int k0 = tid * seg < K ? tid * seg : K, k1 = k0 + seg < K ? k0 + seg : K;
    long long s = 0;
    for (int k = k0; k < k1; ++k) s += cnt[k];
    seg_sum[tid] = s;
    __syncthreads();
    if (tid == 0) {
        long long run = 0;
        for (int t = 0; t < 256; ++t) {
            const long long v = seg_sum[t];
            seg_sum[t] = run;
            run += v;
        }
        off[K] = run;
    }
    __syncthreads();
    long long run = seg_sum[tid];
    for (int k = k0; k < k1; ++k) {
        off[k] = run;
        run += cnt[k];
    }
}

// rows[off[k] + ...] <- the rows of column k's non-zeros, ascending.  Same grid and walk as ksvd_count_kernel.
template <class T>
__global__ void __launch_bounds__(256) ksvd_fill_kernel(const T* __restrict__ X, int N, int K,
                                                        const int* __restrict__ blockoff,
                                                        const long long* __restrict__ off, int* __restrict__ rows) {
    const int tid = threadIdx.x;
    const long r0 = (long)blockIdx.x * kKsvdRowBlock;
    const int nr = (int)((N - r0) < kKsvdRowBlock ? (N - r0) : kKsvdRowBlock);
    for (int k = tid; k < K; k += 256) {
        const T* col = X + r0 * K + k;
        long long pos = off[k] + blockoff[(long)blockIdx.x * K + k];
        const long long end = off[k + 1];   // (never reached: the counts come from the same X)
        for (int r = 0; r < nr; ++r) {
            if (ksvd_nz(col[(long)r * K]) && pos < end) rows[pos++] = (int)(r0 + r);
        }
    }
}

// ---- pass 1: part[chunk, :] = sum over the chunk's rows of conj(g_i) R[i, :] ------------------------------------
// grid: nchunks * ntiles workgroups of 256 (blockIdx.x = chunk * ntiles + tile).  A workgroup owns 64 V adjacent
// columns; its four waves take a quarter of the chunk's rows each, in list order, and the four sums are added in
// wave order: ((w0 + w1) + w2) + w3.  The workgroups of tile 0 also leave gpart[chunk] = sum |g_i|^2.
template <class T, int V>
__global__ void __launch_bounds__(256) ksvd_pass1_kernel(const T* __restrict__ Rm, const T* __restrict__ X,
                                                         const int* __restrict__ rows,
                                                         const long long* __restrict__ off, int k, int K, long F,
                                                         int ntiles, T* __restrict__ part,
                                                         real_t<T>* __restrict__ gpart) {
    typedef KsvdPack<T, V> P;
    typedef real_t<T> R;
    constexpr int kQuarter = kKsvdChunk / 4;
    __shared__ int s_row[kKsvdChunk];
    __shared__ T s_gc[kKsvdChunk];
    __shared__ T s_acc[3][64 * V];
    const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
    const int chunk = blockIdx.x / ntiles, tile = blockIdx.x - chunk * ntiles;
    const long long base = off[k] + (long long)chunk * kKsvdChunk;
    const long long left = off[k + 1] - base;
    const int n = (int)(left < kKsvdChunk ? left : kKsvdChunk);
    for (int e = tid; e < n; e += 256) {
        const int i = rows[base + e];
        s_row[e] = i;
        s_gc[e] = conj_of(X[(long)i * K + k]);
    }
    __syncthreads();
    if (tile == 0 && wave == 0) {
        R a = 0;
        for (int e = lane; e < n; e += 64) a += abs2(s_gc[e]);
        a = wave_sum_all(a);
        if (lane == 0) gpart[chunk] = a;
    }
    const long j = ((long)tile * 64 + lane) * V;
    const bool live = j < F;
    T acc[V];
#pragma unroll
    for (int q = 0; q < V; ++q) acc[q] = zero_of<T>();
    if (live) {
        const int e0 = wave * kQuarter;
        const int e1 = e0 + kQuarter < n ? e0 + kQuarter : n;
#pragma unroll 8
        for (int e = e0; e < e1; ++e) {
            const P r = *reinterpret_cast<const P*>(Rm + (long)s_row[e] * F + j);
            const T gc = s_gc[e];
#pragma unroll
            for (int q = 0; q < V; ++q) acc[q] = fmadd(acc[q], gc, r.v[q]);
        }
    }
    if (wave > 0) {
#pragma unroll
        for (int q = 0; q < V; ++q) s_acc[wave - 1][lane * V + q] = acc[q];
    }
    __syncthreads();
    if (wave == 0 && live) {
        P o;
#pragma unroll
        for (int q = 0; q < V; ++q)
            o.v[q] = add(add(add(acc[q], s_acc[0][lane * V + q]), s_acc[1][lane * V + q]), s_acc[2][lane * V + q]);
        *reinterpret_cast<P*>(part + (long)chunk * F + j) = o;
    }
}

// ---- finish: u = sum of the partials in chunk order + |g|^2 d -> ubuf, and this tile's share of |u|^2, d . u^H
// and |d|^2.  grid: ceil(F / 256) workgroups of 256, a thread owns one column. ---------------------------------
template <class T>
__global__ void __launch_bounds__(256) ksvd_finish_kernel(const T* __restrict__ part,
                                                          const real_t<T>* __restrict__ gpart, int nchunks, int k,
                                                          long F, const T* __restrict__ Dold, T* __restrict__ ubuf,
                                                          real_t<T>* __restrict__ usq, T* __restrict__ udd,
                                                          real_t<T>* __restrict__ dsq) {
    typedef real_t<T> R;
    __shared__ R sh[4];
    __shared__ R s_gn2;
    const int tid = threadIdx.x;
    R a = 0;
    for (int c = tid; c < nchunks; c += 256) a += gpart[c];
    a = block_sum_256(a, sh);
    if (tid == 0) s_gn2 = a;
    __syncthreads();
    const R gn2 = s_gn2;
    const long j = blockIdx.x * 256L + tid;
    R uu = 0, dq = 0;
    T du = zero_of<T>();
    if (j < F) {
        T u = part[j];
#pragma unroll 4
        for (int c = 1; c < nchunks; ++c) u = add(u, part[(long)c * F + j]);
        const T dj = Dold[(long)k * F + j];
        u = add(u, scale(dj, gn2));
        ubuf[j] = u;
        uu = abs2(u);
        dq = abs2(dj);
        du = mul(dj, conj_of(u));
    }
    uu = block_sum_256(uu, sh);
    dq = block_sum_256(dq, sh);
    // (not block_sum_256_parts: handing it du's parts changes which product of mul(dj, conj(u)) the compiler fuses
    // for complex64, and with it the bits of u . d^H)
    const R re = block_sum_256(real_part(du), sh);
    R im = 0;
    if constexpr (scalar_traits<T>::is_complex) im = block_sum_256(du.im, sh);
    if (tid == 0) {
        usq[blockIdx.x] = uu;
        dsq[blockIdx.x] = dq;
        if constexpr (scalar_traits<T>::is_complex) udd[blockIdx.x] = T{re, im};
        else udd[blockIdx.x] = re;
    }
}

// the sum of a[0 .. n) in a fixed order, the same bits in every lane: lane l takes l, l + 64, ..., then the butterfly
template <class S>
__device__ __forceinline__ S ksvd_lane_sum(const S* __restrict__ a, int n, int lane) {
    S s = zero_of<S>();
    for (int t = lane; t < n; t += 64) s = add(s, a[t]);
    return wave_sum_all(s);
}

// ---- pass 2: d' = u / |u| (d where !(|u| > 0));  g' = R[i, :] d'^H + g (d . d'^H);  R[i, :] += g d - g' d';
// X[i, k] = g';  D[k] = d'.  One wave per support row. ----------------------------------------------------------
// grid: ceil(|I| / W) workgroups of 64 W threads, dynamic LDS W * F elements when use_lds.  No barrier: a lane reads
// back only what it stored itself.  D[k] is not read here (d comes from Dold, u from ubuf): wave e of the |I| also
// writes the columns (e + m |I|) 64 V .. of d', so every column is written once.
template <class T, int V>
__global__ void __launch_bounds__(256) ksvd_pass2_kernel(T* __restrict__ Rm, T* __restrict__ X,
                                                         const int* __restrict__ rows,
                                                         const long long* __restrict__ off, int k, int K, long F,
                                                         const T* __restrict__ Dold, T* __restrict__ D,
                                                         const T* __restrict__ ubuf,
                                                         const real_t<T>* __restrict__ usq,
                                                         const T* __restrict__ udd,
                                                         const real_t<T>* __restrict__ dsq, int nparts, int use_lds) {
    typedef KsvdPack<T, V> P;
    typedef real_t<T> R;
    extern __shared__ __attribute__((aligned(16))) unsigned char ksvd_lds[];
    const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
    const long long e = (long long)blockIdx.x * (blockDim.x >> 6) + wave;
    const long long b = off[k];
    const long long cnt = off[k + 1] - b;
    if (e >= cnt) return;
    const long i = rows[b + e];
    T* r = Rm + i * F;
    const T* d = Dold + (long)k * F;
    T* slice = reinterpret_cast<T*>(ksvd_lds) + (use_lds ? (long)wave * F : 0);
    const T g = X[i * K + k];
    const R nrm = sqrt(ksvd_lane_sum(usq, nparts, lane));
    const bool keep_d = !(nrm > R(0));
    const T dd = keep_d ? from_real<T>(ksvd_lane_sum(dsq, nparts, lane))
                        : ksvd_div(ksvd_lane_sum(udd, nparts, lane), nrm);
    T acc = zero_of<T>();
#pragma unroll 4
    for (long j = (long)lane * V; j < F; j += 64 * V) {
        const P rv = *reinterpret_cast<const P*>(r + j);
        const P uv = *reinterpret_cast<const P*>(ubuf + j);
        const P ov = *reinterpret_cast<const P*>(d + j);
#pragma unroll
        for (int q = 0; q < V; ++q) {
            const T dn = ksvd_new_atom(keep_d, ov, uv, q, nrm);
            acc = fmadd(acc, rv.v[q], conj_of(dn));
        }
        if (use_lds) *reinterpret_cast<P*>(slice + j) = rv;
    }
    const T gn = fmadd(wave_sum_all(acc), g, dd);
    const T mgn = sub(zero_of<T>(), gn);
#pragma unroll 4
    for (long j = (long)lane * V; j < F; j += 64 * V) {
        const P rv = use_lds ? *reinterpret_cast<const P*>(slice + j) : *reinterpret_cast<const P*>(r + j);
        const P uv = *reinterpret_cast<const P*>(ubuf + j);
        const P ov = *reinterpret_cast<const P*>(d + j);
        P o;
#pragma unroll
        for (int q = 0; q < V; ++q) {
            const T dn = ksvd_new_atom(keep_d, ov, uv, q, nrm);
            o.v[q] = fmadd(fmadd(rv.v[q], g, ov.v[q]), mgn, dn);
        }
        *reinterpret_cast<P*>(r + j) = o;
    }
    if (lane == 0) X[i * K + k] = gn;
    for (long j = (e * 64 + lane) * V; j < F; j += cnt * 64 * V) {
        const P uv = *reinterpret_cast<const P*>(ubuf + j);
        const P ov = *reinterpret_cast<const P*>(d + j);
        P o;
#pragma unroll
        for (int q = 0; q < V; ++q) o.v[q] = ksvd_new_atom(keep_d, ov, uv, q, nrm);
        *reinterpret_cast<P*>(D + (long)k * F + j) = o;
    }
}

}  // namespace dcp

// ---- the three kernels of the weighted sweep: they use the pieces above, the host path below launches them -----
#include "ksvd_mask.hpp"

namespace dcp {

// ---- workspace ------------------------------------------------------------------------------------------------
template <class T>
struct KsvdWs {
    T* R = nullptr;              // [N, F] the maintained residual
    T* Dold = nullptr;           // [K, F] D at the start of the sweep
    T* part = nullptr;           // [ceil(N / kKsvdChunk), F] pass-1 partials
    real_t<T>* cpart = nullptr;  // the same shape, masked calls only: pass-1 partials of c
    T* ubuf = nullptr;           // [F] u of the atom in flight
    real_t<T>* gpart = nullptr;  // [ceil(N / kKsvdChunk)] |g|^2 per chunk (unmasked; so are udd and dsq)
    real_t<T>* usq = nullptr;    // [ceil(F / 256)] |u|^2, d . u^H and |d|^2 per finish tile
    T* udd = nullptr;
    real_t<T>* dsq = nullptr;
    int* rows = nullptr;         // [N * s] the lists
    long long* off = nullptr;    // [K + 1]
    int* blockcnt = nullptr;     // [ceil(N / kKsvdRowBlock), K] non-zeros per row block and column
    int* blockoff = nullptr;     // the same shape: their running sums down each column
    int* meta = nullptr;         // [4 + K]: the largest row count, then the column counts
    double* mdpart = nullptr;    // [kKsvdMdParts]
    real_t<T>* ext = nullptr;    // complex: the real image of D for the residual product (4KF reals)
};

template <class T>
inline void ksvd_layout(WsLayout& a, KsvdWs<T>& w, int64_t N, int64_t F, int64_t K, int64_t s, bool masked) {
    a.take(w.R, (size_t)N * F);
    a.take(w.Dold, (size_t)K * F);
    a.take(w.part, (size_t)((N + kKsvdChunk - 1) / kKsvdChunk) * F);
    a.take(w.ubuf, (size_t)F);
    a.take(w.gpart, (size_t)((N + kKsvdChunk - 1) / kKsvdChunk));
    a.take(w.usq, (size_t)((F + 255) / 256));
    a.take(w.udd, (size_t)((F + 255) / 256));
    a.take(w.dsq, (size_t)((F + 255) / 256));
    a.take(w.rows, (size_t)N * s);
    a.take(w.off, (size_t)K + 1);
    a.take(w.blockcnt, (size_t)((N + kKsvdRowBlock - 1) / kKsvdRowBlock) * K);
    a.take(w.blockoff, (size_t)((N + kKsvdRowBlock - 1) / kKsvdRowBlock) * K);
    a.take(w.meta, (size_t)K + 4);
    a.take(w.mdpart, (size_t)kKsvdMdParts);
    if (scalar_traits<T>::is_complex) a.take(w.ext, (size_t)4 * K * F);
    if (masked) a.take(w.cpart, (size_t)((N + kKsvdChunk - 1) / kKsvdChunk) * F);
}

// Enqueues the counting half of the list build: afterwards w.meta holds the largest row count and the column counts.
template <class T>
inline int ksvd_count(dcp_handle* h, const T* X, int N, int K, KsvdWs<T>& w) {
    hipStream_t st = h->stream;
    const int nb = (N + kKsvdRowBlock - 1) / kKsvdRowBlock;
    DCP_HIP_OK(h, hipMemsetAsync(w.meta, 0, 4 * sizeof(int), st));
    hipLaunchKernelGGL((ksvd_count_kernel<T>), dim3(nb), dim3(256), 0, st, X, N, K, w.blockcnt, w.meta);
    DCP_LAUNCH_OK(h, hipGetLastError());
    hipLaunchKernelGGL(ksvd_scan_kernel, dim3((K + 255) / 256), dim3(256), 0, st, (const int*)w.blockcnt, nb, K,
                       w.blockoff, w.meta + 4);
    DCP_LAUNCH_OK(h, hipGetLastError());
    hipLaunchKernelGGL(ksvd_offsets_kernel, dim3(1), dim3(256), 0, st, (const int*)(w.meta + 4), K, w.off);
    DCP_LAUNCH_OK(h, hipGetLastError());
    return DCP_OK;
}

// pass 2's workgroup: the row kept in LDS where it fits (use_lds), as many waves (4, 2 or 1) as slices fit
struct KsvdPass2Shape {
    int use_lds, waves;
    size_t lds;
};
template <class T>
inline KsvdPass2Shape ksvd_pass2_shape(int F) {
    const size_t row_bytes = (size_t)F * sizeof(T);
    const int use_lds = row_bytes <= (size_t)kKsvdLdsBytes;
    int waves = 4;
    while (use_lds && waves > 1 && waves * row_bytes > (size_t)kKsvdLdsBytes) waves >>= 1;
    return KsvdPass2Shape{use_lds, waves, use_lds ? waves * row_bytes : 0};
}

// The mask of a sweep: M with a row stride of ms elements (F, or 0 for a 1-D mask); M == nullptr: no mask.
template <class R>
struct KsvdMask {
    const R* M;
    long ms;
};

// The K atoms in order, three launches each: the kernels of this file, or with a mask those of ksvd_mask.hpp.
template <class T, int V>
inline int ksvd_atoms(dcp_handle* h, KsvdMask<real_t<T>> m, T* X, T* D, int F, int K, const int* cnt, KsvdWs<T>& w) {
    typedef real_t<T> R;
    hipStream_t st = h->stream;
    const long ntiles = ((long)F + 64L * V - 1) / (64L * V);
    const int nparts = (int)(((long)F + 255) / 256);
    const KsvdPass2Shape p2 = ksvd_pass2_shape<T>(F);
    const int* rows = w.rows;
    const long long* off = w.off;
    const T* Dold = w.Dold;
    for (int k = 0; k < K; ++k) {
        if (cnt[k] == 0) continue;
        const long nchunks = ((long)cnt[k] + kKsvdChunk - 1) / kKsvdChunk;
        if (nchunks * ntiles > 0x7fffffffL) return fail(h, DCP_ERR_INVALID, "ksvd: the pass-1 grid exceeds 2^31-1");
        const dim3 g1((unsigned)(nchunks * ntiles)), g2((unsigned)((cnt[k] + p2.waves - 1) / p2.waves));
        if (m.M) {
            hipLaunchKernelGGL((ksvd_mask_pass1_kernel<T, V>), g1, dim3(256), 0, st, (const T*)w.R, m.M, m.ms,
                               (const T*)X, rows, off, k, K, (long)F, (int)ntiles, w.part, w.cpart);
            hipLaunchKernelGGL((ksvd_mask_finish_kernel<T>), dim3(nparts), dim3(256), 0, st, (const T*)w.part,
                               (const R*)w.cpart, (int)nchunks, k, (long)F, Dold, w.ubuf, w.usq);
            hipLaunchKernelGGL((ksvd_mask_pass2_kernel<T, V>), g2, dim3(64 * p2.waves), p2.lds, st, w.R, m.M, m.ms, X,
                               rows, off, k, K, (long)F, Dold, D, (const T*)w.ubuf, (const R*)w.usq, nparts,
                               p2.use_lds);
        } else {
            hipLaunchKernelGGL((ksvd_pass1_kernel<T, V>), g1, dim3(256), 0, st, (const T*)w.R, (const T*)X, rows, off,
                               k, K, (long)F, (int)ntiles, w.part, w.gpart);
            hipLaunchKernelGGL((ksvd_finish_kernel<T>), dim3(nparts), dim3(256), 0, st, (const T*)w.part,
                               (const R*)w.gpart, (int)nchunks, k, (long)F, Dold, w.ubuf, w.usq, w.udd, w.dsq);
            hipLaunchKernelGGL((ksvd_pass2_kernel<T, V>), g2, dim3(64 * p2.waves), p2.lds, st, w.R, X, rows, off, k,
                               K, (long)F, Dold, D, (const T*)w.ubuf, (const R*)w.usq, (const T*)w.udd,
                               (const R*)w.dsq, nparts, p2.use_lds);
        }
        DCP_LAUNCH_OK(h, hipGetLastError());
    }
    return DCP_OK;
}

// w.R = Y - X D on the GEMM cores
template <class T>
inline int ksvd_residual(dcp_handle* h, const T* Y, const T* X, const T* D, int N, int F, int K, KsvdWs<T>& w) {
    GemmArgs<T> a;
    a.A = X; a.lda = K; a.B = D; a.ldb = F; a.M = N; a.N = F; a.K = K;
    a.ext_ws = w.ext;
    DCP_LAUNCH_OK(h, (gemm<FORM_NN>(h->stream, a, EpiSubFrom<T>{Y, (long)F, w.R, (long)F})));
    return DCP_OK;
}

// What every sweep does before atom 0: the lists (on the counts of ksvd_count), the copy of D, R = Y - X D.
template <class T>
inline int ksvd_sweep_begin(dcp_handle* h, const T* Y, T* X, T* D, int N, int F, int K, KsvdWs<T>& w) {
    hipStream_t st = h->stream;
    const int nb = (N + kKsvdRowBlock - 1) / kKsvdRowBlock;
    hipLaunchKernelGGL((ksvd_fill_kernel<T>), dim3(nb), dim3(256), 0, st, (const T*)X, N, K,
                       (const int*)w.blockoff, (const long long*)w.off, w.rows);
    DCP_LAUNCH_OK(h, hipGetLastError());
    DCP_HIP_OK(h, hipMemcpyAsync(w.Dold, D, (size_t)K * F * sizeof(T), hipMemcpyDeviceToDevice, st));
    return ksvd_residual<T>(h, Y, (const T*)X, (const T*)D, N, F, K, w);
}

// ... and after atom K - 1: mdpart[b] = max |D - Dold| over workgroup b's share (NaN wins, as np.max), as double
template <class T>
inline int ksvd_sweep_end(dcp_handle* h, const T* D, int F, int K, KsvdWs<T>& w) {
    hipLaunchKernelGGL((reduce_partial_kernel<MaxOp, MapAbsDiff<T>, double>), dim3(grid_for((long)K * F, kKsvdMdParts)),
                       dim3(256), 0, h->stream, MapAbsDiff<T>{D, w.Dold}, (long)K * F, w.mdpart);
    DCP_LAUNCH_OK(h, hipGetLastError());
    return DCP_OK;
}

// Steps 2 and 3 on X whose counts (cnt [K], host) ksvd_count produced: the lists, R = Y - X D, the K atoms, then
// max|D_new - D_old| into w.mdpart.  Enqueues only, from this one call: no host round trip between atoms.
template <class T>
inline int ksvd_sweep(dcp_handle* h, const T* Y, KsvdMask<real_t<T>> m, T* X, T* D, int N, int F, int K,
                      const int* cnt, KsvdWs<T>& w) {
    constexpr int V = ksvd_vec<T>();
    DCP_TRY(ksvd_sweep_begin<T>(h, Y, X, D, N, F, K, w));
    // 16-byte accesses where every row of R, D and the partials starts on a 16-byte boundary and, with a mask, every
    // mask row is aligned for its V reals (F is then a multiple of V, so the rows are where M is)
    const bool vec = V > 1 && ((size_t)F * sizeof(T)) % 16 == 0 && al16_ptr(D) &&
                     (!m.M || reinterpret_cast<uintptr_t>(m.M) % (V * sizeof(real_t<T>)) == 0);
    if (vec) DCP_TRY((ksvd_atoms<T, V>(h, m, X, D, F, K, cnt, w)));
    else DCP_TRY((ksvd_atoms<T, 1>(h, m, X, D, F, K, cnt, w)));
    return ksvd_sweep_end<T>(h, D, F, K, w);
}

// host <- the largest row count, the column counts and (it_dev given) OMP's step count: one synchronisation
inline int ksvd_read_counts(dcp_handle* h, const int* meta, int K, const int* it_dev, int** host_out) {
    void* hostv = nullptr;
    DCP_TRY(host_scratch(h, ((size_t)K + 8) * sizeof(int) + kKsvdMdParts * sizeof(double), &hostv));
    int* hi = reinterpret_cast<int*>(hostv);
    DCP_HIP_OK(h, hipMemcpyAsync(hi, meta, ((size_t)K + 4) * sizeof(int), hipMemcpyDeviceToHost, h->stream));
    if (it_dev != nullptr)
        DCP_HIP_OK(h, hipMemcpyAsync(hi + K + 4, it_dev, sizeof(int), hipMemcpyDeviceToHost, h->stream));
    DCP_HIP_OK(h, hipStreamSynchronize(h->stream));
    *host_out = hi;
    return DCP_OK;
}

// *maxdiff_out <- the maximum of the partial maxima (NaN wins); synchronises the stream
inline int ksvd_read_maxdiff(dcp_handle* h, const double* mdpart, long n, double* maxdiff_out) {
    void* hostv = nullptr;
    DCP_TRY(host_scratch(h, kKsvdMdParts * sizeof(double), &hostv));
    return read_partial_max(h, mdpart, grid_for(n, kKsvdMdParts), reinterpret_cast<double*>(hostv), maxdiff_out);
}

}  // namespace dcp

// ---- the cleaning pass (replacement of unused and duplicate atoms): its kernels, workspace and entry -------------
#include "ksvd_clean.hpp"

namespace dcp {

// The entries.  masked false (dcp_ksvd_sweep_*, dcp_ksvd_step_*): M, mask_ndim and rows_per_pass are nullptr, 0, 0;
// masked true (dcp_ksvd_mask_*): a null mask and mask_ndim outside {1, 2} are refused.
template <class T>
inline int ksvd_sweep_api(dcp_handle* h, const T* Y, const real_t<T>* M, int mask_ndim, bool masked, T* X, T* D,
                          int64_t N, int64_t F, int64_t K, int row_nnz_max, double* maxdiff_out) {
    if (!h) return DCP_ERR_INVALID;
    if (!Y || (masked && !M) || !X || !D || !maxdiff_out) return fail(h, DCP_ERR_INVALID, "null pointer");
    if (masked) DCP_TRY(omp_check_mask(h, "ksvd", mask_ndim, 0));
    DCP_TRY(omp_check_sizes(h, N, F, K));
    if (row_nnz_max < 1 || row_nnz_max > K) return fail(h, DCP_ERR_INVALID, "ksvd: row_nnz_max must be in [1, K]");
    DCP_HIP_OK(h, hipSetDevice(h->device));
    KsvdWs<T> w;
    DCP_TRY(ws_lay_out(h, [&](WsLayout& a) { ksvd_layout<T>(a, w, N, F, K, row_nnz_max, masked); }));
    DCP_TRY(ksvd_count<T>(h, X, (int)N, (int)K, w));
    int* host = nullptr;
    DCP_TRY(ksvd_read_counts(h, w.meta, (int)K, nullptr, &host));
    if (host[0] > row_nnz_max)
        return fail(h, DCP_ERR_INVALID, "ksvd: a row of X has " + std::to_string(host[0]) +
                                            " non-zeros, more than row_nnz_max = " + std::to_string(row_nnz_max));
    const KsvdMask<real_t<T>> m{M, mask_ndim == 2 ? (long)F : 0L};
    DCP_TRY(ksvd_sweep<T>(h, Y, m, X, D, (int)N, (int)F, (int)K, host + 4, w));
    return ksvd_read_maxdiff(h, w.mdpart, (long)K * F, maxdiff_out);
}

// What dcp_ksvd_clean_step_* adds to a step: the threshold, the gate and where the number of marked atoms goes
struct KsvdCleanCall {
    double max_coherence, stop_tol;
    int* n_marked_out;
};

// The coder (OmpCoder: plain OMP, or the masked coder as dcp_omp_mask_* runs it), then the sweep, over one
// workspace layout.  With `clean` (dcp_ksvd_clean_step_*; masked is then whether a mask was given) the cleaning
// pass of ksvd_clean.hpp follows on the sweep's own R: the marking is enqueued before max|D_new - D_old| is read and
// its count comes back in that same synchronisation, so the step gains no host round trip; energies, selection and
// replacement are enqueued (and left in flight on the handle's stream) only if an atom is marked and
// maxdiff >= stop_tol, which a NaN fails.
template <class T>
inline int ksvd_step_api(dcp_handle* h, const T* Y, const real_t<T>* M, int mask_ndim, bool masked, T* X, T* D,
                         int64_t N, int64_t F, int64_t K, int n_nonzero, double coef_tol, int rows_per_pass,
                         double* maxdiff_out, int* it_out, const KsvdCleanCall* clean = nullptr) {
    if (!h) return DCP_ERR_INVALID;
    if (!Y || (masked && !M) || !X || !D || !maxdiff_out || !it_out || (clean && !clean->n_marked_out))
        return fail(h, DCP_ERR_INVALID, "null pointer");
    if (clean) DCP_TRY(ksvd_clean_check(h, M, mask_ndim, clean->max_coherence, clean->stop_tol));
    if (masked) DCP_TRY(omp_check_mask(h, "ksvd", mask_ndim, rows_per_pass));
    DCP_TRY(omp_check_problem<T>(h, N, F, K, n_nonzero, coef_tol));
    DCP_HIP_OK(h, hipSetDevice(h->device));
    OmpCoder<T> coder(M, mask_ndim, masked ? rows_per_pass : 0);
    KsvdWs<T> w;
    KsvdCleanWs<T> c;
    DCP_TRY(ws_lay_out(h, [&](WsLayout& a) {
        coder.layout(a, N, F, K, n_nonzero);
        ksvd_layout<T>(a, w, N, F, K, n_nonzero, masked);
        if (clean) ksvd_clean_layout<T>(a, c, N, F, K, clean->max_coherence > 0.0);
    }));
    DCP_TRY(coder.solve(h, Y, (const T*)D, X, N, F, K, n_nonzero, coef_tol));
    DCP_TRY(ksvd_count<T>(h, X, (int)N, (int)K, w));
    int* host = nullptr;
    DCP_TRY(ksvd_read_counts(h, w.meta, (int)K, coder.it_dev(), &host));
    *it_out = host[K + 4];
    if (host[0] > n_nonzero) return fail(h, DCP_ERR_INTERNAL, "ksvd: the coder returned a row beyond the sparsity");
    const KsvdMask<real_t<T>> m{M, mask_ndim == 2 ? (long)F : 0L};
    DCP_TRY(ksvd_sweep<T>(h, Y, m, X, D, (int)N, (int)F, (int)K, host + 4, w));
    if (!clean) return ksvd_read_maxdiff(h, w.mdpart, (long)K * F, maxdiff_out);
    DCP_TRY(ksvd_clean_mark<T>(h, (const T*)X, (const T*)D, (int)N, (int)F, (int)K, clean->max_coherence, w, c));
    DCP_TRY(ksvd_clean_read<T>(h, w, c, (long)K * F, maxdiff_out, clean->n_marked_out));
    if (*clean->n_marked_out > 0 && *maxdiff_out >= clean->stop_tol)
        DCP_TRY(ksvd_clean_apply<T>(h, Y, m, (const T*)X, D, (int)N, (int)F, (int)K, *clean->n_marked_out, w, c));
    return DCP_OK;
}

// dcp_ksvd_clean_step_*: the step with the cleaning pass behind it; masked is whether a mask was given
template <class T>
inline int ksvd_clean_step_api(dcp_handle* h, const T* Y, const real_t<T>* M, int mask_ndim, T* X, T* D, int64_t N,
                               int64_t F, int64_t K, int n_nonzero, double coef_tol, int rows_per_pass,
                               double* maxdiff_out, int* it_out, double max_coherence, double stop_tol,
                               int* n_marked_out) {
    const KsvdCleanCall clean{max_coherence, stop_tol, n_marked_out};
    return ksvd_step_api<T>(h, Y, M, mask_ndim, M != nullptr || mask_ndim != 0, X, D, N, F, K, n_nonzero, coef_tol,
                            rows_per_pass, maxdiff_out, it_out, &clean);
}

}  // namespace dcp
