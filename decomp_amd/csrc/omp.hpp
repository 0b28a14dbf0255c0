// Orthogonal matching pursuit in Gram form ("batch OMP", Rubinstein, Zibulevsky & Elad 2008):
//
//   min |y - x A|^2  s.t.  |x|_0 <= s        for every row y [F] of Y [N, F], A [K, F]
//
// With alpha0 = y A^H [K], G = A A^H [K, K], n_k = sqrt(G_kk), support I = (), x = 0, at most s times:
//   1. tol given and |r|^2 <= tol: stop             |r|^2 = |y|^2 - Re(x_I . conj(alpha0_I))
//   2. alpha_k = alpha0_k - sum_j x_j G[I_j, k]     (= r . a_k^H; the [N, F] residual is never formed)
//      c_k = |alpha_k| / n_k over k not in I with n_k > 0; k* = the LOWEST index attaining the maximum;
//      maximum <= 0 (or NaN): stop
//   3. L w = G[I, k*] (L: the Cholesky factor of G_II), d = G_k*k* - |w|^2;
//      d <= eps_dep G_k*k* (a_k* numerically in the span of A_I): stop, keeping the previous x
//   4. I <- I + (k*); L gains the row (w^H, sqrt(d)); x_I G_II = alpha0_I through L z = conj(alpha0_I) (only
//      z's last entry is new), L^H v = z, x_I = conj(v)
// The coefficients are those for the caller's A (y ~ x A); the selection is invariant to the scaling of the atoms.
//
// eps_dep = 4096 eps (omp_eps_dep in greedy.hpp, with the reason).
//
// Kernel.  64-thread workgroups, one wave; the wave owns one row at a time and walks the rows grid-stride.  Every
// branch of the greedy loop is wave-uniform (the stop decisions are formed from butterfly reductions that leave the
// same value in all 64 lanes, and pass through readfirstlane); a workgroup is one wave, so rows that stop at different
// steps cannot wait for each other.  No atomics except one integer max per wave for the step count; every sum has a
// fixed order, so results are bitwise reproducible.
//   selection   each lane takes the correlations k = lane, lane + 64, ... (greedy_lane_best), then the butterfly on
//               (value, index) of greedy.hpp.  alpha is not stored: a lane forms alpha_k from alpha0_k and the rows
//               G[I_j, :] (row I_j is contiguous in k: coalesced; G is Hermitian, row I_j holds a_Ij . a_k^H as
//               needed, no conjugate) right where it scores it.
//   L           the OmpFactor of greedy.hpp in the wave's LDS (OmpCarve); z, x and 1 / L_jj live in lane j's registers.
//   alpha0      tier 0, K <= 512 (kOmpRegK): in registers, 1 / 2 / 4 / 8 per lane, with 1 / n_k beside them
//               tier 1, K <= 2048 (kOmpLdsK): the row's alpha0 in LDS
//               tier 2, above: read from the global [N, K] alpha0 itself at every step (L2)
// Limits: s <= 64 real, s <= 32 complex (the LDS image of L; the split of atom_blk()); any K >= 1.
#pragma once
#include <hip/hip_runtime.h>

#include "greedy.hpp"
#include "lasso_impl.hpp"

namespace dcp {

constexpr int kOmpRegK = 512;    // alpha0 in registers up to this K (8 per lane)
constexpr int kOmpLdsK = 2048;   // alpha0 in LDS up to this K; the global alpha0 above
constexpr int kOmpChunk = 4;     // correlations per lane and pass in tiers 1 and 2

template <class T>
constexpr int omp_cap() { return scalar_traits<T>::is_complex ? 32 : 64; }

__device__ __forceinline__ float  omp_mag(float a)  { return fabsf(a); }
__device__ __forceinline__ double omp_mag(double a) { return fabs(a); }
template <class R>
__device__ __forceinline__ R omp_mag(cx<R> a) { return sqrt(abs2(a)); }

// Scores U correlations of this lane, k = kbase + 64 q + lane: alpha_k = a0[q] - sum_j xs[j] G[sel[j], k], masked out
// where k >= K, k is in the support or n_k = 0; keeps the lane's best (bc, bk), lower k on ties.
template <class T, int U>
__device__ __forceinline__ void omp_score(const T (&a0)[U], const real_t<T> (&inv)[U], int kbase, int lane,
                                          const T* __restrict__ G, int K, int n, const T* xs, const int* sel,
                                          real_t<T>& bc, int& bk) {
    typedef real_t<T> R;
    T a[U];
    int kq[U], kc[U];
    bool hit[U];
#pragma unroll
    for (int q = 0; q < U; ++q) {
        kq[q] = kbase + 64 * q + lane;
        kc[q] = kq[q] < K ? kq[q] : K - 1;
        a[q] = a0[q];
        hit[q] = false;
    }
#pragma unroll 2
    for (int j = 0; j < n; ++j) {
        const T xj = xs[j];       // LDS, one address for the wave: a broadcast
        const int ij = sel[j];
        const T* g = G + (long)ij * K;
#pragma unroll
        for (int q = 0; q < U; ++q) {
            a[q] = fmsub(a[q], xj, g[kc[q]]);
            hit[q] = hit[q] || ij == kq[q];
        }
    }
#pragma unroll
    for (int q = 0; q < U; ++q)
        greedy_lane_best(bc, bk, omp_mag(a[q]) * inv[q], !hit[q] && kq[q] < K && inv[q] > R(0), kq[q]);
}

// grid: any; one 64-thread workgroup walks rows blockIdx.x, blockIdx.x + gridDim.x, ...
// TIER 0: K <= 64 NPL; dynamic LDS OmpCarve<T>(s, TIER == 1 ? K : 0).bytes.  ynorm2 is read only when tol >= 0.
// *it_max (zero on entry) receives the largest support size.
template <class T, int TIER, int NPL>
__global__ void __launch_bounds__(64) omp_greedy_kernel(const T* __restrict__ alpha0, const T* __restrict__ G,
                                                        const real_t<T>* __restrict__ invn,
                                                        const real_t<T>* __restrict__ ynorm2, T* __restrict__ X,
                                                        int N, int K, int s, real_t<T> tol, int* __restrict__ it_max) {
    typedef real_t<T> R;
    extern __shared__ __attribute__((aligned(16))) unsigned char omp_lds[];
    const int lane = threadIdx.x;
    const OmpCarve<T> cv(s, TIER == 1 ? K : 0);
    T* xs = reinterpret_cast<T*>(omp_lds + cv.xs);
    T* a0s = reinterpret_cast<T*>(omp_lds + cv.a0s);   // tier 1 only
    int* sel = reinterpret_cast<int*>(omp_lds + cv.sel);
    OmpFactor<T> fac{reinterpret_cast<T*>(omp_lds), omp_ld(s), lane, lane < s ? lane : s - 1, 0};
    const bool use_tol = tol >= R(0);

    // tier 0: 1 / n_k of this lane's atoms, once per wave
    R invr[NPL];
    if constexpr (TIER == 0) {
#pragma unroll
        for (int q = 0; q < NPL; ++q) {
            const int k = 64 * q + lane;
            invr[q] = omp_keep(invn[k < K ? k : K - 1], k < K);
        }
    }
    int wave_max = 0;

    for (long row = blockIdx.x; row < N; row += gridDim.x) {
        const T* a0row = alpha0 + row * K;
        T a0r[NPL];
        if constexpr (TIER == 0) {
#pragma unroll
            for (int q = 0; q < NPL; ++q) {
                const int k = 64 * q + lane;
                a0r[q] = omp_keep(a0row[k < K ? k : K - 1], k < K);
            }
        } else if constexpr (TIER == 1) {
            __syncthreads();   // the previous row's last reads of a0s
            for (int k = lane; k < K; k += 64) a0s[k] = a0row[k];
            __syncthreads();
        }
        const R yn2 = use_tol ? ynorm2[row] : R(0);
        R r2 = yn2;
        int n = 0;             // support size, wave-uniform
        int my_sel = 0;        // lane j < n: I_j
        T z = zero_of<T>();    // lane j < n: z_j of L z = conj(alpha0_I)
        T x = zero_of<T>();    // lane j < n: x_j
        T a0sel = zero_of<T>();   // lane j < n: alpha0_{I_j}
        R dinv = R(0);         // lane j < n: 1 / L_jj

        while (n < s) {
            if (use_tol && __builtin_amdgcn_readfirstlane((int)!(r2 > tol))) break;   // |r|^2 <= tol (or NaN)
            // ---- selection ----
            R bc = R(-1);
            int bk = 0x7fffffff;
            if constexpr (TIER == 0) {
                omp_score<T, NPL>(a0r, invr, 0, lane, G, K, n, xs, sel, bc, bk);
            } else {
                for (int kb = 0; kb < K; kb += 64 * kOmpChunk) {
                    T a0c[kOmpChunk];
                    R invc[kOmpChunk];
#pragma unroll
                    for (int q = 0; q < kOmpChunk; ++q) {
                        const int k = kb + 64 * q + lane, kk = k < K ? k : K - 1;
                        a0c[q] = TIER == 1 ? a0s[kk] : a0row[kk];
                        invc[q] = invn[kk];
                    }
                    omp_score<T, kOmpChunk>(a0c, invc, kb, lane, G, K, n, xs, sel, bc, bk);
                }
            }
            greedy_wave_best(bc, bk);
            if (__builtin_amdgcn_readfirstlane((int)!(bc > R(0)))) break;   // nothing correlates
            const int kstar = __builtin_amdgcn_readfirstlane(bk);
            // ---- the Cholesky pivot: L w = G[I, k*] ----
            const R gkk = real_part(G[(long)kstar * K + kstar]);
            const T a0k = a0row[kstar];
            fac.n = n;
            R wn2;
            const T w = fac.forward(omp_keep(G[(long)my_sel * K + kstar], lane < n), dinv, wn2);
            const R d = gkk - wn2;
            if (__builtin_amdgcn_readfirstlane((int)fac.dependent(d, gkk))) break;   // keep the previous x
            // ---- accept: row n of L, z_n, then L^H v = z ----
            const R ldiag = sqrt(d), rdiag = R(1) / ldiag;
            const T wc = omp_keep(conj_of(w), lane < n);
            {
                const T zn_part = wave_sum_all(omp_keep(mul(wc, z), lane < n));   // sum_{m<n} L[n][m] z_m
                const T zn = scale(sub(conj_of(a0k), zn_part), rdiag);
                fac.accept(wc, ldiag);
                if (lane == n) {
                    sel[n] = kstar;
                    my_sel = kstar;
                    a0sel = a0k;
                    dinv = rdiag;
                    z = zn;
                }
            }
            __syncthreads();
            x = conj_of(fac.backward(z, dinv, wc));
            if (lane <= n) xs[lane] = x;   // (the scoring loop's reads of xs lie before the barrier above)
            ++n;
            __syncthreads();
            if (use_tol) r2 = yn2 - real_part(wave_sum_all(omp_keep(mul(x, conj_of(a0sel)), lane < n)));
        }

        // ---- the row of X, zeros off the support ----
        omp_scatter_row(sel, xs, n, X + row * K, K, lane);
        wave_max = n > wave_max ? n : wave_max;
        __syncthreads();   // the next row's writes to xs / sel after this row's reads
    }
    if (lane == 0 && wave_max > 0) atomicMax(it_max, wave_max);
}

// invn[k] = 1 / sqrt(G_kk) where G_kk > 0, else 0 (such an atom is never selected); clears *it_zero.
template <class T>
__global__ void __launch_bounds__(256) omp_invnorm_kernel(const T* __restrict__ G, int K, real_t<T>* __restrict__ invn,
                                                          int* __restrict__ it_zero) {
    typedef real_t<T> R;
    if (blockIdx.x == 0 && threadIdx.x == 0) *it_zero = 0;
    for (long k = blockIdx.x * 256L + threadIdx.x; k < K; k += (long)gridDim.x * 256L) {
        const R g = real_part(G[k * K + k]);
        invn[k] = g > R(0) ? R(1) / sqrt(g) : R(0);
    }
}

// out[row] = |Y[row, :]|^2, one 256-thread workgroup per row
template <class T>
__global__ void __launch_bounds__(256) omp_rownorm2_kernel(const T* __restrict__ Y, long F,
                                                           real_t<T>* __restrict__ out) {
    typedef real_t<T> R;
    __shared__ R sh[4];
    const T* y = Y + (long)blockIdx.x * F;
    R acc = 0;
    for (long j = threadIdx.x; j < F; j += 256) acc += abs2(y[j]);
    const R tot = block_sum_256(acc, sh);
    if (threadIdx.x == 0) out[blockIdx.x] = tot;
}

template <class T, int TIER, int NPL>
inline hipError_t launch_omp_cfg(hipStream_t st, const T* alpha0, const T* G, const real_t<T>* invn,
                                 const real_t<T>* ynorm2, T* X, int N, int K, int s, real_t<T> tol, int* it_dev) {
    const int grid = N < 8192 ? N : 8192;
    hipLaunchKernelGGL((omp_greedy_kernel<T, TIER, NPL>), dim3(grid), dim3(64), OmpCarve<T>(s, TIER == 1 ? K : 0).bytes, st,
                       alpha0, G, invn, ynorm2, X, N, K, s, tol, it_dev);
    return hipGetLastError();
}

// The greedy kernel on alpha0 [N, K], G [K, K], ynorm2 [N] (read only when tol >= 0); invn [K] and it_dev are
// workspace.  Enqueues only: *it_dev holds the largest support size once the stream has run.
template <class T>
inline int omp_greedy(dcp_handle* h, const T* alpha0, const T* G, const real_t<T>* ynorm2, T* X, int N, int K, int s,
                      double tol, real_t<T>* invn, int* it_dev) {
    typedef real_t<T> R;
    hipStream_t st = h->stream;
    hipLaunchKernelGGL((omp_invnorm_kernel<T>), dim3(grid_for(K)), dim3(256), 0, st, G, K, invn, it_dev);
    DCP_LAUNCH_OK(h, hipGetLastError());
    const R t = tol >= 0.0 ? (R)tol : R(-1);
    hipError_t e;
    if (K <= 64) e = launch_omp_cfg<T, 0, 1>(st, alpha0, G, invn, ynorm2, X, N, K, s, t, it_dev);
    else if (K <= 128) e = launch_omp_cfg<T, 0, 2>(st, alpha0, G, invn, ynorm2, X, N, K, s, t, it_dev);
    else if (K <= 256) e = launch_omp_cfg<T, 0, 4>(st, alpha0, G, invn, ynorm2, X, N, K, s, t, it_dev);
    else if (K <= kOmpRegK) e = launch_omp_cfg<T, 0, 8>(st, alpha0, G, invn, ynorm2, X, N, K, s, t, it_dev);
    else if (K <= kOmpLdsK) e = launch_omp_cfg<T, 1, 1>(st, alpha0, G, invn, ynorm2, X, N, K, s, t, it_dev);
    else e = launch_omp_cfg<T, 2, 1>(st, alpha0, G, invn, ynorm2, X, N, K, s, t, it_dev);
    DCP_LAUNCH_OK(h, e);
    return DCP_OK;
}

// ---- workspace: the fields of LassoWs the solve uses (the dictionary step lays them out with the same function) ----
template <class T>
inline void omp_layout(WsLayout& a, LassoWs<T>& w, int64_t N, int64_t F, int64_t K) {
    a.take(w.yAt, (size_t)N * K);                 // alpha0
    a.take(w.AAt, (size_t)K * K);                 // G
    w.slab_count = (size_t)kMaxSplits * K * K;    // split-K partials of G
    a.take(w.slabs, w.slab_count);
    a.take(w.s, (size_t)K);                       // 1 / n_k
    a.take(w.rowscale, (size_t)N);                // |y|^2
    a.take(w.flag, 4);
    if (scalar_traits<T>::is_complex) a.take(w.ext1, (size_t)4 * K * F);
}

// `what` is the refused parameter with its entry's family, `size` the name of the number of atoms, in the message
inline int omp_check_sparsity(dcp_handle* h, int64_t K, int64_t n_nonzero, int cap, const char* what = "omp: n_nonzero",
                              const char* size = "K") {
    if (n_nonzero < 1 || n_nonzero > cap || n_nonzero > K)
        return fail(h, DCP_ERR_INVALID, std::string(what) + " must be in [1, min(" + size + ", " + std::to_string(cap) +
                                            ")] (the cap is 64 for real and 32 for complex dtypes)");
    return DCP_OK;
}

// Both products on the GEMM cores, then the greedy kernel.  Enqueues only; w.flag[0] holds the step count.
template <class T>
inline int omp_solve(dcp_handle* h, const T* Y, const T* A, T* X, int N, int F, int K, int s, double tol,
                     LassoWs<T>& w) {
    typedef real_t<T> R;
    hipStream_t st = h->stream;
    {   // alpha0 = Y A^H
        GemmArgs<T> a;
        a.A = Y; a.lda = F; a.B = A; a.ldb = F; a.M = N; a.N = K; a.K = F; a.conjB = true;
        a.ext_ws = w.ext1;
        DCP_LAUNCH_OK(h, (gemm<FORM_NT>(st, a, EpiStore<T>{w.yAt, K})));
    }
    DCP_TRY(gram_kk<T>(h, A, A, K, F, w, w.AAt));   // G = A A^H
    if (tol >= 0.0) {
        hipLaunchKernelGGL((omp_rownorm2_kernel<T>), dim3(N), dim3(256), 0, st, Y, (long)F, w.rowscale);
        DCP_LAUNCH_OK(h, hipGetLastError());
    }
    return omp_greedy<T>(h, (const T*)w.yAt, (const T*)w.AAt, (const R*)w.rowscale, X, N, K, s, tol, w.s, w.flag);
}

// *it_out = the device word, after the stream has run
inline int omp_read_it(dcp_handle* h, const int* it_dev, int* it_out) { return read_scalar(h, it_dev, it_out); }

// The argument checks every OMP and K-SVD entry shares, in this order: sizes, tol, sparsity.  An entry without a
// channel axis (omp_gram_api) passes F = 1; one without a coder (the K-SVD sweep) takes the sizes part alone.
inline int omp_check_sizes(dcp_handle* h, int64_t N, int64_t F, int64_t K) {
    if (N <= 0 || F <= 0 || K <= 0) return fail(h, DCP_ERR_INVALID, "sizes must be positive");
    if (N > 0x7fffffffLL || F > 0x7fffffffLL || K > 0x7fffffffLL)
        return fail(h, DCP_ERR_INVALID, "dimension exceeds 2^31-1");
    return DCP_OK;
}

// ynorm2_missing: omp_gram_api's tol >= 0 without the row norms, refused where it always was (before the sparsity)
template <class T>
inline int omp_check_problem(dcp_handle* h, int64_t N, int64_t F, int64_t K, int n_nonzero, double tol,
                             bool ynorm2_missing = false) {
    DCP_TRY(omp_check_sizes(h, N, F, K));
    if (tol != tol) return fail(h, DCP_ERR_INVALID, "omp: tol is NaN");
    if (ynorm2_missing) return fail(h, DCP_ERR_INVALID, "omp: ynorm2 is null but tol >= 0");
    return omp_check_sparsity(h, K, n_nonzero, omp_cap<T>());
}

template <class T>
inline int omp_gram_api(dcp_handle* h, const T* alpha0, const T* G, const real_t<T>* ynorm2, T* X, int64_t N,
                        int64_t K, int n_nonzero, double tol, int* it_out) {
    typedef real_t<T> R;
    if (!h) return DCP_ERR_INVALID;
    if (!alpha0 || !G || !X || !it_out) return fail(h, DCP_ERR_INVALID, "null pointer");
    DCP_TRY(omp_check_problem<T>(h, N, 1, K, n_nonzero, tol, tol >= 0.0 && !ynorm2));
    DCP_HIP_OK(h, hipSetDevice(h->device));
    R* invn = nullptr;
    int* it_dev = nullptr;
    DCP_TRY(ws_lay_out(h, [&](WsLayout& a) {
        a.take(invn, (size_t)K);
        a.take(it_dev, 4);
    }));
    DCP_TRY(omp_greedy<T>(h, alpha0, G, ynorm2, X, (int)N, (int)K, n_nonzero, tol, invn, it_dev));
    return omp_read_it(h, it_dev, it_out);
}

}  // namespace dcp
