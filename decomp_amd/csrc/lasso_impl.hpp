// Batched LASSO / NNLS inner solves on the device (float, double, complex64, complex128).
//
// Reference path restated as kernels:
//   decomp/lasso.py:97-189    solve_fastpath: row-normalise A, rescale alpha / tol / x
//   decomp/lasso.py:192-241   soft thresholds (real, complex, positive)
//   decomp/lasso.py:244-271   one proximal-gradient step, plain and masked
//   decomp/lasso.py:274-445   ista / acc_ista / fista (+ 2-D mask variants)
//   decomp/lasso.py:526-583   coordinate descent (+ mask variant)
//   decomp/math_utils/eigen.py:9-20  Gershgorin bound
//
// Structure on the GPU: the per-iteration x.AAt product is the GEMM; everything the
// reference does elementwise around it (gradient, step, soft threshold, momentum
// extrapolation, |dx| - tol stop test) is the GEMM's epilogue, so one iteration is ONE
// kernel (two when a 2-D mask forces the chained (x A o M) A^H form).  The step size
// 1/L stays on the device; the host only reads a 4-byte flag on every 10th iteration,
// exactly where the reference evaluates its stop test.
// Coordinate descent uses the Gram form (rows of A are unit norm, lasso.py:528):
//   g = y A^H - x AAt;  x_k <- S(g_k + x_k AAt_kk, alpha_k);  g -= dx_k AAt[k, :]
// which is what lasso.py:539-548 computes, at 2NK^2 instead of 2NKF.K flops per sweep.
#pragma once
#include <math.h>

#include "gemm.hpp"
#include "handle.hpp"
#include "kernels_small.hpp"
#include "nmf_impl.hpp"  // kMaxSplits, column_sums
#include "lasso_extra.hpp"  // parallel_cd and admm kernels
#include "prox_loop.hpp"    // prox_gradient_loop, flag_publish_kernel, poll_host_flag

namespace dcp {

enum { PROX_REAL = 0, PROX_COMPLEX = 1, PROX_POSITIVE = 2 };

// ---- proximal operators ------------------------------------------------------------------
template <int PROX, class T>
__device__ __forceinline__ T prox_apply(T z, real_t<T> thr) {
    typedef real_t<T> R;
    if constexpr (scalar_traits<T>::is_complex) {
        // lasso.py:223-225: max(|z| - t, 0) * z / (|z| + 1e-15)
        const R r = absval(z);
        const R m = max_np(r - thr, R(0));
        const R den = r + R(1.0e-15);
        T sgn;
        sgn.re = z.re / den;
        sgn.im = z.im / den;
        return scale(sgn, m);
    } else {
        if (PROX == PROX_POSITIVE) {  // lasso.py:241
            const T v = z - thr;
            return max_np(v, T(0));
        }
        // lasso.py:206-207: max(|z| - t, 0) * sign(z)
        const T m = max_np(absval(z) - thr, T(0));
        const T sg = z > T(0) ? T(1) : (z < T(0) ? T(-1) : (z == T(0) ? T(0) : z /*NaN*/));
        return m * sg;
    }
}

// ---- epilogues -------------------------------------------------------------------------------
// One proximal-gradient step fused into the GEMM that yields back = v.AAt (or (vA o M)A^H):
//   z = v + Linv * (yAt - back) ; x_new = S(z, Linv*alpha_k [* rowscale_n]) ;
//   v_next = x_new + coef * (x_new - x_prev) ; violation flag |x_new - x_prev| - tol_k >= 0
template <class T, int PROX>
struct EpiProxStep {
    typedef real_t<T> R;
    const T* yAt;
    const T* v;
    const T* xprev;
    T* xnew;
    T* vnext;  // nullable (plain ista)
    long ld;
    const R* Linv;      // device scalar
    const R* alpha;     // [K]
    const R* tolk;      // [K]
    const R* rowscale;  // nullable [N]  (2-D mask: sum_f mask[n, f])
    R coef;
    int check;
    int* flag;
    __device__ __forceinline__ void operator()(int r, int c, T back, int) const {
        const long i = (long)r * ld + c;
        const R li = Linv[0];
        const T z = add(v[i], scale(sub(yAt[i], back), li));
        R thr = li * alpha[c];
        if (rowscale != nullptr) thr = li * (alpha[c] * rowscale[r]);
        const T xn = prox_apply<PROX>(z, thr);
        xnew[i] = xn;
        const T d = sub(xn, xprev[i]);
        if (vnext != nullptr) vnext[i] = add(xn, scale(d, coef));
        if (check && !((absval(d) - tolk[c]) < R(0))) *flag = 1;
    }
    // float32: the same step on 4 consecutive columns of a row (16-byte loads of y.A^H, v, x_prev and
    // stores of x_new / v_next: the epilogue reads three arrays per element, see epi_vec4)
    static constexpr bool kVec4 = std::is_same<T, float>::value;
    bool vec_ok() const { return aligned16(yAt, v, xprev, xnew, alpha, tolk, vnext, ld); }
    __device__ __forceinline__ void vec4(int r, int c0, f32x4 back, int) const {
        if constexpr (std::is_same<T, float>::value) {
            const long i = (long)r * ld + c0;
            const float li = Linv[0];
            const f32x4 y4 = load4(yAt + i);
            const f32x4 v4 = load4(v + i);
            const f32x4 p4 = load4(xprev + i);
            const f32x4 a4 = load4(alpha + c0);
            const float rs = rowscale != nullptr ? rowscale[r] : 1.0f;
            f32x4 xn, vn;
            bool viol = false;
#pragma unroll
            for (int e = 0; e < 4; ++e) {
                const float z = v4[e] + (y4[e] - back[e]) * li;
                float thr = li * a4[e];
                if (rowscale != nullptr) thr = li * (a4[e] * rs);
                xn[e] = prox_apply<PROX>(z, thr);
                const float d = xn[e] - p4[e];
                vn[e] = xn[e] + d * coef;
                if (check && !((fabsf(d) - tolk[c0 + e]) < 0.0f)) viol = true;
            }
            store4(xnew + i, xn);
            if (vnext != nullptr) store4(vnext + i, vn);
            if (viol) *flag = 1;
        }
    }
    // complex64: two consecutive columns of a row (16 bytes) per call, see CplxColEpi
    static constexpr bool kCVec2 = std::is_same<T, c64>::value;
    bool cvec_ok() const { return aligned16<2>(yAt, v, xprev, xnew, vnext, ld); }
    __device__ __forceinline__ void cvec2(int r, int c0, f32x4 back, int) const {
        if constexpr (std::is_same<T, c64>::value) {
            const long i = (long)r * ld + c0;
            const float li = Linv[0];
            const f32x4 y4 = load4(yAt + i);
            const f32x4 v4 = load4(v + i);
            const f32x4 p4 = load4(xprev + i);
            const float rs = rowscale != nullptr ? rowscale[r] : 1.0f;
            f32x4 xn4, vn4;
            bool viol = false;
#pragma unroll
            for (int e = 0; e < 2; ++e) {
                const c64 bk{back[2 * e], back[2 * e + 1]};
                const c64 z = add(c64{v4[2 * e], v4[2 * e + 1]}, scale(sub(c64{y4[2 * e], y4[2 * e + 1]}, bk), li));
                float thr = li * alpha[c0 + e];
                if (rowscale != nullptr) thr = li * (alpha[c0 + e] * rs);
                const c64 xn = prox_apply<PROX>(z, thr);
                const c64 d = sub(xn, c64{p4[2 * e], p4[2 * e + 1]});
                const c64 vn = add(xn, scale(d, coef));
                xn4[2 * e] = xn.re; xn4[2 * e + 1] = xn.im;
                vn4[2 * e] = vn.re; vn4[2 * e + 1] = vn.im;
                if (check && !((absval(d) - tolk[c0 + e]) < 0.0f)) viol = true;
            }
            store4(xnew + i, xn4);
            if (vnext != nullptr) store4(vnext + i, vn4);
            if (viol) *flag = 1;
        }
    }
};

// The same step in the "H form" (no 2-D mask):  with H = I - Linv A A^H and r = Linv y A^H, both formed ONCE per
// solve,   v + Linv (y A^H - v A A^H) = v H + r ,   so the epilogue of the v.H product reads ONE [N, K] array (r)
// instead of three (y A^H, v, x_prev) -- x_prev is only touched when the iteration needs x_new - x_prev (momentum,
// or the stop test of iterations 0, 10, ...).  One launch of the dictionary step's 8192 x 512 x 512 iteration is a
// single lock-step round of workgroups (main loop, then epilogue, nothing to overlap them with), so its [N, K]
// epilogue traffic is exposed time: 84 MB -> 34 MB per launch.  Same fixed point, same iterates up to rounding
// (the Gram-form remark of DESIGN.md section 2 applies: a re-association of lasso.py:248-256).
template <class T, int PROX>
struct EpiProxStepH {
    typedef real_t<T> R;
    const T* rs;        // Linv * yAt
    const T* xprev;     // read only when need_prev
    T* xnew;
    T* vnext;           // nullable (plain ista)
    long ld;
    const R* Linv;      // device scalar
    const R* alpha;     // [K]
    const R* tolk;      // [K]
    R coef;
    int check;
    int need_prev;      // check != 0 or vnext != nullptr
    int* flag;
    // last iteration of a solve that returns its latest iterate (ista, fista): x_new / s goes straight to the
    // caller's array (lasso.py:189), one elementwise pass fewer
    T* xfinal = nullptr;
    const R* sdiv = nullptr;
    __device__ __forceinline__ static T unscale(T v, R sk) {
        if constexpr (scalar_traits<T>::is_complex) { v.re = v.re / sk; v.im = v.im / sk; }
        else v = v / sk;
        return v;
    }
    __device__ __forceinline__ void operator()(int r, int c, T back, int) const {
        const long i = (long)r * ld + c;
        const T z = add(back, rs[i]);
        const T xn = prox_apply<PROX>(z, Linv[0] * alpha[c]);
        xnew[i] = xn;
        if (xfinal != nullptr) xfinal[i] = unscale(xn, sdiv[c]);
        if (need_prev) {
            const T d = sub(xn, xprev[i]);
            if (vnext != nullptr) vnext[i] = add(xn, scale(d, coef));
            if (check && !((absval(d) - tolk[c]) < R(0))) *flag = 1;
        }
    }
    static constexpr bool kVec4 = std::is_same<T, float>::value;
    bool vec_ok() const {
        return aligned16(rs, xprev, xnew, alpha, tolk, vnext, ld) && (xfinal == nullptr || aligned16(xfinal, sdiv));
    }
    __device__ __forceinline__ void vec4(int r, int c0, f32x4 back, int) const {
        if constexpr (std::is_same<T, float>::value) {
            const long i = (long)r * ld + c0;
            const float li = Linv[0];
            const f32x4 r4 = load4(rs + i);
            const f32x4 a4 = load4(alpha + c0);
            f32x4 xn;
#pragma unroll
            for (int e = 0; e < 4; ++e) xn[e] = prox_apply<PROX>(back[e] + r4[e], li * a4[e]);
            store4(xnew + i, xn);
            if (xfinal != nullptr) {
                const f32x4 s4 = load4(sdiv + c0);
                f32x4 xf;
#pragma unroll
                for (int e = 0; e < 4; ++e) xf[e] = xn[e] / s4[e];
                store4(xfinal + i, xf);
            }
            if (need_prev) {
                const f32x4 p4 = load4(xprev + i);
                f32x4 vn;
                bool viol = false;
#pragma unroll
                for (int e = 0; e < 4; ++e) {
                    const float d = xn[e] - p4[e];
                    vn[e] = xn[e] + d * coef;
                    if (check && !((fabsf(d) - tolk[c0 + e]) < 0.0f)) viol = true;
                }
                if (vnext != nullptr) store4(vnext + i, vn);
                if (viol) *flag = 1;
            }
        }
    }
    static constexpr bool kCVec2 = std::is_same<T, c64>::value;
    bool cvec_ok() const { return aligned16<2>(rs, xprev, xnew, vnext, xfinal, ld); }
    __device__ __forceinline__ void cvec2(int r, int c0, f32x4 back, int) const {
        if constexpr (std::is_same<T, c64>::value) {
            const long i = (long)r * ld + c0;
            const float li = Linv[0];
            const f32x4 r4 = load4(rs + i);
            f32x4 xn4;
            c64 xn[2];
#pragma unroll
            for (int e = 0; e < 2; ++e) {
                const c64 z{back[2 * e] + r4[2 * e], back[2 * e + 1] + r4[2 * e + 1]};
                xn[e] = prox_apply<PROX>(z, li * alpha[c0 + e]);
                xn4[2 * e] = xn[e].re; xn4[2 * e + 1] = xn[e].im;
            }
            store4(xnew + i, xn4);
            if (xfinal != nullptr) {
                const float s0 = sdiv[c0], s1 = sdiv[c0 + 1];
                const f32x4 xf = {xn4[0] / s0, xn4[1] / s0, xn4[2] / s1, xn4[3] / s1};
                store4(xfinal + i, xf);
            }
            if (need_prev) {
                const f32x4 p4 = load4(xprev + i);
                f32x4 vn4;
                bool viol = false;
#pragma unroll
                for (int e = 0; e < 2; ++e) {
                    const c64 d = sub(xn[e], c64{p4[2 * e], p4[2 * e + 1]});
                    const c64 vn = add(xn[e], scale(d, coef));
                    vn4[2 * e] = vn.re; vn4[2 * e + 1] = vn.im;
                    if (check && !((absval(d) - tolk[c0 + e]) < 0.0f)) viol = true;
                }
                if (vnext != nullptr) store4(vnext + i, vn4);
                if (viol) *flag = 1;
            }
        }
    }
};

// AAt <- I - Linv AAt (in place, [K, K]), yAt <- Linv yAt (in place, [N, K]): the H form's two operands; and, in the
// same pass over [N, K], the solver's starting point xs = x * s (lasso.py:131; xsrc null: already done)
template <class T>
__global__ void __launch_bounds__(256) hform_prepare_kernel(T* __restrict__ AAt, long K, T* __restrict__ yAt,
                                                            long nk, const real_t<T>* __restrict__ Linv,
                                                            const T* __restrict__ xsrc,
                                                            const real_t<T>* __restrict__ s, T* __restrict__ xs) {
    typedef real_t<T> R;
    const R li = Linv[0];
    const long kk = K * K;
    for (long i = blockIdx.x * 256L + threadIdx.x; i < kk + nk; i += (long)gridDim.x * 256L) {
        if (i < kk) {
            const long r = i / K, c = i - r * K;
            T h = scale(AAt[i], -li);
            if (r == c) h = add(h, from_real<T>(R(1)));
            AAt[i] = h;
        } else {
            const long j = i - kk;
            yAt[j] = scale(yAt[j], li);
            if (xsrc != nullptr) xs[j] = scale(xsrc[j], s[j % K]);
        }
    }
}

// out = base - acc   (g = yAt - x.AAt for coordinate descent)
template <class T>
struct EpiSubFrom {
    const T* base;
    long ld_base;
    T* out;
    long ld_out;
    __device__ __forceinline__ void operator()(int r, int c, T v, int) const {
        out[(long)r * ld_out + c] = sub(base[(long)r * ld_base + c], v);
    }
};

// out = base - acc * mask   (r = y o M - (x A) o M for masked coordinate descent)
template <class T>
struct EpiMaskedResidual {
    const T* base;
    const real_t<T>* mask;
    T* out;
    long ld;
    __device__ __forceinline__ void operator()(int r, int c, T v, int) const {
        const long i = (long)r * ld + c;
        out[i] = sub(base[i], scale(v, mask[i]));
    }
};

// ---- small kernels -----------------------------------------------------------------------------
// alpha_k = (alpha / s_k) * nvalid ;  tol_k = tol * s_k        (lasso.py:129-130,135-138)
template <class R>
__global__ void __launch_bounds__(256) lasso_scalars_kernel(const R* __restrict__ s, long K, R alpha,
                                                            R tol, const R* __restrict__ nvalid_dev,
                                                            R nvalid_const, R* __restrict__ alphak,
                                                            R* __restrict__ tolk, int* __restrict__ flag_zero) {
    if (blockIdx.x == 0 && threadIdx.x == 0) *flag_zero = 0;   // the stop flag starts every solve cleared
    const R nv = nvalid_dev != nullptr ? nvalid_dev[0] : nvalid_const;
    for (long k = blockIdx.x * 256L + threadIdx.x; k < K; k += (long)gridDim.x * 256L) {
        alphak[k] = (alpha / s[k]) * nv;
        tolk[k] = tol * s[k];
    }
}

// out[n, k] = x[n, k] * s[k]  (mul != 0)  or  x[n, k] / s[k]     (lasso.py:131,189)
template <class T>
__global__ void __launch_bounds__(256) col_scale_kernel(const T* __restrict__ x, const real_t<T>* __restrict__ s,
                                                        long rows, long K, int mul, T* __restrict__ out) {
    typedef real_t<T> R;
    const long n = rows * K;
    for (long i = blockIdx.x * 256L + threadIdx.x; i < n; i += (long)gridDim.x * 256L) {
        const long k = i % K;
        const R sk = s[k];
        T v = x[i];
        if (mul) {
            v = scale(v, sk);
        } else {
            if constexpr (scalar_traits<T>::is_complex) { v.re = v.re / sk; v.im = v.im / sk; }
            else v = v / sk;
        }
        out[i] = v;
    }
}

// Linv = 1 / max_j sum_i |AAt[i, j]|   (eigen.py:20, lasso.py:286), two stages:
// stage 1: partial[s, j] = sum over a stripe of rows of |AAt[i, j]|  (coalesced along j)
template <class T>
__global__ void __launch_bounds__(256) colabs_partial_kernel(const T* __restrict__ a, long K,
                                                             long rows_per_blk,
                                                             real_t<T>* __restrict__ partial) {
    typedef real_t<T> R;
    const long r0 = blockIdx.y * rows_per_blk;
    const long r1 = min(K, r0 + rows_per_blk);
    for (long c = blockIdx.x * 256L + threadIdx.x; c < K; c += (long)gridDim.x * 256L) {
        R acc = 0;
        for (long r = r0; r < r1; ++r) acc += absval(a[r * K + c]);
        partial[blockIdx.y * K + c] = acc;
    }
}
// stage 2 (one workgroup): column sums of the stripes in order, max over columns, inverse.
template <class R>
__global__ void __launch_bounds__(256) gershgorin_finish_kernel(const R* __restrict__ partial, long K,
                                                                int stripes, R* __restrict__ Linv) {
    __shared__ R sh[4];
    R best = 0;
    for (long j = threadIdx.x; j < K; j += 256) {
        // four interleaved running sums (a fixed order): with one, the loop is a chain of
        // dependent L2 round trips (measured 31 us at K = 512 for 128 KiB of partials)
        R a0 = 0, a1 = 0, a2 = 0, a3 = 0;
        int s = 0;
        for (; s + 15 < stripes; s += 16) {   // sixteen loads in flight, same four interleaved sums
            R v[16];
#pragma unroll
            for (int u = 0; u < 16; ++u) v[u] = partial[(long)(s + u) * K + j];
#pragma unroll
            for (int u = 0; u < 16; u += 4) {
                a0 += v[u];
                a1 += v[u + 1];
                a2 += v[u + 2];
                a3 += v[u + 3];
            }
        }
        for (; s + 3 < stripes; s += 4) {
            a0 += partial[(long)s * K + j];
            a1 += partial[(long)(s + 1) * K + j];
            a2 += partial[(long)(s + 2) * K + j];
            a3 += partial[(long)(s + 3) * K + j];
        }
        for (; s < stripes; ++s) a0 += partial[(long)s * K + j];
        const R acc = (a0 + a1) + (a2 + a3);
        best = max_np(acc, best);
    }
    R m = block_max_256(best, sh);
    if (threadIdx.x == 0) {
        Linv[0] = R(1) / m;
        Linv[2] = m;    // the bound itself (parallel_cd: p = int(K / bound), lasso.py:468)
    }
}

// out[f] = v[f] / count   (mean over the batch of the mask, lasso.py:300-303)
template <class R>
__global__ void __launch_bounds__(256) scale_vec_kernel(const R* __restrict__ v, long n, R divisor,
                                                        R* __restrict__ out) {
    for (long i = blockIdx.x * 256L + threadIdx.x; i < n; i += (long)gridDim.x * 256L)
        out[i] = v[i] / divisor;
}

// Coordinate-descent sweeps in Gram form.  One wave per row; lane l holds columns l + 64m of the
// row's x and g in registers, plus AAt_kk, alpha_k, tol_k of its columns.
//
// A coordinate whose update is a zero step (x_k unchanged) leaves g untouched, so it commutes
// with everything: per 64-column slot ALL lanes evaluate their candidate step at once, a ballot
// finds the first coordinate (in sweep order) that really moves, only that one is applied
// (g -= dx AAt[k, :], one coalesced row read) and the lanes behind it are re-evaluated.  The
// sequence of applied updates is exactly that of the sequential sweep (lasso.py:539-548); with
// sparse codes a sweep costs ~(#changed coordinates) steps instead of K.
// Sweeps [.., + nsweeps); the FIRST one is a check sweep when check_first != 0 (the reference tests on
// sweeps 0, 10, 20, ...).  `cond` (nullable): the flag of the check sweep launched just before -- zero means its
// test was met and the reference returned there (lasso.py:546-551), so this launch does nothing.
template <class T, int PROX, int MAXM>
__global__ void __launch_bounds__(256) cd_gram_kernel(T* __restrict__ X, T* __restrict__ G,
                                                      const T* __restrict__ AAt,
                                                      const real_t<T>* __restrict__ alphak,
                                                      const real_t<T>* __restrict__ tolk, long rows,
                                                      int K, int nsweeps, int check_first,
                                                      int* __restrict__ flag,
                                                      const int* __restrict__ cond) {
    typedef real_t<T> R;
    // the sweeps behind a check sweep whose test was met are not run (lasso.py:546-551 returns there): decided on
    // the device from the check sweep's flag, so the host does not have to read it before launching them
    if (cond != nullptr && *cond == 0) return;
    const int lane = threadIdx.x & 63;
    const long row = (long)blockIdx.x * 4 + (threadIdx.x >> 6);
    if (row >= rows) return;
    const int M = (K + 63) / 64;
    T x[MAXM], g[MAXM], akk[MAXM];
    R al[MAXM], tl[MAXM];
    // (loads are unconditional on a clamped column and selected afterwards: a load under a lane
    //  predicate becomes its own branch + full wait, i.e. one memory round trip per slot)
#pragma unroll
    for (int m = 0; m < MAXM; ++m) {
        const int c = lane + 64 * m;
        const bool ok = (m < M && c < K);
        const int cc = ok ? c : 0;
        const T xv = X[row * K + cc], gv = G[row * K + cc], av = AAt[(long)cc * K + cc];
        const R alv = alphak[cc], tlv = tolk[cc];
        x[m] = ok ? xv : zero_of<T>();
        g[m] = ok ? gv : zero_of<T>();
        akk[m] = ok ? av : zero_of<T>();
        al[m] = ok ? alv : R(0);
        tl[m] = ok ? tlv : R(1);
    }
    bool viol = false;
    for (int s = 0; s < nsweeps; ++s) {
        const bool check = check_first && (s == 0);
#pragma unroll
        for (int m = 0; m < MAXM; ++m) {
            if (m >= M) break;
            const int kend = min(64, K - 64 * m);
            int cursor = 0;   // lanes < cursor of this slot are final for this sweep
            while (true) {
                // candidate step of every lane's coordinate against the current g
                const T z = fmadd(g[m], x[m], akk[m]);
                const T xn = prox_apply<PROX>(z, al[m]);
                const T d = sub(xn, x[m]);
                const bool moves = (lane >= cursor) && (lane < kend) && (abs2(d) != R(0));
                const unsigned long long mask = __ballot(moves);
                if (mask == 0ull) {
                    // every remaining coordinate of the slot is a zero step: |0| - tol_k
                    if (check && lane >= cursor && lane < kend && !((R(0) - tl[m]) < R(0))) viol = true;
                    break;
                }
                const int kk = __ffsll((long long)mask) - 1;     // first moving coordinate
                if (check && lane >= cursor && lane < kk && !((R(0) - tl[m]) < R(0))) viol = true;
                const T dk = lane_get(d, kk);
                if (lane == kk) {
                    x[m] = xn;
                    if (check && !((absval(d) - tl[m]) < R(0))) viol = true;
                }
                const T* arow = AAt + (long)(64 * m + kk) * K;
                T ar[MAXM];   // the whole row in flight at once (one L2 round trip per applied step)
#pragma unroll
                for (int mm = 0; mm < MAXM; ++mm) {
                    const int c = lane + 64 * mm;
                    ar[mm] = arow[(mm < M && c < K) ? c : 0];
                }
#pragma unroll
                for (int mm = 0; mm < MAXM; ++mm) {
                    const int c = lane + 64 * mm;
                    const T gn = fmsub(g[mm], dk, ar[mm]);
                    g[mm] = (mm < M && c < K) ? gn : g[mm];
                }
                cursor = kk + 1;
            }
        }
    }
#pragma unroll
    for (int m = 0; m < MAXM; ++m) {
        const int c = lane + 64 * m;
        if (m < M && c < K) {
            X[row * K + c] = x[m];
            G[row * K + c] = g[m];
        }
    }
    if (__ballot(viol) != 0ull && lane == 0) *flag = 1;
}

// The same sweep for dictionaries wider than the register form's 2048 atoms (64 lanes x 32 slots): the
// row's x and g stay in global memory (their own row of X / G: L2-resident, touched by this wave only,
// every lane only ever reads and writes ITS columns c = lane (mod 64), so program order is the only
// ordering needed), one 64-column slot at a time lives in registers while its coordinates are swept, and
// an applied step updates the other slots' g by read-modify-write, eight slots in flight.  Arithmetic
// and update order are those of cd_gram_kernel (identical results where both apply).
template <class T, int PROX>
__global__ void __launch_bounds__(256) cd_gram_wide_kernel(T* __restrict__ X, T* __restrict__ G,
                                                           const T* __restrict__ AAt,
                                                           const real_t<T>* __restrict__ alphak,
                                                           const real_t<T>* __restrict__ tolk, long rows,
                                                           int K, int nsweeps, int check_first,
                                                           int* __restrict__ flag,
                                                           const int* __restrict__ cond) {
    typedef real_t<T> R;
    if (cond != nullptr && *cond == 0) return;   // (see cd_gram_kernel)
    const int lane = threadIdx.x & 63;
    const long row = (long)blockIdx.x * 4 + (threadIdx.x >> 6);
    if (row >= rows) return;
    const int M = (K + 63) / 64;
    T* xrow = X + row * K;
    T* grow = G + row * K;
    bool viol = false;
    for (int s = 0; s < nsweeps; ++s) {
        const bool check = check_first && (s == 0);
        for (int m = 0; m < M; ++m) {
            const int c0 = lane + 64 * m;
            const bool ok = c0 < K;
            const int cc = ok ? c0 : 0;
            const T xv = xrow[cc], gv = grow[cc], av = AAt[(long)cc * K + cc];
            const R alv = alphak[cc], tlv = tolk[cc];
            T x = ok ? xv : zero_of<T>();
            T g = ok ? gv : zero_of<T>();
            const T akk = ok ? av : zero_of<T>();
            const R al = ok ? alv : R(0);
            const R tl = ok ? tlv : R(1);
            const int kend = min(64, K - 64 * m);
            int cursor = 0;
            while (true) {
                const T z = fmadd(g, x, akk);
                const T xn = prox_apply<PROX>(z, al);
                const T d = sub(xn, x);
                const bool moves = (lane >= cursor) && (lane < kend) && (abs2(d) != R(0));
                const unsigned long long mask = __ballot(moves);
                if (mask == 0ull) {
                    if (check && lane >= cursor && lane < kend && !((R(0) - tl) < R(0))) viol = true;
                    break;
                }
                const int kk = __ffsll((long long)mask) - 1;
                if (check && lane >= cursor && lane < kk && !((R(0) - tl) < R(0))) viol = true;
                const T dk = lane_get(d, kk);
                if (lane == kk) {
                    x = xn;
                    if (check && !((absval(d) - tl) < R(0))) viol = true;
                }
                const T* arow = AAt + (long)(64 * m + kk) * K;
                g = ok ? fmsub(g, dk, arow[cc]) : g;          // this slot: the register copy
                for (int m0 = 0; m0 < M; m0 += 8) {               // the other slots: in memory
                    T ar[8], gg[8];
#pragma unroll
                    for (int u = 0; u < 8; ++u) {
                        const int c = lane + 64 * (m0 + u);
                        const int ci = (m0 + u < M && c < K) ? c : 0;
                        ar[u] = arow[ci];
                        gg[u] = grow[ci];
                    }
#pragma unroll
                    for (int u = 0; u < 8; ++u) {
                        const int c = lane + 64 * (m0 + u);
                        if (m0 + u < M && m0 + u != m && c < K) grow[c] = fmsub(gg[u], dk, ar[u]);
                    }
                }
                cursor = kk + 1;
            }
            if (ok) {
                xrow[c0] = x;
                grow[c0] = g;
            }
        }
    }
    if (__ballot(viol) != 0ull && lane == 0) *flag = 1;
}

// Masked coordinate descent, as written in lasso.py:555-583: with r = (y - x.A) o M kept in
// memory,  x_k <- S(r . conj(A_k) + x_k (A_k . conj(A_k)), alpha_nk);  r -= dx (A_k o M).
// One workgroup per row; F-length dot products by block reduction.  (Parity path for
// lasso.solve(mask=...); not on a BASELINE config.)
template <class T, int PROX>
__global__ void __launch_bounds__(256) cd_mask_kernel(T* __restrict__ X, T* __restrict__ Rres,
                                                      const T* __restrict__ A,
                                                      const real_t<T>* __restrict__ mask,
                                                      const real_t<T>* __restrict__ akk,
                                                      const real_t<T>* __restrict__ alphak,
                                                      const real_t<T>* __restrict__ rowscale,
                                                      const real_t<T>* __restrict__ tolk, int K, long F,
                                                      int nsweeps, int check_last,
                                                      int* __restrict__ flag) {
    typedef real_t<T> R;
    __shared__ R sh[4];
    __shared__ T s_d;
    const long row = blockIdx.x;
    T* r = Rres + row * F;
    const R* mrow = mask + row * F;
    bool viol = false;
    for (int s = 0; s < nsweeps; ++s) {
        const bool check = check_last && (s == nsweeps - 1);
        for (int k = 0; k < K; ++k) {
            const T* ak = A + (long)k * F;
            R pre = 0, pim = 0;
            for (long f = threadIdx.x; f < F; f += 256) {
                const T t = mul(r[f], conj_of(ak[f]));
                pre += real_part(t);
                pim += imag_part(t);
            }
            const T dot = block_sum_256_parts<T>(pre, pim, sh);
            if (threadIdx.x == 0) {
                const T xk = X[row * K + k];
                const T z = add(dot, scale(xk, akk[k]));
                const T xn = prox_apply<PROX>(z, alphak[k] * rowscale[row]);
                const T d = sub(xn, xk);
                if (check && !((absval(d) - tolk[k]) < R(0))) *flag = 1;
                X[row * K + k] = xn;
                s_d = d;
            }
            __syncthreads();
            const T d = s_d;
            if (abs2(d) != R(0))
                for (long f = threadIdx.x; f < F; f += 256)
                    r[f] = sub(r[f], mul(d, scale(ak[f], mrow[f])));
            __syncthreads();
        }
    }
    (void)viol;
}

// akk[k] = sum_f |A[k, f]|^2  is what A_k . conj(A_k) evaluates to; computed by the row-norm
// kernel as s^2.  This helper squares a vector.
template <class R>
__global__ void __launch_bounds__(256) square_vec_kernel(const R* __restrict__ v, long n, R* __restrict__ out) {
    for (long i = blockIdx.x * 256L + threadIdx.x; i < n; i += (long)gridDim.x * 256L)
        out[i] = v[i] * v[i];
}

// Widest dictionary the register form of the coordinate descent takes (64 lanes x 32 slots).  The
// environment variable DCP_CD_REGISTER_LIMIT (tests only) lowers it, so that the memory-resident form
// can be checked bit for bit against the register form on the same problem.
inline int cd_register_limit() {
    const char* e = getenv("DCP_CD_REGISTER_LIMIT");
    int v = e ? atoi(e) : 2048;
    if (v < 1024) v = 1024;     // the launch ladder above 1024 is the only place it is consulted
    if (v > 2048) v = 2048;
    return v;
}

// ---- the solver ----------------------------------------------------------------------------------
template <class T>
struct LassoWs {
    typedef real_t<T> R;
    T* An = nullptr;     // [K,F] row-normalised (and 1-D-masked) design matrix
    T* Ym = nullptr;     // [N,F] y o mask (any mask)
    T* yAt = nullptr;    // [N,K]
    T* AAt = nullptr;    // [K,K]
    T* Am = nullptr;     // [K,F] A o mean(mask)  (2-D mask: Lipschitz bound only)
    T* slabs = nullptr;  // split-K partials of AAt
    T* xb[4] = {nullptr, nullptr, nullptr, nullptr};  // iterates [N,K]
    T* G = nullptr;      // [N,K] CD gradient
    T* T1 = nullptr;     // [N,F] (v A) o M
    R* s = nullptr;      // [K] row norms of A
    R* alphak = nullptr; // [K]
    R* tolk = nullptr;   // [K]
    R* akk = nullptr;    // [K]
    R* rowscale = nullptr;  // [N]
    R* mbar = nullptr;   // [F]
    R* part = nullptr;   // column-sum partials [64, F]
    R* scal = nullptr;   // [4]: Linv, nvalid, L
    work_t<T>* inv_a = nullptr;  // admm: K x K work matrices (ping-pong) or the [N,K,K] per-row systems
    work_t<T>* inv_b = nullptr;
    R* gpart = nullptr;  // [64, K] Gershgorin column-sum stripes
    R* ext1 = nullptr;   // complex: real extended image of a [K,F] operand (4KF reals)
    R* ext2 = nullptr;   // complex: real extended image of AAt (4K^2 reals)
    int* flag = nullptr;
    size_t slab_count = 0;
};

template <class T>
inline void lasso_layout(WsLayout& a, LassoWs<T>& w, int64_t N, int64_t F, int64_t K, int mask_ndim, int method) {
    a.take(w.An, (size_t)K * F);
    if (mask_ndim != 0) a.take(w.Ym, (size_t)N * F);
    a.take(w.yAt, (size_t)N * K);
    a.take(w.AAt, (size_t)K * K);
    if (mask_ndim == 2) a.take(w.Am, (size_t)K * F);
    w.slab_count = (size_t)kMaxSplits * K * K;
    a.take(w.slabs, w.slab_count);
    for (int i = 0; i < 4; ++i) a.take(w.xb[i], (size_t)N * K);
    if ((method == DCP_LASSO_CD || method == DCP_LASSO_PARALLEL_CD) && mask_ndim != 2)
        a.take(w.G, (size_t)N * K);
    if (mask_ndim == 2) a.take(w.T1, (size_t)N * F);
    if (method == DCP_LASSO_ADMM) {
        if (mask_ndim == 2) {
            a.take(w.inv_a, (size_t)N * K * K);
        } else {
            a.take(w.inv_a, (size_t)K * K);
            a.take(w.inv_b, (size_t)K * K);
        }
    }
    a.take(w.s, (size_t)K);
    a.take(w.alphak, (size_t)K);
    a.take(w.tolk, (size_t)K);
    a.take(w.akk, (size_t)K);
    a.take(w.rowscale, (size_t)N);
    a.take(w.mbar, (size_t)F);
    a.take(w.part, (size_t)64 * F);
    a.take(w.scal, 4);
    a.take(w.gpart, (size_t)64 * K);
    a.take(w.flag, 4);
    if (scalar_traits<T>::is_complex) {
        a.take(w.ext1, (size_t)4 * K * F);
        a.take(w.ext2, (size_t)4 * K * K);
    }
}

// C[K,K] = P . Q^H for [K,F] operands, reduction over F split into ordered slabs.
template <class T>
inline int gram_kk(dcp_handle* h, const T* P, const T* Q, int K, int F, LassoWs<T>& w, T* out) {
    GemmArgs<T> g;
    g.A = P; g.lda = F; g.B = Q; g.ldb = F; g.M = K; g.N = K; g.K = F;
    g.conjB = true;
    g.ext_ws = w.ext1;
    // float32, >= 256 atoms: 64 x 64 tiles x 8 splits (tools/gemm_hook_sweep.py 0 512 512 4096: 31 us with the
    // slab sum against 45 us for the 128 x 128 x 64 tile x 32 splits the automatic plan takes)
    if (std::is_same<T, float>::value && K >= 256 && K <= 1024) g.tile = TILE_SMALL;
    plan_splits<FORM_NT>(g, 512, kMaxSplits);
    if ((size_t)g.ksplits * K * K > w.slab_count) return fail(h, DCP_ERR_INTERNAL, "lasso slab plan");
    DCP_LAUNCH_OK(h, (gemm<FORM_NT>(h->stream, g, EpiSlab<T>{w.slabs, K, (long)K * K})));
    launch_reduce_slabs_scalar<T>(h->stream, w.slabs, (long)K * K, g.ksplits, (long)K * K, out);
    DCP_LAUNCH_OK(h, hipGetLastError());
    return DCP_OK;
}

// The dictionary step's deferred *it_out of a coordinate-descent solve (see lasso_cd_gram): called
// once the rest of the step has been enqueued, when the flag has long landed.
inline int lasso_settle_deferred(dcp_handle* h) {
    if (h->lasso_deferred_flag == nullptr) return DCP_OK;
    int* f = h->lasso_deferred_flag;
    h->lasso_deferred_flag = nullptr;
    const bool copy = h->lasso_deferred_copy;   // DCP_LASSO_OMP: the word IS the count (dict_lasso)
    h->lasso_deferred_copy = false;
    DCP_TRY(poll_host_flag(h, f));
    if (copy) {
        if (h->lasso_deferred_it != nullptr) *h->lasso_deferred_it = *f;
    } else if (*f == 0 && h->lasso_deferred_it != nullptr) {
        *h->lasso_deferred_it = h->lasso_deferred_it_met;
    }
    h->lasso_deferred_it = nullptr;
    return DCP_OK;
}

// scal[0] = 1 / L, scal[2] = L for L = max_j sum_i |M[i, j]|  (eigen.py:20)
template <class T>
inline int gershgorin_bound(dcp_handle* h, const T* M, int K, LassoWs<T>& w) {
    typedef real_t<T> R;
    const int stripes = K >= 64 ? 64 : K;
    const long rows_per = (K + stripes - 1) / stripes;
    hipLaunchKernelGGL((colabs_partial_kernel<T>), dim3(grid_for(K, 64), stripes), dim3(256), 0,
                       h->stream, M, (long)K, rows_per, w.gpart);
    DCP_LAUNCH_OK(h, hipGetLastError());
    hipLaunchKernelGGL((gershgorin_finish_kernel<R>), dim3(1), dim3(256), 0, h->stream,
                       (const R*)w.gpart, (long)K, stripes, w.scal);
    DCP_LAUNCH_OK(h, hipGetLastError());
    return DCP_OK;
}

// Inputs of the two solvers that need more than (alpha, tol, maxiter).
struct LassoExtra {
    const int* order = nullptr;   // parallel_cd: device int32 [order_rows, K] shuffle table
    int64_t order_rows = 0;
    double rho = 1.0;             // admm
    // the caller enqueues more work on the same stream right behind the solve (the dictionary step's x^H [y | x]
    // product): skip the stream synchronisation at the end -- *it_out is known on the host without it
    bool no_final_sync = false;
    // start the dictionary step's registered row prefetch (dcp_dict_prefetch_rows_bytes) right behind the y.A^H
    // product, beside the solver's iterations.  Measured (round 4, configs[2] end to end): 1.720 ms / step against
    // 1.699 when it runs beside the atom sweep instead -- the dictionary step leaves it off.
    bool start_prefetch = false;
};

// One prepared solve, as the solvers below read it.
template <class T>
struct LassoProblem {
    typedef real_t<T> R;
    dcp_handle* h;
    hipStream_t st;
    int N, F, K;
    const R* mask;       // null, [F] (mask_ndim 1: folded into An and Ym by lasso_prepare) or [N,F] (mask_ndim 2)
    int mask_ndim;
    const R* rowscale;   // 2-D mask: its row sums [N]; null otherwise
    T* X;                // [N,K] in: initial estimate, out: solution
    LassoWs<T>& w;       // after lasso_prepare: An, s, alphak, tolk, yAt, flag = 0, and (see there) xb[0] = x * s
    int* host_flag;      // 64 bytes of pinned host memory
    int maxiter;
    const LassoExtra& extra;
};

// What a solver leaves: the reference's iteration count and the buffer that holds x * s.
template <class T>
struct LassoOutcome {
    int it;
    T* result;
    bool final_in_place;   // the last iteration's epilogue has already written x = result / s into X
};

// v [N,K] times a K x K matrix (A A^H, or what a solver made of it); complex: its real extended image goes to ext2
template <class T>
inline GemmArgs<T> codes_kk_product(const LassoProblem<T>& p, const T* v, const T* M) {
    GemmArgs<T> a;
    a.A = v; a.lda = p.K; a.B = M; a.ldb = p.K; a.M = p.N; a.N = p.K; a.K = p.K;
    a.ext_ws = p.w.ext2;
    return a;
}

// 2-D mask: T1 = (v An) o M, then T1 An^H with the solver's step in the epilogue
template <class T, class Epi>
inline int masked_back_projection(const LassoProblem<T>& p, const T* v, const Epi& epi) {
    const LassoWs<T>& w = p.w;
    GemmArgs<T> a1;
    a1.A = v; a1.lda = p.K; a1.B = w.An; a1.ldb = p.F; a1.M = p.N; a1.N = p.F; a1.K = p.K;
    a1.ext_ws = w.ext1;
    DCP_LAUNCH_OK(p.h, (gemm<FORM_NN>(p.st, a1, EpiMulMask<T>{p.mask, p.F, w.T1, p.F})));
    GemmArgs<T> a2;
    a2.A = w.T1; a2.lda = p.F; a2.B = w.An; a2.ldb = p.F; a2.M = p.N; a2.N = p.K; a2.K = p.F;
    a2.conjB = true;
    a2.ext_ws = w.ext1;
    DCP_LAUNCH_OK(p.h, (gemm<FORM_NT>(p.st, a2, epi)));
    return DCP_OK;
}

// parallel_cd and admm: step(i, check) enqueues iteration i; the stop test of every tenth one (lasso.py:479, :612) is
// read synchronously right behind it.  *met_at = the iteration whose test was met; untouched when maxiter ran out.
template <class T, class Step>
inline int sync_checked_loop(const LassoProblem<T>& p, Step&& step, int* met_at) {
    for (int i = 0; i < p.maxiter; ++i) {
        const int check = (i % 10 == 0) ? 1 : 0;
        if (check) DCP_HIP_OK(p.h, hipMemsetAsync(p.w.flag, 0, sizeof(int), p.st));
        DCP_TRY(step(i, check));
        if (check) {
            bool viol = true;
            DCP_TRY(read_scalar(p.h, (const int*)p.w.flag, &viol, p.host_flag));
            if (!viol) { *met_at = i; break; }
        }
    }
    return DCP_OK;
}

// Mask folding, row normalisation, the scaled alpha / tol, x * s and y A^H (lasso.py:120-131).  scale_x = false
// leaves xb[0] to the solver (lasso_prox forms x * s in a pass it makes anyway).
template <class T>
inline int lasso_prepare(const LassoProblem<T>& p, const T* Y, const T* A, real_t<T> alpha, real_t<T> tol,
                         bool scale_x) {
    typedef real_t<T> R;
    LassoWs<T>& w = p.w;
    const int N = p.N, F = p.F, K = p.K;
    // ---- 1-D mask folds into y and A (lasso.py:120-122); any mask: Ym = y o M ----
    const T* Ause = A;
    const T* Yuse = p.mask_ndim != 0 ? w.Ym : Y;
    if (p.mask_ndim == 1) {
        hipLaunchKernelGGL((mul_mask_kernel<T>), dim3(grid_for((long)K * F)), dim3(256), 0, p.st, A, p.mask,
                           (long)K, (long)F, 0L, w.An);
        DCP_LAUNCH_OK(p.h, hipGetLastError());
        Ause = w.An;
    }
    if (p.mask_ndim != 0) {   // (mask row stride 0: the same [F] mask for every sample)
        hipLaunchKernelGGL((mul_mask_kernel<T>), dim3(grid_for((long)N * F)), dim3(256), 0, p.st, Y, p.mask,
                           (long)N, (long)F, p.mask_ndim == 2 ? (long)F : 0L, w.Ym);
        DCP_LAUNCH_OK(p.h, hipGetLastError());
        if (p.mask_ndim == 1)
            hipLaunchKernelGGL((reduce_vector_kernel<SumOp, R, FinStore<R>>), dim3(1), dim3(256), 0, p.st, p.mask,
                               (long)F, FinStore<R>{w.scal + 1});   // sum(mask)
        else
            hipLaunchKernelGGL((rowsum_kernel<R>), dim3(N), dim3(256), 0, p.st, p.mask, (long)F, (long)F, w.rowscale);
        DCP_LAUNCH_OK(p.h, hipGetLastError());
    }
    // ---- A scaling (lasso.py:124-131): s = |A_k|, An = A / s, alpha/s, tol*s, x*s ----
    hipLaunchKernelGGL((row_normalize_kernel<T>), dim3(K), dim3(256), 0, p.st, Ause, (long)F, (long)F, 1,
                       (const T*)nullptr, 0L, w.An, (long)F, (R*)nullptr, w.s);
    DCP_LAUNCH_OK(p.h, hipGetLastError());
    hipLaunchKernelGGL((lasso_scalars_kernel<R>), dim3(grid_for(K, 64)), dim3(256), 0, p.st, w.s, (long)K,
                       alpha, tol, p.mask_ndim == 1 ? w.scal + 1 : (const R*)nullptr,
                       p.mask_ndim == 2 ? R(1) : R(F), w.alphak, w.tolk, w.flag);
    DCP_LAUNCH_OK(p.h, hipGetLastError());
    if (scale_x) {
        hipLaunchKernelGGL((col_scale_kernel<T>), dim3(grid_for((long)N * K)), dim3(256), 0, p.st, (const T*)p.X,
                           (const R*)w.s, (long)N, (long)K, 1, w.xb[0]);
        DCP_LAUNCH_OK(p.h, hipGetLastError());
    }
    // ---- yAt = (y o M) An^H ----
    GemmArgs<T> a;
    a.A = Yuse; a.lda = F; a.B = w.An; a.ldb = F; a.M = N; a.N = K; a.K = F; a.conjB = true;
    a.ext_ws = w.ext1;
    // deep reduction, few big tiles: ordered split-K partials in the (still unused) iterate buffers
    const long stride = (long)(w.xb[2] - w.xb[1]);
    const int ys = (stride >= (long)N * K && w.xb[3] - w.xb[2] == stride) ? plan_deep_nt(a, 3) : 1;
    if (ys > 1) {
        DCP_LAUNCH_OK(p.h, (gemm<FORM_NT>(p.st, a, EpiSlab<T>{w.xb[1], K, stride})));
        launch_reduce_slabs<T>(p.st, (const T*)w.xb[1], stride, ys, (long)N * K, w.yAt);
        DCP_LAUNCH_OK(p.h, hipGetLastError());
    } else {
        DCP_LAUNCH_OK(p.h, (gemm<FORM_NT>(p.st, a, EpiStore<T>{w.yAt, K})));
    }
    if (p.extra.start_prefetch) DCP_TRY(start_registered_prefetch(p.h));
    return DCP_OK;
}

// ns sweeps of the Gram-form coordinate descent over xb[0] and G; check_first: the first one raises *flag when its
// stop test is violated; cond != null: the device skips the launch when *cond is zero.
// (the register form holds a row's K coefficients in one wave: 64 lanes x up to 32 slots;
//  wider dictionaries take the memory-resident form -- the reference has no limit, lasso.py:526-552)
template <class T, int PROX>
inline int launch_cd_gram(const LassoProblem<T>& p, int ns, int check_first, const int* cond) {
    typedef real_t<T> R;
    const LassoWs<T>& w = p.w;
    const int K = p.K;
    auto launch = [&](auto kernel) {
        hipLaunchKernelGGL(kernel, dim3((p.N + 3) / 4), dim3(256), 0, p.st, w.xb[0], w.G, (const T*)w.AAt,
                           (const R*)w.alphak, (const R*)w.tolk, (long)p.N, K, ns, check_first, w.flag, cond);
    };
    if (K <= 64) launch(cd_gram_kernel<T, PROX, 1>);
    else if (K <= 128) launch(cd_gram_kernel<T, PROX, 2>);
    else if (K <= 256) launch(cd_gram_kernel<T, PROX, 4>);
    else if (K <= 512) launch(cd_gram_kernel<T, PROX, 8>);
    else if (K <= 1024) launch(cd_gram_kernel<T, PROX, 16>);
    else if (K <= cd_register_limit()) launch(cd_gram_kernel<T, PROX, 32>);
    else launch(cd_gram_wide_kernel<T, PROX>);
    DCP_LAUNCH_OK(p.h, hipGetLastError());
    return DCP_OK;
}

// ---------------- coordinate descent, Gram form (mask none or 1-D) ----------------
// gram_ready: AAt already holds An An^H (parallel_cd's fallback).  it_out: where a deferred count goes.
template <class T, int PROX>
inline int lasso_cd_gram(const LassoProblem<T>& p, bool gram_ready, int* it_out, LassoOutcome<T>* out) {
    LassoWs<T>& w = p.w;
    const int maxiter = p.maxiter;
    if (!gram_ready) DCP_TRY(gram_kk<T>(p.h, w.An, w.An, p.K, p.F, w, w.AAt));
    const GemmArgs<T> g = codes_kk_product<T>(p, w.xb[0], w.AAt);   // G = yAt - x AAt
    DCP_LAUNCH_OK(p.h, (gemm<FORM_NN>(p.st, g, EpiSubFrom<T>{w.yAt, p.K, w.G, p.K})));
    // Ten sweeps = a check sweep (0, 10, 20, ...: lasso.py:546-551) launched on its own and the up to nine sweeps
    // behind it in a second launch that the DEVICE skips when the check sweep met the test (its flag is still
    // zero): the codes are then exactly those the reference returns, and nothing on the host has to read the flag
    // between the two launches.  The flag travels to pinned host memory behind them (flag_publish_kernel) and is
    // polled only where the host needs it: to decide on ANOTHER ten sweeps, or for *it_out -- which the
    // dictionary step defers to the end of the step (LassoExtra::no_final_sync), so that its default solve
    // (cd x 10) puts no host round trip into the middle of the step.
    // (Rounds 3-4 ran one launch per ten sweeps with the post-check codes parked in a snapshot and read the flag
    // synchronously: ~37 us of idle GPU per solve in the kernel trace, plus a fill and a copy kernel.)
    int sweep = 0;
    while (sweep < maxiter) {
        int last = sweep + 9;
        if (last > maxiter - 1) last = maxiter - 1;
        // (w.flag is zero here: lasso_scalars_kernel at the start of the solve, flag_publish_kernel afterwards)
        DCP_TRY((launch_cd_gram<T, PROX>(p, 1, 1, nullptr)));                              // the check sweep
        if (last > sweep) DCP_TRY((launch_cd_gram<T, PROX>(p, last - sweep, 0, w.flag)));  // the rest, unless met
        *reinterpret_cast<volatile int*>(p.host_flag) = -1;                 // sentinel: nothing has landed yet
        hipLaunchKernelGGL(flag_publish_kernel<void>, dim3(1), dim3(64), 0, p.st, w.flag, p.host_flag);
        DCP_LAUNCH_OK(p.h, hipGetLastError());
        if (last == maxiter - 1 && p.extra.no_final_sync) {
            // the last ten sweeps of a solve inside the dictionary step: *it_out is settled by
            // lasso_settle_deferred() once the rest of the step has been enqueued
            p.h->lasso_deferred_flag = p.host_flag;
            p.h->lasso_deferred_it = it_out;
            p.h->lasso_deferred_it_met = sweep;
            break;
        }
        DCP_TRY(poll_host_flag(p.h, p.host_flag));
        if (*p.host_flag == 0) {
            out->it = sweep;
            break;
        }
        sweep = last + 1;
    }
    return DCP_OK;
}

// ---------------- coordinate descent with a 2-D mask (as written) ----------------
template <class T, int PROX>
inline int lasso_cd_rows(const LassoProblem<T>& p, LassoOutcome<T>* out) {
    typedef real_t<T> R;
    LassoWs<T>& w = p.w;
    const int N = p.N, F = p.F, K = p.K, maxiter = p.maxiter;
    T* xcur = w.xb[0];
    GemmArgs<T> a;   // r = y o M - (x An) o M
    a.A = xcur; a.lda = K; a.B = w.An; a.ldb = F; a.M = N; a.N = F; a.K = K;
    a.ext_ws = w.ext1;
    DCP_LAUNCH_OK(p.h, (gemm<FORM_NN>(p.st, a, EpiMaskedResidual<T>{w.Ym, p.mask, w.T1, (long)F})));
    // A_k . conj(A_k) of the normalised rows, as the reference evaluates it (== 1 up to rounding)
    hipLaunchKernelGGL((row_normalize_kernel<T>), dim3(K), dim3(256), 0, p.st, (const T*)w.An, (long)F,
                       (long)F, 1, (const T*)nullptr, 0L, w.Am, (long)F, (R*)nullptr, w.akk);
    DCP_LAUNCH_OK(p.h, hipGetLastError());
    hipLaunchKernelGGL((square_vec_kernel<R>), dim3(grid_for(K, 64)), dim3(256), 0, p.st,
                       (const R*)w.akk, (long)K, w.akk);
    DCP_LAUNCH_OK(p.h, hipGetLastError());
    int sweep = 0;
    while (sweep < maxiter) {
        int last = (sweep % 10 == 0) ? sweep : (sweep / 10 + 1) * 10;
        int check_last = 1;
        if (last > maxiter - 1) { last = maxiter - 1; check_last = (last % 10 == 0); }
        const int ns = last - sweep + 1;
        DCP_HIP_OK(p.h, hipMemsetAsync(w.flag, 0, sizeof(int), p.st));
        hipLaunchKernelGGL((cd_mask_kernel<T, PROX>), dim3(N), dim3(256), 0, p.st, xcur, w.T1,
                           (const T*)w.An, p.mask, (const R*)w.akk, (const R*)w.alphak,
                           (const R*)w.rowscale, (const R*)w.tolk, K, (long)F, ns, check_last,
                           w.flag);
        DCP_LAUNCH_OK(p.h, hipGetLastError());
        sweep = last + 1;
        if (check_last) {
            bool viol = true;
            DCP_TRY(read_scalar(p.h, (const int*)w.flag, &viol, p.host_flag));
            if (!viol) { out->it = last; break; }
        }
    }
    return DCP_OK;
}

// ---------------- parallel coordinate descent (lasso.py:476-484, 515-523) ----------------
// p = int(K / Gershgorin(A A^H)) coordinates per row and iteration, unmasked Gram matrix in every variant
// (lasso.py:464-470, 503-509); p <= 1 falls back to plain coordinate descent.
template <class T, int PROX>
inline int lasso_pcd(const LassoProblem<T>& p, int* it_out, LassoOutcome<T>* out) {
    typedef real_t<T> R;
    LassoWs<T>& w = p.w;
    const int K = p.K;
    DCP_TRY(gram_kk<T>(p.h, w.An, w.An, K, p.F, w, w.AAt));
    DCP_TRY(gershgorin_bound<T>(p.h, w.AAt, K, w));
    R bound = 0;
    DCP_TRY(read_scalar(p.h, (const R*)(w.scal + 2), &bound,
                        reinterpret_cast<R*>(reinterpret_cast<char*>(p.host_flag) + 16)));
    const R ratio = (R)K / bound;
    const int pcd_p = (ratio == ratio && ratio < R(2147483647)) ? (int)ratio : 0;
    if (pcd_p <= 1) {
        if (p.mask_ndim == 2)
            return fail(p.h, DCP_ERR_REF_TYPEERROR,
                        "parallel_cd with a full mask and p <= 1: the reference's fallback call "
                        "raises TypeError (lasso.py:509)");
        return lasso_cd_gram<T, PROX>(p, true, it_out, out);
    }
    if (p.extra.order == nullptr || p.extra.order_rows < (int64_t)p.maxiter)
        return fail(p.h, DCP_ERR_INVALID, "parallel_cd needs a shuffle table of >= maxiter rows");
    // iteration i reads x0 from xb[i & 1], leaves x0 + dx * select in the other and its full update in xb[2]
    T* Xnew = w.xb[2];
    int met_at = -1;
    DCP_TRY(sync_checked_loop(p, [&](int i, int check) -> int {
        T* X0 = w.xb[i & 1];
        EpiPcdStep<T, PROX> epi{w.yAt, X0, Xnew, w.xb[(i & 1) ^ 1], (long)K, w.alphak, w.tolk, p.rowscale,
                                p.extra.order + (long)i * K, pcd_p, check, w.flag};
        if (p.mask_ndim == 2) return masked_back_projection(p, X0, epi);
        DCP_LAUNCH_OK(p.h, (gemm<FORM_NN>(p.st, codes_kk_product<T>(p, X0, w.AAt), epi)));   // back = x0 AAt
        return DCP_OK;
    }, &met_at));
    if (met_at >= 0) out->it = met_at;
    out->result = met_at >= 0 ? Xnew : w.xb[p.maxiter & 1];   // met: the full update (lasso.py:479-480)
    return DCP_OK;
}

// ---------------- ADMM (lasso.py:586-618) ----------------
template <class T, int PROX>
inline int lasso_admm(const LassoProblem<T>& p, LassoOutcome<T>* out) {
    typedef real_t<T> R;
    typedef work_t<T> TW;
    LassoWs<T>& w = p.w;
    const int N = p.N, K = p.K;
    const R rho = (R)p.extra.rho;
    T* xcur = w.xb[0];
    DCP_TRY(gram_kk<T>(p.h, w.An, w.An, K, p.F, w, w.AAt));
    hipLaunchKernelGGL((inv_load_kernel<T>), dim3(grid_for((long)K * K)), dim3(256), 0, p.st,
                       (const T*)w.AAt, K, p.extra.rho, w.inv_a);
    DCP_LAUNCH_OK(p.h, hipGetLastError());
    TW* src = w.inv_a;
    TW* dst = w.inv_b;
    for (int k = 0; k < K; ++k) {
        hipLaunchKernelGGL((gj_step_kernel<TW>), dim3(grid_for((long)K * K)), dim3(256), 0, p.st,
                           (const TW*)src, dst, K, k);
        TW* t = src; src = dst; dst = t;
    }
    DCP_LAUNCH_OK(p.h, hipGetLastError());
    T* Minv = w.AAt;     // (AAt + rho I)^-1 replaces AAt
    hipLaunchKernelGGL((inv_store_kernel<T>), dim3(grid_for((long)K * K)), dim3(256), 0, p.st,
                       (const TW*)src, (long)K * K, Minv);
    DCP_LAUNCH_OK(p.h, hipGetLastError());
    T* U = w.xb[1];
    hipLaunchKernelGGL((admm_init_kernel<T>), dim3(grid_for((long)N * K)), dim3(256), 0, p.st,
                       (const T*)w.yAt, (const T*)xcur, (long)N * K, rho, U, w.xb[2]);
    DCP_LAUNCH_OK(p.h, hipGetLastError());
    DCP_TRY(sync_checked_loop(p, [&](int i, int check) -> int {
        T* V = w.xb[2 + (i & 1)];    // v ping-pongs between xb[2] and xb[3]
        T* Vn = w.xb[3 - (i & 1)];
        EpiAdmmStep<T, PROX> epi{w.yAt, xcur, U, Vn, (long)K, w.alphak, w.tolk, rho, check, w.flag};
        DCP_LAUNCH_OK(p.h, (gemm<FORM_NN>(p.st, codes_kk_product<T>(p, V, Minv), epi)));   // x_new = V Minv
        return DCP_OK;
    }, &out->it));   // lasso.py:612-614
    return DCP_OK;
}

// ---------------- ADMM with a 2-D mask: one K x K system per row (lasso.py:621-657) ----------------
template <class T, int PROX>
inline int lasso_admm_rows(const LassoProblem<T>& p, LassoOutcome<T>* out) {
    typedef real_t<T> R;
    typedef work_t<T> TW;
    LassoWs<T>& w = p.w;
    const int N = p.N, K = p.K;
    const R rho = (R)p.extra.rho;
    T* xcur = w.xb[0];
    // dynamic LDS of the two per-row kernels: pivot row + column (2 K work elements) and V (K elements);
    // beyond the default 64 KiB the per-function cap is raised, up to the CU's 160 KiB (K <= 10240 real,
    // 5120 complex -- where ONE row's K x K system is already 0.8 GB; the reference, lasso.py:620-657,
    // holds the same N K^2 array)
    const size_t gj_lds = (size_t)2 * K * sizeof(TW), step_lds = (size_t)K * sizeof(T);
    if (gj_lds > 160 * 1024)
        return fail(p.h, DCP_ERR_UNSUPPORTED, "masked admm: n_features too large for the per-row inverse");
    if (gj_lds > 65536)
        DCP_HIP_OK(p.h, hipFuncSetAttribute(reinterpret_cast<const void*>(&gj_batched_kernel<TW>),
                                            hipFuncAttributeMaxDynamicSharedMemorySize, (int)gj_lds));
    if (step_lds > 65536)
        DCP_HIP_OK(p.h, hipFuncSetAttribute(reinterpret_cast<const void*>(&admm_mask_step_kernel<T, PROX>),
                                            hipFuncAttributeMaxDynamicSharedMemorySize, (int)step_lds));
    hipLaunchKernelGGL((admm_mask_system_kernel<T>), dim3(N), dim3(256), 0, p.st, (const T*)w.An, p.mask,
                       K, (long)p.F, p.extra.rho, w.inv_a);
    DCP_LAUNCH_OK(p.h, hipGetLastError());
    hipLaunchKernelGGL((gj_batched_kernel<TW>), dim3(N), dim3(256), (size_t)2 * K * sizeof(TW), p.st,
                       w.inv_a, K);
    DCP_LAUNCH_OK(p.h, hipGetLastError());
    T* U = w.xb[1];
    T* V = w.xb[2];
    hipLaunchKernelGGL((admm_init_kernel<T>), dim3(grid_for((long)N * K)), dim3(256), 0, p.st,
                       (const T*)w.yAt, (const T*)xcur, (long)N * K, rho, U, V);
    DCP_LAUNCH_OK(p.h, hipGetLastError());
    DCP_TRY(sync_checked_loop(p, [&](int, int check) -> int {
        hipLaunchKernelGGL((admm_mask_step_kernel<T, PROX>), dim3(N), dim3(256),
                           (size_t)K * sizeof(T), p.st, (const T*)w.yAt, (const TW*)w.inv_a, xcur, U, V,
                           K, (const R*)w.alphak, (const R*)w.rowscale, (const R*)w.tolk, rho, check,
                           w.flag);
        DCP_LAUNCH_OK(p.h, hipGetLastError());
        return DCP_OK;
    }, &out->it));
    return DCP_OK;
}

// ---------------- ista / acc_ista / fista ----------------
template <class T, int PROX>
inline int lasso_prox(const LassoProblem<T>& p, int method, LassoOutcome<T>* out) {
    typedef real_t<T> R;
    LassoWs<T>& w = p.w;
    const int N = p.N, F = p.F, K = p.K;
    const T* Abar = w.An;
    if (p.mask_ndim == 2) {   // Lipschitz bound from (A o mean_batch(M)) A^H   (lasso.py:317)
        DCP_TRY(column_sums<R>(p.h, p.mask, F, N, F, w.part, w.mbar));
        hipLaunchKernelGGL((scale_vec_kernel<R>), dim3(grid_for(F, 64)), dim3(256), 0, p.st,
                           (const R*)w.mbar, (long)F, R(N), w.mbar);
        DCP_LAUNCH_OK(p.h, hipGetLastError());
        hipLaunchKernelGGL((mul_mask_kernel<T>), dim3(grid_for((long)K * F)), dim3(256), 0, p.st,
                           (const T*)w.An, (const R*)w.mbar, (long)K, (long)F, 0L, w.Am);
        DCP_LAUNCH_OK(p.h, hipGetLastError());
        Abar = w.Am;
    }
    DCP_TRY(gram_kk<T>(p.h, Abar, w.An, K, F, w, w.AAt));
    DCP_TRY(gershgorin_bound<T>(p.h, w.AAt, K, w));
    if (p.mask_ndim != 2) {   // AAt becomes H = I - Linv A A^H (see EpiProxStepH); xb[0] = x * s in the same pass
        hipLaunchKernelGGL((hform_prepare_kernel<T>), dim3(grid_for((long)K * K + (long)N * K)), dim3(256), 0, p.st,
                           w.AAt, (long)K, w.yAt, (long)N * K, (const R*)w.scal, (const T*)p.X, (const R*)w.s, w.xb[0]);
        DCP_LAUNCH_OK(p.h, hipGetLastError());
    }
    const bool mom = (method != DCP_LASSO_ISTA);
    bool wrote_final = false;
    auto step = [&](int i, T* V, T* P, T* Nw, T* Vn, R coef, int check, bool is_last) -> int {
        if (p.mask_ndim == 2) {   // back = ((V An) o M) An^H, prox step in the epilogue
            EpiProxStep<T, PROX> epi{w.yAt, V, P, Nw, Vn, (long)K, w.scal, w.alphak, w.tolk, p.rowscale, coef, check,
                                     w.flag};
            return masked_back_projection(p, V, epi);
        }
        GemmArgs<T> a = codes_kk_product<T>(p, V, w.AAt);   // back = V H, prox step in the epilogue
        // complex: the extended image of A A^H (ext2 holds nothing else during the loop) is built by
        // the first iteration and reused by the others (a product with fewer samples than atoms takes
        // the planar-rows form instead, which images V and ignores this flag)
        a.ext_ready = i > 0 && gemm_route<FORM_NN>(a).image != IMG_ROWS_A;
        // float32, >= 512 atoms, at least one 128 x 128 tile per two CUs: the 8-wave 128 x 128 x 64 tile
        // (8192 x 512 x 512: 45 us against 50 us on the 64 x 64 tile for the bare product; dictionary step
        // 1.64 -> 1.62 ms).  complex64 measured slower on it and keeps the automatic choice.
        if (std::is_same<T, float>::value && K >= 512 && (long)ceil_div(N, 128) * ceil_div(K, 128) >= 128)
            a.tile = TILE_MID;
        EpiProxStepH<T, PROX> epih{w.yAt, P, Nw, Vn, (long)K, w.scal, w.alphak, w.tolk,
                                   coef, check, (check || mom) ? 1 : 0, w.flag};
        if (is_last && method != DCP_LASSO_ACC_ISTA) {   // the iterate lasso.py:297 / :415 return
            epih.xfinal = p.X;
            epih.sdiv = w.s;
            wrote_final = true;
        }
        DCP_LAUNCH_OK(p.h, (gemm<FORM_NN>(p.st, a, epih)));
        return DCP_OK;
    };
    ProxLoopResult<T> res;
    DCP_TRY(prox_gradient_loop<T>(p.h, w.xb, method, p.maxiter, w.flag, p.host_flag, step, &res));
    *out = LassoOutcome<T>{res.it, res.result, wrote_final && !res.converged};
    return DCP_OK;
}

// X = x / s (lasso.py:189) unless the solver's last epilogue wrote it, the optional synchronisation, *it_out.
template <class T>
inline int lasso_finish(const LassoProblem<T>& p, const LassoOutcome<T>& out, int* it_out) {
    if (!out.final_in_place) {
        hipLaunchKernelGGL((col_scale_kernel<T>), dim3(grid_for((long)p.N * p.K)), dim3(256), 0, p.st,
                           (const T*)out.result, (const real_t<T>*)p.w.s, (long)p.N, (long)p.K, 0, p.X);
        DCP_LAUNCH_OK(p.h, hipGetLastError());
    }
    if (!p.extra.no_final_sync) DCP_HIP_OK(p.h, hipStreamSynchronize(p.st));
    *it_out = out.it;
    return DCP_OK;
}

// solve_fastpath (lasso.py:97-189).  Y [N,F], A [K,F], X [N,K] (in: initial estimate, out:
// solution), mask: null, [F] (mask_ndim 1) or [N,F] (mask_ndim 2).  *it_out as the reference.
template <class T, int PROX>
inline int lasso_solve(dcp_handle* h, const T* Y, const real_t<T>* mask, int mask_ndim, const T* A,
                       T* X, int64_t N64, int64_t F64, int64_t K64, real_t<T> alpha, real_t<T> tol,
                       int maxiter, int method, int* it_out, LassoWs<T>& w,
                       const LassoExtra& extra = LassoExtra()) {
    typedef real_t<T> R;
    h->lasso_deferred_flag = nullptr;   // (a deferral an earlier, failed call never settled dies here)
    h->lasso_deferred_it = nullptr;
    h->lasso_deferred_copy = false;
    void* hostv = nullptr;
    DCP_TRY(host_scratch(h, 64, &hostv));
    const LassoProblem<T> p{h, h->stream, (int)N64, (int)F64, (int)K64, mask, mask_ndim,
                            mask_ndim == 2 ? (const R*)w.rowscale : nullptr, X, w, reinterpret_cast<int*>(hostv),
                            maxiter, extra};
    const bool prox = method == DCP_LASSO_ISTA || method == DCP_LASSO_ACC_ISTA || method == DCP_LASSO_FISTA;
    // ista / acc_ista / fista without a 2-D mask: x * s is formed by hform_prepare_kernel in its pass over [N, K]
    DCP_TRY(lasso_prepare<T>(p, Y, A, alpha, tol, !(prox && mask_ndim != 2)));
    LassoOutcome<T> out{maxiter - 1, w.xb[0], false};
    if (method == DCP_LASSO_PARALLEL_CD) DCP_TRY((lasso_pcd<T, PROX>(p, it_out, &out)));
    else if (method == DCP_LASSO_ADMM && mask_ndim != 2) DCP_TRY((lasso_admm<T, PROX>(p, &out)));
    else if (method == DCP_LASSO_ADMM) DCP_TRY((lasso_admm_rows<T, PROX>(p, &out)));
    else if (method == DCP_LASSO_CD && mask_ndim != 2) DCP_TRY((lasso_cd_gram<T, PROX>(p, false, it_out, &out)));
    else if (method == DCP_LASSO_CD) DCP_TRY((lasso_cd_rows<T, PROX>(p, &out)));
    else DCP_TRY((lasso_prox<T, PROX>(p, method, &out)));
    return lasso_finish<T>(p, out, it_out);
}

}  // namespace dcp
