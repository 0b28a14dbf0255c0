// The GEMM epilogues: functors that fuse a solver's per-element update rule into the product that yields its
// last operand.  All are called as epi(row, col, acc, split).  A functor may also offer the 16-byte forms the
// cores look for (vec4: four float columns of a row, gemm_mfma_f32.hpp; cvec2: two complex64 columns, gemm.hpp;
// quot4: the denominator tail, gemm_mfma_bf16x6.hpp).  Which form runs is decided per launch from shapes and
// addresses, so the rule of this file is: a formula is written ONCE, as a function of one element, and the forms
// differ only in how they move data -- each loads, calls that function per element, and stores.
#pragma once
#include <stdint.h>
#include <type_traits>

#include "reduce.hpp"
#include "scalar.hpp"

namespace dcp {

// ------------------------------------------------------------------ vocabulary ----
// The MU quotient  x * max(num, 0) / max(den, 1e-15)  (grads.py:84,93) ...
template <class T>
__device__ __forceinline__ T mu_quotient(T x, T num, T den) {
    return x * max_np(num, T(0)) / max_np(den, T(1.0e-15));
}
// ... with the L1/L2 penalty on the codes in the denominator, den + l1 + l2 x (written out, numerator first: the
// kernels that take it keep the instruction schedule they had) ...
template <class T>
__device__ __forceinline__ T mu_quotient(T x, T num, T den, T l1, T l2) {
    return x * max_np(num, T(0)) / max_np(den + l1 + l2 * x, T(1.0e-15));
}
// ... and under a compile-time PEN, for a denominator that arrives as a value (a GEMM accumulator, a slab sum):
// the penalty goes onto it first (without PEN l1 and l2 are not read).
template <bool PEN, class T>
__device__ __forceinline__ T mu_quotient_if(T x, T num, T den, T l1, T l2) {
    if constexpr (PEN) den = den + l1 + l2 * x;
    return mu_quotient(x, num, den);
}

// 16 bytes of floats at p; at columns c0 .. of row r of an array with leading dimension ld (in elements of P: four
// floats, or two complex64).
__device__ __forceinline__ f32x4 load4(const void* p) { return *reinterpret_cast<const f32x4*>(p); }
__device__ __forceinline__ void store4(void* p, f32x4 v) { *reinterpret_cast<f32x4*>(p) = v; }
template <class P>
__device__ __forceinline__ f32x4 row4(const P* p, int r, long ld, int c0) { return load4(p + (long)r * ld + c0); }
template <class P>
__device__ __forceinline__ void store_row4(P* p, int r, long ld, int c0, f32x4 v) { store4(p + (long)r * ld + c0, v); }

// Host: may the 16-byte form run?  Every pointer named is 16-byte aligned (a null one is) and every leading
// dimension a multiple of Q elements (4 floats, 2 complex64).
inline bool al16_ptr(const void* q) { return (reinterpret_cast<uintptr_t>(q) & 15) == 0; }
template <int Q>
inline bool al16_one(const void* q) { return al16_ptr(q); }
template <int Q>
inline bool al16_one(long ld) { return (ld % Q) == 0; }
template <int Q = 4, class... A>
inline bool aligned16(A... a) { return (al16_one<Q>(a) && ...); }

// ------------------------------------------------------------------ stores ----
template <class T>
struct EpiStore {  // C[row, col] = acc
    // 16-byte epilogue available but OFF (interleaved in-process A/B, tools/vec_ab.py): x.D 16384x4096x256
    // 0.326 ms with it, 0.318 without: for a pure store the quad transposes cost as much VALU issue as the
    // narrower stores save.  It pays where the epilogue also LOADS per element (EpiMuNum: 1.045 -> 1.010 ms
    // on the dominant kernel).
    static constexpr bool kVec4 = false;
    T* C;
    long ldc;
    __device__ __forceinline__ void operator()(int r, int c, T v, int) const {
        C[(long)r * ldc + c] = v;
    }
    bool vec_ok() const { return aligned16(C, ldc); }
    __device__ __forceinline__ void vec4(int r, int c0, f32x4 v, int) const {
        store_row4(reinterpret_cast<float*>(C), r, ldc, c0, v);
    }
};

template <class T>
struct EpiStoreSub {  // C[row, col] = acc - sub  (the HALS x sweep's C = Y D^T - l1 under an L1 penalty)
    static constexpr bool kVec4 = false;
    T* C;
    long ldc;
    T sub;
    __device__ __forceinline__ void operator()(int r, int c, T v, int) const {
        C[(long)r * ldc + c] = v - sub;
    }
};

template <class T>
struct EpiSlab {  // split-K partial: slab[split][row, col] = acc
    static constexpr bool kVec4 = false;   // neutral in the A/B (1.134 vs 1.130 ms on x^T.Y): off
    T* slab;
    long ldc;
    long slab_stride;
    __device__ __forceinline__ void operator()(int r, int c, T v, int s) const {
        slab[(long)s * slab_stride + (long)r * ldc + c] = v;
    }
    bool vec_ok() const { return aligned16(slab, ldc, slab_stride); }
    __device__ __forceinline__ void vec4(int r, int c0, f32x4 v, int s) const {
        store_row4(reinterpret_cast<float*>(slab) + (long)s * slab_stride, r, ldc, c0, v);
    }
    // pair schedule of the fp32 MFMA core (TileCfg PIPE = 3): two adjacent columns in one 8-byte store
    static constexpr bool kVec2 = std::is_same<T, float>::value;
    bool vec2_ok() const {
        return (reinterpret_cast<uintptr_t>(slab) & 7) == 0 && (ldc % 2) == 0 && (slab_stride % 2) == 0;
    }
    __device__ __forceinline__ void store2(int r, int c0, float v0, float v1, int s) const {
        typedef float f32x2 __attribute__((ext_vector_type(2)));
        *reinterpret_cast<f32x2*>(reinterpret_cast<float*>(slab) + (long)s * slab_stride + (long)r * ldc + c0) =
            f32x2{v0, v1};
    }
};

// ------------------------------------------------------------------ the MU quotient ----
// out = mu_quotient(cur, acc, den): acc is the POSITIVE gradient part (grads.py:84 with grad_pos produced by this
// GEMM).  den: full matrix (ld_den > 0) or one value per column (ld_den == 0), e.g. KL's colsum(D).
template <class T>
struct EpiMuNum {
    static constexpr bool kVec4 = std::is_same<T, float>::value;
    const T* cur;
    long ld_cur;
    const T* den;
    long ld_den;
    T* out;
    long ld_out;
    __device__ __forceinline__ void operator()(int r, int c, T v, int) const {
        const T d = den[(long)r * ld_den + c];
        out[(long)r * ld_out + c] = mu_quotient(cur[(long)r * ld_cur + c], v, d);
    }
    // (ld_den == 0: one denominator per column, read as 4 consecutive values of the vector)
    bool vec_ok() const { return aligned16(cur, den, out, ld_cur, ld_den, ld_out); }
    __device__ __forceinline__ void vec4(int r, int c0, f32x4 v, int) const {
        const f32x4 d = row4(reinterpret_cast<const float*>(den), r, ld_den, c0);
        const f32x4 x = row4(reinterpret_cast<const float*>(cur), r, ld_cur, c0);
        f32x4 o;
#pragma unroll
        for (int e = 0; e < 4; ++e) o[e] = mu_quotient(x[e], v[e], d[e]);
        store_row4(reinterpret_cast<float*>(out), r, ld_out, c0, o);
    }
};

// EpiMuNum with the L1/L2 penalty on the codes.  A type of its own, so that the unpenalised instantiations stay
// exactly as they are; l1 / l2 are uniform kernel arguments (SGPRs).
template <class T>
struct EpiMuNumPen : EpiMuNum<T> {
    T l1, l2;
    __device__ __forceinline__ void operator()(int r, int c, T v, int) const {
        const T d = this->den[(long)r * this->ld_den + c];
        const T x = this->cur[(long)r * this->ld_cur + c];
        this->out[(long)r * this->ld_out + c] = mu_quotient(x, v, d, l1, l2);
    }
    __device__ __forceinline__ void vec4(int r, int c0, f32x4 v, int) const {
        const f32x4 d = row4(reinterpret_cast<const float*>(this->den), r, this->ld_den, c0);
        const f32x4 x = row4(reinterpret_cast<const float*>(this->cur), r, this->ld_cur, c0);
        f32x4 o;
#pragma unroll
        for (int e = 0; e < 4; ++e) o[e] = mu_quotient(x[e], v[e], d[e], (float)l1, (float)l2);
        store_row4(reinterpret_cast<float*>(this->out), r, this->ld_out, c0, o);
    }
};

// EpiMuNum / EpiMuNumPen whose denominator cur . gram is formed by the product's own workgroup (the denominator
// tail of the 256 x 256 split-bf16 NT kernel, gemm_mfma_bf16x6.hpp) and never stored:
//   out = mu_quotient(cur, acc, den [, l1, l2]),   den = (cur . gram)[r, c]
// The quotient is the function EpiMuNum calls, so out is bitwise what the two-kernel path gives.
template <bool PEN>
struct EpiMuGramDen {
    static constexpr bool kVec4 = true;
    static constexpr bool kDenTail = true;
    const float* cur;
    long ld_cur;
    const float* gram;   // [depth, depth]
    long ld_gram;
    int depth;
    float* out;
    long ld_out;
    float l1 = 0.0f, l2 = 0.0f;
    bool vec_ok() const { return aligned16(cur, gram, out, ld_cur, ld_gram, ld_out); }
    __device__ __forceinline__ void quot4(int r, int c0, f32x4 v, f32x4 d) const {
        const f32x4 x = row4(cur, r, ld_cur, c0);
        f32x4 o;
#pragma unroll
        for (int e = 0; e < 4; ++e) {
            if constexpr (PEN) o[e] = mu_quotient(x[e], v[e], d[e], l1, l2);
            else o[e] = mu_quotient(x[e], v[e], d[e]);
        }
        store_row4(out, r, ld_out, c0, o);
    }
};

// out = mu_quotient(cur, num, acc): acc is the NEGATIVE gradient part.
template <class T>
struct EpiMuDen {
    const T* cur;
    long ld_cur;
    const T* num;
    long ld_num;
    T* out;
    long ld_out;
    __device__ __forceinline__ void operator()(int r, int c, T v, int) const {
        const T nu = num[(long)r * ld_num + c];
        out[(long)r * ld_out + c] = mu_quotient(cur[(long)r * ld_cur + c], nu, v);
    }
};

// Split-K numerator: out = mu_quotient(cur, sum_s slab_s, acc [, l1, l2]).  acc is the NEGATIVE part (x.G);
// the positive part (Y.D^T) arrives as S ordered split-K partials, summed here in the fixed order
// 0..S-1 (slab_sum, as mu_quotient_slabs_kernel does).  With few rows per GPU the Y.D^T product splits its
// reduction; the quotient then rides on the x.G product (16-byte epilogue) instead of a pass of its own.
// PEN: the L1/L2 penalty on the codes; without it l1 and l2 are not read.
template <class T, bool PEN>
struct EpiMuDenSlabs {
    static constexpr bool kVec4 = std::is_same<T, float>::value;
    const T* cur;
    long ld_cur;
    const T* slabs;      // [S][rows, ld_slab]
    long ld_slab;
    long slab_stride;
    int S;
    T* out;
    long ld_out;
    T l1 = T(0), l2 = T(0);
    __device__ __forceinline__ void operator()(int r, int c, T v, int) const {
        const T nu = slab_sum(slabs, slab_stride, S, (long)r * ld_slab + c);
        const T x = cur[(long)r * ld_cur + c];
        out[(long)r * ld_out + c] = mu_quotient_if<PEN>(x, nu, v, l1, l2);
    }
    bool vec_ok() const { return aligned16(cur, slabs, out, ld_cur, ld_slab, slab_stride, ld_out); }
    __device__ __forceinline__ void vec4(int r, int c0, f32x4 v, int) const {
        if constexpr (std::is_same<T, float>::value) {
            const f32x4 nu = slab_sum(reinterpret_cast<const f32x4*>(slabs + (long)r * ld_slab + c0), slab_stride / 4, S, 0L);
            const f32x4 x = row4(cur, r, ld_cur, c0);
            f32x4 q;
#pragma unroll
            for (int e = 0; e < 4; ++e) q[e] = mu_quotient_if<PEN>(x[e], nu[e], v[e], l1, l2);
            store_row4(out, r, ld_out, c0, q);
        }
    }
};

// ------------------------------------------------------------------ masks ----
// out = acc * mask  (f = (x.D) o M, grads.py:113,123): the element function is scale()
template <class T>
struct EpiMulMask {
    const real_t<T>* mask;
    long ld_mask;
    T* out;
    long ld_out;
    __device__ __forceinline__ void operator()(int r, int c, T v, int) const {
        out[(long)r * ld_out + c] = scale(v, mask[(long)r * ld_mask + c]);
    }
    static constexpr bool kVec4 = std::is_same<T, float>::value;   // one load per element: 16-byte form
    bool vec_ok() const { return aligned16(mask, out, ld_mask, ld_out); }
    __device__ __forceinline__ void vec4(int r, int c0, f32x4 v, int) const {
        if constexpr (std::is_same<T, float>::value) {
            const f32x4 m = row4(mask, r, ld_mask, c0);
            f32x4 o;
#pragma unroll
            for (int e = 0; e < 4; ++e) o[e] = scale(v[e], m[e]);
            store_row4(out, r, ld_out, c0, o);
        }
    }
};

// out = acc * mask for a BINARY mask handed over as row bits (see epi_rowbits in gemm_mfma_f32.hpp):
// the factor is exactly 1.0f or 0.0f and the product is formed as in EpiMulMask (so NaN / Inf / -0
// behave as the reference's  f * mask).  float only (the fp32 MFMA core implements the protocol).
struct EpiMulMaskBits {
    static constexpr bool kRowBits = true;
    const uint32_t* bits;   // [(rows + 31) / 32][ld_bits]
    long ld_bits;
    float* out;
    long ld_out;
    __device__ __forceinline__ uint32_t load_bits(int row0, int col) const {
        return bits[(long)(row0 >> 5) * ld_bits + col];
    }
    __device__ __forceinline__ void with_bit(int r, int c, float v, uint32_t bit, int) const {
        out[(long)r * ld_out + c] = scale(v, bit ? 1.0f : 0.0f);
    }
    __device__ __forceinline__ void operator()(int, int, float, int) const {}
};

// out = w y + (1 - w) acc,  w = mask in [0, 1]: the data with its missing part filled in from the current model
// (the E step of em-hals, nmf_hals.hip).  Formed as one multiply (1 - w) acc and one fma with w y, so that for
// finite operands w == 1 returns y and w == 0 returns acc bit for bit.  No select: every element loads y and w
// and runs the same two operations.
__device__ __forceinline__ float fma_np(float a, float b, float c) { return __builtin_fmaf(a, b, c); }
__device__ __forceinline__ double fma_np(double a, double b, double c) { return __builtin_fma(a, b, c); }
template <class T>
struct EpiImpute {
    const T* y;      // y, mask and out are [rows, ld] with one leading dimension: one offset per element
    const T* mask;
    T* out;
    long ld;
    __device__ __forceinline__ static T fill(T w, T yy, T v) {
        const T t = (T(1) - w) * v;
        return fma_np(w, yy, t);
    }
    __device__ __forceinline__ void operator()(int r, int c, T v, int) const {
        const long o = (long)r * ld + c;
        const T w = mask[o];
        const T yy = y[o];
        out[o] = fill(w, yy, v);
    }
    static constexpr bool kVec4 = std::is_same<T, float>::value;   // two loads per element: 16-byte form
    bool vec_ok() const { return aligned16(y, mask, out, ld); }
    __device__ __forceinline__ void vec4(int r, int c0, f32x4 v, int) const {
        if constexpr (std::is_same<T, float>::value) {
            const long o = (long)r * ld + c0;
            const f32x4 w = load4(mask + o);
            const f32x4 yy = load4(y + o);
            f32x4 q;
#pragma unroll
            for (int e = 0; e < 4; ++e) q[e] = fill(w[e], yy[e], v[e]);
            store4(out + o, q);
        }
    }
};

// KL ratio: out = (y [* mask]) / (acc + 1e-15)   (grads.py:145-149,154-158)
template <class T>
struct EpiKlRatio {
    const T* y;
    long ld_y;
    const T* mask;  // nullable
    long ld_mask;
    T* out;
    long ld_out;
    __device__ __forceinline__ static T ratio(T ym, T v) { return ym / (v + T(1.0e-15)); }   // ym: y, masked
    __device__ __forceinline__ void operator()(int r, int c, T v, int) const {
        T yy = y[(long)r * ld_y + c];
        if (mask != nullptr) yy = yy * mask[(long)r * ld_mask + c];
        out[(long)r * ld_out + c] = ratio(yy, v);
    }
    static constexpr bool kVec4 = std::is_same<T, float>::value;
    bool vec_ok() const { return aligned16(y, out, ld_y, ld_out) && (mask == nullptr || aligned16(mask, ld_mask)); }
    __device__ __forceinline__ void vec4(int r, int c0, f32x4 v, int) const {
        if constexpr (std::is_same<T, float>::value) {
            f32x4 yy = row4(y, r, ld_y, c0);
            if (mask != nullptr) yy = yy * row4(mask, r, ld_mask, c0);
            f32x4 o;
#pragma unroll
            for (int e = 0; e < 4; ++e) o[e] = ratio(yy[e], v[e]);
            store_row4(out, r, ld_out, c0, o);
        }
    }
};

// ---- beta-divergence (DCP_LIK_BETA) ------------------------------------------------------------------
// Exponent forms of the two parts R1 = (Y o M) o V^(beta-2), R2 = M o V^(beta-1), V = acc + 1e-15: closed
// forms for the common betas, one log2 + one exp2 per element otherwise.
enum BetaMode { BETA_0 = 0, BETA_HALF = 1, BETA_1 = 2, BETA_3HALF = 3, BETA_2 = 4, BETA_3 = 5, BETA_GEN = 6 };
inline int beta_mode(double b) {
    return b == 0.0 ? BETA_0 : b == 0.5 ? BETA_HALF : b == 1.0 ? BETA_1 : b == 1.5 ? BETA_3HALF
         : b == 2.0 ? BETA_2 : b == 3.0 ? BETA_3 : BETA_GEN;
}
__device__ __forceinline__ float beta_rsqrt(float v) { return rsqrtf(v); }
__device__ __forceinline__ double beta_rsqrt(double v) { return rsqrt(v); }
__device__ __forceinline__ float beta_pow(float v, float e) { return exp2f(e * log2f(v)); }
__device__ __forceinline__ double beta_pow(double v, double e) { return exp(e * log(v)); }

template <class T>
__device__ __forceinline__ void beta_parts(int mode, T e, T acc, T ym, T m, T& r1, T& r2) {
    const T v = acc + T(1.0e-15);
    switch (mode) {
    case BETA_0: { const T r = T(1) / v; r1 = ym * r * r; r2 = m * r; break; }
    case BETA_HALF: { const T s = beta_rsqrt(v); r1 = ym * (s * s * s); r2 = m * s; break; }
    case BETA_1: { r1 = ym / v; r2 = m; break; }
    case BETA_3HALF: { const T s = beta_rsqrt(v); r1 = ym * s; r2 = m * (s * v); break; }
    case BETA_2: { r1 = ym; r2 = m * v; break; }
    case BETA_3: { r1 = ym * v; r2 = m * (v * v); break; }
    default: { const T p = beta_pow(v, e); r1 = ym * p; r2 = m * (p * v); break; }
    }
}

// Forward product of a beta step: both gradient operands in one pass over x.D.
//   r1 = (Y o M) o V^(beta-2),  r2 = M o V^(beta-1)       (M = 1 without a mask)
// ym is Y o M (the caller's pre-masked Y); mode = beta_mode(beta), e = beta - 2.
template <class T>
struct EpiBetaParts {
    static constexpr bool kVec4 = std::is_same<T, float>::value;
    const T* ym;
    long ld_y;
    const T* mask;  // nullable
    long ld_mask;
    int mode;
    T e;
    T* r1;
    T* r2;
    long ld_out;
    __device__ __forceinline__ void operator()(int r, int c, T v, int) const {
        const T m = mask != nullptr ? mask[(long)r * ld_mask + c] : T(1);
        T a, b;
        beta_parts<T>(mode, e, v, ym[(long)r * ld_y + c], m, a, b);
        r1[(long)r * ld_out + c] = a;
        r2[(long)r * ld_out + c] = b;
    }
    bool vec_ok() const {
        return aligned16(ym, r1, r2, ld_y, ld_out) && (mask == nullptr || aligned16(mask, ld_mask));
    }
    __device__ __forceinline__ void vec4(int r, int c0, f32x4 v, int) const {
        if constexpr (std::is_same<T, float>::value) {
            const f32x4 yy = row4(ym, r, ld_y, c0);
            f32x4 m = {1.0f, 1.0f, 1.0f, 1.0f};
            if (mask != nullptr) m = row4(mask, r, ld_mask, c0);
            f32x4 a, b;
#pragma unroll
            for (int i = 0; i < 4; ++i) {
                float ai, bi;
                beta_parts<float>(mode, e, v[i], yy[i], m[i], ai, bi);
                a[i] = ai;
                b[i] = bi;
            }
            store_row4(r1, r, ld_out, c0, a);
            store_row4(r2, r, ld_out, c0, b);
        }
    }
};

// d_beta(y | v) in double (Fevotte & Idier 2011):
//   beta = 0: y/v - log(y/v) - 1     beta = 1: y log(y/v) - y + v  (0 log 0 = 0)
//   otherwise (y^beta + (beta-1) v^beta - beta y v^(beta-1)) / (beta (beta-1))
__device__ __forceinline__ double beta_divergence_elem(double beta, double y, double v) {
    if (beta == 0.0) {
        const double q = y / v;
        return q - log(q) - 1.0;
    }
    if (beta == 1.0) return (y > 0.0 ? y * log(y / v) : 0.0) - y + v;
    if (beta == 2.0) {
        const double d = y - v;
        return 0.5 * d * d;
    }
    return (pow(y, beta) + (beta - 1.0) * pow(v, beta) - beta * y * pow(v, beta - 1.0)) / (beta * (beta - 1.0));
}

// out = M o d_beta(Y | acc + 1e-15), an entry with M == 0 contributing exactly 0 (reduced by reduce_partial_kernel: SumOp over MapValue)
template <class T>
struct EpiBetaDivergence {
    const T* y;
    long ld_y;
    const T* mask;  // nullable
    long ld_mask;
    double beta;
    T* out;
    long ld_out;
    __device__ __forceinline__ void operator()(int r, int c, T v, int) const {
        const double m = mask != nullptr ? (double)mask[(long)r * ld_mask + c] : 1.0;
        double d = 0.0;
        if (m != 0.0) d = m * beta_divergence_elem(beta, (double)y[(long)r * ld_y + c], (double)v + 1.0e-15);
        out[(long)r * ld_out + c] = (T)d;
    }
};

// Residual: out = (y - acc) [* mask]   (parity metric; reduced by reduce_partial_kernel: SumOp over MapAbs2)
template <class T>
struct EpiResidual {
    const T* y;
    long ld_y;
    const real_t<T>* mask;  // nullable
    long ld_mask;
    T* out;
    long ld_out;
    __device__ __forceinline__ void operator()(int r, int c, T v, int) const {
        T d = sub(y[(long)r * ld_y + c], v);
        if (mask != nullptr) d = scale(d, mask[(long)r * ld_mask + c]);
        out[(long)r * ld_out + c] = d;
    }
};

}  // namespace dcp
