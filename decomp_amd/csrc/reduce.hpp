// The reduction vocabulary of the small kernels, defined once: cross-lane moves, wave and workgroup sums and maxima,
// the flat (map, reduce) kernel pair, the ordered slab sum and the publication of a finished maximum.  Every sum here
// has one fixed order, spelled out at its definition; the results are bitwise reproducible because every kernel sums
// through these and nothing else.  No float atomics.
#pragma once
#include <hip/hip_runtime.h>
#include "scalar.hpp"

namespace dcp {

// ---- cross-lane moves (wave64; cx moves .re and .im) ---------------------------------------------
// v of lane (lane ^ m)
__device__ __forceinline__ int    lane_xor(int v, int m)    { return __shfl_xor(v, m, 64); }
__device__ __forceinline__ float  lane_xor(float v, int m)  { return __shfl_xor(v, m, 64); }
__device__ __forceinline__ double lane_xor(double v, int m) { return __shfl_xor(v, m, 64); }
template <class R>
__device__ __forceinline__ cx<R> lane_xor(cx<R> v, int m) { return cx<R>{lane_xor(v.re, m), lane_xor(v.im, m)}; }

// v of lane (lane + o); the lanes whose source is past the wave keep their own v
__device__ __forceinline__ int    lane_down(int v, int o)    { return __shfl_down(v, o, 64); }
__device__ __forceinline__ float  lane_down(float v, int o)  { return __shfl_down(v, o, 64); }
__device__ __forceinline__ double lane_down(double v, int o) { return __shfl_down(v, o, 64); }

// v of lane l, l any per-lane index (ds_bpermute)
__device__ __forceinline__ float  lane_get(float v, int l)  { return __shfl(v, l, 64); }
__device__ __forceinline__ double lane_get(double v, int l) { return __shfl(v, l, 64); }
template <class R>
__device__ __forceinline__ cx<R> lane_get(cx<R> v, int l) { return cx<R>{lane_get(v.re, l), lane_get(v.im, l)}; }

// v of lane l in every lane; l is wave-uniform (v_readlane_b32)
__device__ __forceinline__ float lane_bcast(float v, int l) {
    return __int_as_float(__builtin_amdgcn_readlane(__float_as_int(v), l));
}
__device__ __forceinline__ double lane_bcast(double v, int l) {
    const long long b = __double_as_longlong(v);
    const int lo = __builtin_amdgcn_readlane((int)(b & 0xffffffffLL), l);
    const int hi = __builtin_amdgcn_readlane((int)(b >> 32), l);
    return __longlong_as_double(((long long)hi << 32) | (unsigned int)lo);
}
template <class R>
__device__ __forceinline__ cx<R> lane_bcast(cx<R> v, int l) { return cx<R>{lane_bcast(v.re, l), lane_bcast(v.im, l)}; }

// ---- wave reductions -----------------------------------------------------------------------------
// lane 0 <- v[0] + v[32], then + the lanes 16, 8, 4, 2, 1 further on (six shift-down steps, offsets 32 .. 1)
template <class R>
__device__ __forceinline__ R wave_sum(R v) {
#pragma unroll
    for (int o = 32; o > 0; o >>= 1) v += lane_down(v, o);
    return v;
}
// lane 0 <- the maximum, by the same steps; NaN propagates, as in np.max
template <class R>
__device__ __forceinline__ R wave_max(R v) {
#pragma unroll
    for (int o = 32; o > 0; o >>= 1) v = max_np(lane_down(v, o), v);
    return v;
}
// the sum over the 64 lanes, the same bits in every lane: a butterfly, offsets 32 .. 1 (a + b == b + a at every step)
template <class T>
__device__ __forceinline__ T wave_sum_all(T v) {
#pragma unroll
    for (int m = 32; m >= 1; m >>= 1) v = add(v, lane_xor(v, m));
    return v;
}

// Sum of one double per lane over the 64 lanes of a wave, with DPP row shifts / row broadcasts
// (VALU latency) instead of the LDS crossbar of __shfl_xor (six dependent ds_bpermute pairs are
// the longest chain of a recursion step otherwise).  Invalid / masked-out source lanes contribute
// +0.0 (bound_ctrl, old = 0).  The total lands in lane 63 and is read back as a wave-uniform value.
template <int CTRL, int ROW_MASK>
__device__ __forceinline__ double dpp_add_f64(double x) {
    const int lo = __double2loint(x), hi = __double2hiint(x);
    const int slo = __builtin_amdgcn_update_dpp(0, lo, CTRL, ROW_MASK, 0xf, true);
    const int shi = __builtin_amdgcn_update_dpp(0, hi, CTRL, ROW_MASK, 0xf, true);
    return x + __hiloint2double(shi, slo);
}
__device__ __forceinline__ double wave_sum_f64(double x) {
    x = dpp_add_f64<0x111, 0xf>(x);   // row_shr:1
    x = dpp_add_f64<0x112, 0xf>(x);   // row_shr:2
    x = dpp_add_f64<0x114, 0xf>(x);   // row_shr:4
    x = dpp_add_f64<0x118, 0xf>(x);   // row_shr:8   -> lane 15 of every row holds its row sum
    x = dpp_add_f64<0x142, 0xa>(x);   // row_bcast:15 into rows 1 and 3
    x = dpp_add_f64<0x143, 0xc>(x);   // row_bcast:31 into rows 2 and 3 -> lane 63 holds the total
    const int lo = __builtin_amdgcn_readlane(__double2loint(x), 63);
    const int hi = __builtin_amdgcn_readlane(__double2hiint(x), 63);
    return __hiloint2double(hi, lo);
}

// ---- workgroup reductions: WAVES waves (256 threads by default), sh holds WAVES values; the result is valid in
// thread 0: the wave results left to right, sh[0] + sh[1] + sh[2] + sh[3].  Both barriers are inside, so one sh serves
// any number of calls in a row. ----
struct SumOp {
    template <class R> static __device__ __forceinline__ R join(R acc, R v) { return acc + v; }
    template <class R> static __device__ __forceinline__ R wave(R v) { return wave_sum(v); }
};
struct MaxOp {   // NaN propagates (np.max)
    template <class R> static __device__ __forceinline__ R join(R acc, R v) { return max_np(v, acc); }
    template <class R> static __device__ __forceinline__ R wave(R v) { return wave_max(v); }
};
template <class Op, int WAVES = 4, class R>
__device__ __forceinline__ R block_reduce(R v, R* sh) {
    v = Op::wave(v);
    const int lane = threadIdx.x & 63, w = threadIdx.x >> 6;
    if (lane == 0) sh[w] = v;
    __syncthreads();
    R r = 0;
    if (threadIdx.x == 0) {
        r = sh[0];
        for (int i = 1; i < WAVES; ++i) r = Op::join(r, sh[i]);
    }
    __syncthreads();
    return r;
}
template <int WAVES = 4, class R>
__device__ __forceinline__ R block_sum_256(R v, R* sh) { return block_reduce<SumOp, WAVES>(v, sh); }
template <int WAVES = 4, class R>
__device__ __forceinline__ R block_max_256(R v, R* sh) { return block_reduce<MaxOp, WAVES>(v, sh); }
// the sum of a T given as its parts: the real parts, then (complex T only) the imaginary parts
template <class T>
__device__ __forceinline__ T block_sum_256_parts(real_t<T> re, real_t<T> im, real_t<T>* sh) {
    const real_t<T> tre = block_sum_256(re, sh);
    if constexpr (scalar_traits<T>::is_complex) return T{tre, block_sum_256(im, sh)};
    else return tre;
}

// ---- the flat reductions ---------------------------------------------------------------------------
// partial[block] = Out(reduce_i map(i)) over the workgroup's grid-stride share of [0, n): every thread folds its
// elements in increasing i, then block_reduce.  The accumulation type is what map returns; the number of workgroups
// is part of the order (the caller reduces `partial` in block order).
template <class Op, class Map, class Out>
__global__ void __launch_bounds__(256) reduce_partial_kernel(Map map, long n, Out* __restrict__ partial) {
    typedef decltype(map(0L)) A;
    __shared__ A sh[4];
    A acc = 0;
    for (long i = blockIdx.x * 256L + threadIdx.x; i < n; i += (long)gridDim.x * 256L) acc = Op::join(acc, map(i));
    const A t = block_reduce<Op>(acc, sh);
    if (threadIdx.x == 0) partial[blockIdx.x] = (Out)t;
}
// One workgroup: fin(reduce_i v[i]) in thread 0 (a maximum is over values >= 0).
template <class Op, class R, class Fin>
__global__ void __launch_bounds__(256) reduce_vector_kernel(const R* __restrict__ v, long n, Fin fin) {
    __shared__ R sh[4];
    R acc = 0;
    for (long i = threadIdx.x; i < n; i += 256) acc = Op::join(acc, v[i]);
    const R t = block_reduce<Op>(acc, sh);
    if (threadIdx.x == 0) fin(t);
}
template <class R>
struct FinStore {   // out[0] = the result
    R* out;
    __device__ __forceinline__ void operator()(R t) const { out[0] = t; }
};
// out[0] = max_i v[i] (v >= 0), one workgroup
template <class R>
inline void launch_final_max(hipStream_t st, const R* v, long n, R* out) {
    hipLaunchKernelGGL((reduce_vector_kernel<MaxOp, R, FinStore<R>>), dim3(1), dim3(256), 0, st, v, n, FinStore<R>{out});
}

// the maps: each returns its summand in the accumulation type
template <class T>
struct MapAbs2 {   // |a_i|^2, squared in T, summed in double (residual norm)
    const T* a;
    __device__ __forceinline__ double operator()(long i) const { return (double)abs2(a[i]); }
};
template <class T>
struct MapValue {   // a_i in double
    const T* a;
    __device__ __forceinline__ double operator()(long i) const { return (double)a[i]; }
};
template <class T>
struct MapNegative {   // 1 where `x >= 0` fails (so NaN counts, exactly as assertion.py:99-100 fails on it)
    const T* x;
    __device__ __forceinline__ double operator()(long i) const { return (x[i] >= T(0)) ? 0.0 : 1.0; }
};
// Gaussian.logp (grads.py:127-135), summand (-0.5 ((y - f) / scale)^2 - log(scale) - pi / 2) [* mask], d = y - f given
template <class T>
struct MapGaussLogp {
    const T* d;
    const T* mask;
    double inv_scale, cst;
    __device__ __forceinline__ double operator()(long i) const {
        const double z = (double)d[i] * inv_scale;
        double t = -0.5 * z * z - cst;
        if (mask != nullptr) t *= (double)mask[i];
        return t;
    }
};
template <class T>
struct MapAbsDiff {   // |a_i - b_i|
    const T* a;
    const T* b;
    __device__ __forceinline__ real_t<T> operator()(long i) const { return absval(sub(a[i], b[i])); }
};

// ---- the ordered slab sum ------------------------------------------------------------------------
// sum_s slabs[s * stride + i], s = 0 .. S-1 left to right (bitwise reproducible).  DEPTHS = the loads kept in flight,
// largest first: rounds of that many slabs while they last, then one at a time -- one at a time the loop is a chain
// of L2 round trips (16 us for 64 slabs of a 64 x 64 Gram matrix; eight in flight: 5.9 us).  The order is the same for
// every DEPTHS.  T: a scalar, cx, or a 16-byte vector of reals (element-wise, so the same bits per element).
typedef double f64x2 __attribute__((ext_vector_type(2)));
DCP_HD f32x4 add(f32x4 a, f32x4 b) { return a + b; }
DCP_HD f64x2 add(f64x2 a, f64x2 b) { return a + b; }

// slab_sums: the same for N element indices at once, their loads interleaved (two sums that advance together).
template <int DEPTH, int N, class T>
__device__ __forceinline__ int slab_round(const T* __restrict__ slabs, long stride, int S, const long (&i)[N], int s,
                                          T (&acc)[N]) {   // adds slabs s, s + 1, ...; returns the next one
    for (; s + DEPTH - 1 < S; s += DEPTH) {
        T v[DEPTH][N];
#pragma unroll
        for (int u = 0; u < DEPTH; ++u)
#pragma unroll
            for (int q = 0; q < N; ++q) v[u][q] = slabs[(long)(s + u) * stride + i[q]];
#pragma unroll
        for (int u = 0; u < DEPTH; ++u)
#pragma unroll
            for (int q = 0; q < N; ++q) acc[q] = add(acc[q], v[u][q]);
    }
    return s;
}
template <int... DEPTHS, int N, class T>
__device__ __forceinline__ void slab_sums(const T* __restrict__ slabs, long stride, int S, const long (&i)[N],
                                          T (&acc)[N]) {
#pragma unroll
    for (int q = 0; q < N; ++q) acc[q] = slabs[i[q]];
    int s = 1;
    ((s = slab_round<DEPTHS>(slabs, stride, S, i, s, acc)), ...);
    slab_round<1>(slabs, stride, S, i, s, acc);
}
template <int... DEPTHS, class T>
__device__ __forceinline__ T slab_sum(const T* __restrict__ slabs, long stride, int S, long i) {
    const long at[1] = {i};
    T acc[1];
    slab_sums<DEPTHS...>(slabs, stride, S, at, acc);
    return acc[0];
}

// ---- a finished maximum, published ---------------------------------------------------------------
__device__ __forceinline__ void atomic_max_nonneg(float* p, float v) {
    atomicMax(reinterpret_cast<unsigned int*>(p), __float_as_uint(v));
}
__device__ __forceinline__ void atomic_max_nonneg(double* p, double v) {
    atomicMax(reinterpret_cast<unsigned long long*>(p), (unsigned long long)__double_as_longlong(v));
}
__device__ __forceinline__ float atomic_max_nonneg_ret(float* p, float v) {
    return __uint_as_float(atomicMax(reinterpret_cast<unsigned int*>(p), __float_as_uint(v)));
}
__device__ __forceinline__ double atomic_max_nonneg_ret(double* p, double v) {
    return __longlong_as_double((long long)atomicMax(reinterpret_cast<unsigned long long*>(p),
                                                     (unsigned long long)__double_as_longlong(v)));
}
// the value as the memory-side atomic unit holds it (a plain load may hit a line of this XCD's L2)
__device__ __forceinline__ float atomic_read_nonneg(float* p) {
    return __uint_as_float(atomicMax(reinterpret_cast<unsigned int*>(p), 0u));
}
__device__ __forceinline__ double atomic_read_nonneg(double* p) {
    return __longlong_as_double((long long)atomicMax(reinterpret_cast<unsigned long long*>(p), 0ull));
}

// Called by ONE thread of every workgroup of the grid with the workgroup's maximum m >= 0: the global maximum
// without a second launch.  |.| >= 0, so the IEEE bit pattern is monotone in the value and a NaN (0x7fc..) wins, as
// np.max would have it.  *gmax must be zero on entry.
// With a ticket the max is a RETURNING atomic and the ticket's increment is made to depend on the returned value: the
// max has been performed at the memory side before the arrival is counted, without a __threadfence (an L2 write-back
// on this part: ~2 us of a 12 us kernel).  The workgroup that arrives LAST (no waiting) publishes the finished maximum
// to *host_out -- device-mapped pinned host memory, where the host polls for it: no copy kernel and no event in
// between (4.2 us + a launch boundary + ~6 us of barrier packet per MU iteration).  The store needs no system fence --
// it is written through to the fabric, and the kernel's end releases it at the latest.  *ticket must be zero on entry;
// with reset_ticket it is again on exit (otherwise whoever clears *gmax clears it).
// Without a ticket: the plain atomic max, nothing published.
template <class R>
__device__ __forceinline__ void publish_max(R m, R* gmax, unsigned int* ticket, R* host_out, bool reset_ticket) {
    if (ticket == nullptr) {
        atomic_max_nonneg(gmax, m);
        return;
    }
    unsigned int inc = 1u;
    const R old = atomic_max_nonneg_ret(gmax, m);
    asm volatile("; the arrival is counted behind the max" : "+v"(inc) : "v"(old));
    if (atomicAdd(ticket, inc) == gridDim.x - 1u) {
        *host_out = atomic_read_nonneg(gmax);
        if (reset_ticket) atomicExch(ticket, 0u);
    }
}

}  // namespace dcp
