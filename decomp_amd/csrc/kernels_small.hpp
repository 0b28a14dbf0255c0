// Small HBM-bound kernels around the GEMM cores: split-K slab reduction, row
// normalisation (+ max|dD|), elementwise products / quotients, column sums,
// sign scans.  All are deterministic (no float atomics).
#pragma once
#include <hip/hip_runtime.h>
#include "epilogue.hpp"   // mu_quotient
#include "reduce.hpp"
#include "scalar.hpp"

namespace dcp {

inline int grid_for(long n, int cap = 2048) {
    long g = (n + 255) / 256;
    if (g < 1) g = 1;
    if (g > cap) g = cap;
    return (int)g;
}

// out[i] = sum_s slabs[s*stride + i], s in fixed order 0..S-1 (bitwise reproducible).
template <class T>
__global__ void __launch_bounds__(256) reduce_slabs_kernel(const T* __restrict__ slabs, long stride,
                                                           int S, long count, T* __restrict__ out) {
    for (long i = blockIdx.x * 256L + threadIdx.x; i < count; i += (long)gridDim.x * 256L)
        out[i] = slab_sum<16, 8>(slabs, stride, S, i);   // sixteen, then eight loads in flight
}
// on the scalar kernel, one workgroup per 256 elements up to `cap`
template <class T>
inline void launch_reduce_slabs_scalar(hipStream_t st, const T* slabs, long stride, int S, long count, T* out,
                                       int cap = 2048) {
    hipLaunchKernelGGL((reduce_slabs_kernel<T>), dim3(grid_for(count, cap)), dim3(256), 0, st, slabs, stride, S, count,
                       out);
}

// The same sum on 16-byte vectors (float x 4 / double x 2 per thread and slab): same order per element, so the same
// bits; a quarter of the threads and memory instructions on what is a latency-bound stream (the [K, F+K] statistics of
// an NMF iteration: 13 -> ~7 us).  count, stride multiples of VEC; slabs, out 16-byte aligned.
template <class T, int VEC>
__global__ void __launch_bounds__(256) reduce_slabs_vec_kernel(const T* __restrict__ slabs, long stride, int S,
                                                               long count, T* __restrict__ out) {
    typedef T vec_t __attribute__((ext_vector_type(VEC)));
    const long nvec = count / VEC, svec = stride / VEC;
    const vec_t* __restrict__ in = reinterpret_cast<const vec_t*>(slabs);
    vec_t* __restrict__ o = reinterpret_cast<vec_t*>(out);
    for (long i = blockIdx.x * 256L + threadIdx.x; i < nvec; i += (long)gridDim.x * 256L)
        o[i] = slab_sum<8, 2>(in, svec, S, i);
}

// Ordered slab sum, vectorised where the layout allows (real types).
template <class T>
inline void launch_reduce_slabs(hipStream_t st, const T* slabs, long stride, int S, long count, T* out) {
    if constexpr (std::is_same<T, float>::value || std::is_same<T, double>::value) {
        constexpr int VEC = 16 / sizeof(T);
        if (count % VEC == 0 && stride % VEC == 0 && (reinterpret_cast<uintptr_t>(slabs) & 15) == 0 &&
            (reinterpret_cast<uintptr_t>(out) & 15) == 0 && count >= 64 * 1024) {
            long g = (count / VEC + 255) / 256;
            if (g > 2048) g = 2048;
            hipLaunchKernelGGL((reduce_slabs_vec_kernel<T, VEC>), dim3((unsigned)g), dim3(256), 0, st, slabs, stride, S,
                               count, out);
            return;
        }
    }
    launch_reduce_slabs_scalar<T>(st, slabs, stride, S, count, out);
}

// reduce_slabs_kernel's sum (the same left-to-right order) with an affine term: out[i] = sum_s slabs[s][i] - sub,
// plus add_diag on the diagonal of a [diag_n, diag_n] matrix when diag_n > 0.  The HALS x sweep folds the L1/L2
// penalty on the codes into its operands with it: C = Y D^T - l1 (sub) and G = D D^T + l2 I (add_diag).
template <class T>
__global__ void __launch_bounds__(256) reduce_slabs_affine_kernel(const T* __restrict__ slabs, long stride, int S,
                                                                  long count, T sub, long diag_n, T add_diag,
                                                                  T* __restrict__ out) {
    for (long i = blockIdx.x * 256L + threadIdx.x; i < count; i += (long)gridDim.x * 256L) {
        T acc = slab_sum(slabs, stride, S, i);
        if (diag_n > 0 && i % (diag_n + 1) == 0) acc = acc + add_diag;
        out[i] = acc - sub;
    }
}

template <class T>
inline void launch_reduce_slabs_affine(hipStream_t st, const T* slabs, long stride, int S, long count, T sub,
                                       long diag_n, T add_diag, T* out) {
    hipLaunchKernelGGL((reduce_slabs_affine_kernel<T>), dim3(grid_for(count)), dim3(256), 0, st, slabs, stride, S, count,
                       sub, diag_n, add_diag, out);
}

// Same, for a [rows, cols] matrix written into a wider destination (leading dim ld_out).
template <class T>
__global__ void __launch_bounds__(256) reduce_slabs_rows_kernel(const T* __restrict__ slabs,
                                                                long stride, int S, long rows,
                                                                long cols, T* __restrict__ out,
                                                                long ld_out) {
    const long count = rows * cols;
    for (long i = blockIdx.x * 256L + threadIdx.x; i < count; i += (long)gridDim.x * 256L) {
        const long r = i / cols, c = i - r * cols;
        out[r * ld_out + c] = slab_sum(slabs, stride, S, i);
    }
}

// out[r, c] = v[r] for c in [0, cols)  (a per-row value broadcast along the row)
template <class T>
__global__ void __launch_bounds__(256) bcast_rows_kernel(const T* __restrict__ v, long rows,
                                                         long cols, T* __restrict__ out,
                                                         long ld_out) {
    const long count = rows * cols;
    for (long i = blockIdx.x * 256L + threadIdx.x; i < count; i += (long)gridDim.x * 256L) {
        const long r = i / cols, c = i - r * cols;
        out[r * ld_out + c] = v[r];
    }
}

// out[r, c] = v[c] for r in [0, rows)  (a per-column value repeated on every row)
template <class T>
__global__ void __launch_bounds__(256) bcast_cols_kernel(const T* __restrict__ v, long rows, long cols,
                                                         T* __restrict__ out) {
    const long count = rows * cols;
    for (long i = blockIdx.x * 256L + threadIdx.x; i < count; i += (long)gridDim.x * 256L)
        out[i] = v[i % cols];
}

// out = a o b (elementwise; b real "mask" of the same shape, or broadcast along rows when
// b_row_stride == 0).
template <class T>
__global__ void __launch_bounds__(256) mul_mask_kernel(const T* __restrict__ a,
                                                       const real_t<T>* __restrict__ m, long rows,
                                                       long cols, long m_row_stride,
                                                       T* __restrict__ out) {
    const long n = rows * cols;
    for (long i = blockIdx.x * 256L + threadIdx.x; i < n; i += (long)gridDim.x * 256L) {
        const long r = i / cols, c = i - r * cols;
        out[i] = scale(a[i], m[r * m_row_stride + c]);
    }
}

// Row-bit image of a mask (EpiMulMaskBits): word (g, c) holds (mask[32 g + b, c] != 0) in bit b.
// *not_binary is set when some entry is neither 0 nor 1 (the bit image then cannot stand in for the
// mask).  One thread per (row group, column): the 32 row reads of a wave are 256-byte coalesced rows.
template <class R>
__global__ void __launch_bounds__(256) mask_rowbits_kernel(const R* __restrict__ mask, long rows, long cols,
                                                           uint32_t* __restrict__ bits,
                                                           int* __restrict__ not_binary) {
    const long groups = (rows + 31) / 32;
    const long n = groups * cols;
    bool bad = false;
    for (long i = blockIdx.x * 256L + threadIdx.x; i < n; i += (long)gridDim.x * 256L) {
        const long g = i / cols, c = i - g * cols;
        uint32_t w = 0;
        // eight rows in flight per round: unconditional loads from a clamped row, selected afterwards
        // (a load under `if (r < rows)` is a branch and a full wait of its own)
        for (int b0 = 0; b0 < 32; b0 += 8) {
            R m[8];
#pragma unroll
            for (int u = 0; u < 8; ++u) {
                const long r = g * 32 + b0 + u;
                m[u] = mask[(r < rows ? r : rows - 1) * cols + c];
            }
#pragma unroll
            for (int u = 0; u < 8; ++u) {
                const bool in = (g * 32 + b0 + u) < rows;
                if (in && m[u] != R(0)) w |= (1u << (b0 + u));
                if (in && m[u] != R(0) && m[u] != R(1)) bad = true;
            }
        }
        bits[i] = w;
    }
    if (bad) atomicOr(not_binary, 1);
}

// out = cur * max(num, 0) / max(den, eps)   (grads.py:84,93), arbitrary leading dims.
// den_bcast: 0 = full [rows, cols]; 1 = one value per row (den[row]); 2 = one per column.
template <class T>
__global__ void __launch_bounds__(256) mu_quotient_kernel(const T* __restrict__ cur, long ld_cur,
                                                          const T* __restrict__ num, long ld_num,
                                                          const T* __restrict__ den, long ld_den,
                                                          int den_bcast, long rows, long cols,
                                                          T* __restrict__ out, long ld_out) {
    const long n = rows * cols;
    for (long i = blockIdx.x * 256L + threadIdx.x; i < n; i += (long)gridDim.x * 256L) {
        const long r = i / cols, c = i - r * cols;
        const T d = den_bcast == 0 ? den[r * ld_den + c] : (den_bcast == 1 ? den[r] : den[c]);
        const T nu = num[r * ld_num + c];
        out[r * ld_out + c] = mu_quotient(cur[r * ld_cur + c], nu, d);
    }
}

// out = cur * max(sum_s slabs[s], 0) / max(den, eps): the MU quotient for a split-K numerator.
// den: [rows, cols] (ld_den = cols) or one value per column (ld_den = 0).
// PEN: the L1/L2 penalty on the codes, the denominator is den + l1 + l2 cur (without it l1, l2 are not read).
template <class T, bool PEN>
__global__ void __launch_bounds__(256) mu_quotient_slabs_kernel(const T* __restrict__ cur,
                                                                const T* __restrict__ slabs,
                                                                long stride, int S,
                                                                const T* __restrict__ den, long ld_den,
                                                                long rows, long cols, T l1, T l2,
                                                                T* __restrict__ out) {
    const long n = rows * cols;
    for (long i = blockIdx.x * 256L + threadIdx.x; i < n; i += (long)gridDim.x * 256L) {
        const T nu = slab_sum(slabs, stride, S, i);
        const long r = i / cols, c = i - r * cols;
        const T d = den[r * ld_den + c];
        const T x = cur[i];
        out[i] = mu_quotient_if<PEN>(x, nu, d, l1, l2);
    }
}

// The MU quotient for the STACKED split-K product [den ; num] (rows [0, count) of every slab hold the
// negative part, rows [count, 2 count) the positive part): out = cur * max(sum num, 0) / max(sum den, eps),
// both sums advancing together.  PEN as above.
template <class T, bool PEN>
__global__ void __launch_bounds__(256) mu_quotient_stacked_kernel(const T* __restrict__ cur,
                                                                  const T* __restrict__ slabs, long stride,
                                                                  int S, long count, T l1, T l2,
                                                                  T* __restrict__ out) {
    for (long i = blockIdx.x * 256L + threadIdx.x; i < count; i += (long)gridDim.x * 256L) {
        const long at[2] = {i, count + i};
        T sum[2];
        slab_sums(slabs, stride, S, at, sum);
        const T x = cur[i];
        out[i] = mu_quotient_if<PEN>(x, sum[1], sum[0], l1, l2);
    }
}

// One workgroup per row of U[K, F]:  out = U / sqrt(sum |U|^2)  (strict) or
// U / sqrt(max(sum |U|^2, 1)).  Optionally block-max of |ref - out| into rowmax[row].
template <class T>
__global__ void __launch_bounds__(256) row_normalize_kernel(const T* __restrict__ U, long ld_u,
                                                            long F, int strict,
                                                            const T* __restrict__ ref, long ld_ref,
                                                            T* __restrict__ out, long ld_out,
                                                            real_t<T>* __restrict__ rowmax,
                                                            real_t<T>* __restrict__ norm_out = nullptr,
                                                            real_t<T>* __restrict__ gmax = nullptr,
                                                            real_t<T>* __restrict__ gmax_zero = nullptr,
                                                            unsigned int* __restrict__ ticket = nullptr,
                                                            real_t<T>* __restrict__ host_out = nullptr) {
    typedef real_t<T> R;
    __shared__ R sh[4];
    __shared__ R s_inv;
    const long row = blockIdx.x;
    const T* u = U + row * ld_u;
    // rows of up to 4096 elements stay in registers between the two passes (one HBM/L2 round
    // trip instead of two: this kernel sits on the replicated, latency-bound tail of a step)
    constexpr int CACHE = 16;
    const bool cached = F <= 256L * CACHE;
    T rc[CACHE];
    R acc = 0;
    if (cached) {
#pragma unroll
        for (int q = 0; q < CACHE; ++q) {
            const long j = threadIdx.x + 256L * q;
            rc[q] = (j < F) ? u[j] : zero_of<T>();
            acc += abs2(rc[q]);
        }
    } else {
        for (long j = threadIdx.x; j < F; j += 256) acc += abs2(u[j]);
    }
    R tot = block_sum_256(acc, sh);
    if (threadIdx.x == 0) {
        if (!strict) tot = tot > R(1) ? tot : R(1);
        s_inv = sqrt(tot);
        if (norm_out != nullptr) norm_out[row] = s_inv;
    }
    __syncthreads();
    const R nrm = s_inv;
    R md = 0;
    auto emit = [&](long j, T v) {
        T o;  // a true division, as the reference's U / sqrt(.)
        if constexpr (scalar_traits<T>::is_complex) {
            o.re = v.re / nrm;
            o.im = v.im / nrm;
        } else {
            o = v / nrm;
        }
        if (ref != nullptr) {
            const R d = absval(sub(ref[row * ld_ref + j], o));
            md = max_np(d, md);
        }
        out[row * ld_out + j] = o;
    };
    if (cached) {
#pragma unroll
        for (int q = 0; q < CACHE; ++q) {
            const long j = threadIdx.x + 256L * q;
            if (j < F) emit(j, rc[q]);
        }
    } else {
        for (long j = threadIdx.x; j < F; j += 256) emit(j, u[j]);
    }
    if (rowmax != nullptr || gmax != nullptr) {
        R m = block_max_256(md, sh);
        if (threadIdx.x == 0) {
            if (rowmax != nullptr) rowmax[row] = m;
            // the global maximum (publish_max); the other ping-pong slot is cleared for the next iteration
            if (gmax_zero != nullptr && row == 0) *gmax_zero = R(0);
            if (gmax != nullptr) publish_max(m, gmax, ticket, host_out, true);
        }
    }
}

// Column sums of a[rows, cols] over rows: stage 1 partial[b, c] over a row stripe,
// stage 2 = reduce_slabs_kernel.  (KL denominators: grads.py:146,155.)
template <class T>
__global__ void __launch_bounds__(256) colsum_partial_kernel(const T* __restrict__ a, long ld,
                                                             long rows, long cols, long rows_per_blk,
                                                             T* __restrict__ partial) {
    const long r0 = blockIdx.y * rows_per_blk;
    const long r1 = min(rows, r0 + rows_per_blk);
    for (long c = blockIdx.x * 256L + threadIdx.x; c < cols; c += (long)gridDim.x * 256L) {
        // four independent running sums: the loop is load-latency bound with one
        T a0 = zero_of<T>(), a1 = zero_of<T>(), a2 = zero_of<T>(), a3 = zero_of<T>();
        long r = r0;
        for (; r + 3 < r1; r += 4) {
            a0 = add(a0, a[r * ld + c]);
            a1 = add(a1, a[(r + 1) * ld + c]);
            a2 = add(a2, a[(r + 2) * ld + c]);
            a3 = add(a3, a[(r + 3) * ld + c]);
        }
        for (; r < r1; ++r) a0 = add(a0, a[r * ld + c]);
        partial[blockIdx.y * cols + c] = add(add(a0, a1), add(a2, a3));
    }
}

// Row sums of a[rows, cols]: one block per row.
template <class T>
__global__ void __launch_bounds__(256) rowsum_kernel(const T* __restrict__ a, long ld, long cols,
                                                     T* __restrict__ out) {
    __shared__ T sh[4];
    const long row = blockIdx.x;
    T acc = 0;
    for (long j = threadIdx.x; j < cols; j += 256) acc += a[row * ld + j];
    T t = block_sum_256(acc, sh);
    if (threadIdx.x == 0) out[row] = t;
}

}  // namespace dcp
