// Masked approximate K-SVD: the dictionary update of ksvd.hpp for data with holes, the trainer that goes with the
// masked coder of omp_mask.hpp,
//
//   min sum_if M_if |Y_if - (X D)_if|^2  s.t.  |x_i|_0 <= s, |d_k| = 1     Y [N, F], X [N, K], D [K, F], M [N, F] >= 0
//
// The weights enter linearly (m, not m^2: the convention of omp_mask.hpp); a 1-D mask [F] is the 2-D one with every
// row equal.  One iteration: X = masked omp(Y, D, s; M) (unchanged); R = Y - X D once, on the GEMM cores, hidden
// entries included -- they never enter a sum except multiplied by M, so Y must be finite there and its values there do
// not influence the result; then one weighted rank-1 alternating step per atom, for k = 0 .. K-1 in order, with
// I = {i : X[i, k] != 0} ascending and fixed for the sweep (the lists of ksvd.hpp):
//   I empty: atom k is left as it is
//   g = X[I, k], d = D[k], m_i = M[i, :]:
//     c_f  = sum_{i in I} m_if |g_i|^2
//     n_f  = sum_{i in I} m_if conj(g_i) R_if + c_f d_f
//     u_f  = n_f / c_f where c_f > 0, else d_f        (a column hidden in every support row keeps its value)
//     d'   = u / |u|, or d where !(|u| > 0)            (a NaN keeps d)
//     q_i  = sum_f m_if |d'_f|^2
//     g'_i = (sum_f m_if R_if conj(d'_f) + g_i sum_f m_if d_f conj(d'_f)) / q_i where q_i > 0, else 0
//     R[I, :] += g d - g' d';  X[I, k] = g';  D[k] = d'
// Monotone: with E = R[I, :] + g d (never formed), u minimises sum m |E - g u|^2 over u for the fixed g (column by
// column a weighted least-squares problem in one unknown); the objective does not change under
// (g, u) -> (g |u|, u / |u|); and g' minimises it over g for d' (row by row, one unknown).  So no atom step increases
// the weighted objective, and R = Y - X D holds throughout.  With M = 1: c_f = |g|^2, u is ksvd.hpp's u divided by
// |g|^2, q_i = 1: the sweep of ksvd.hpp up to the rounding of that division.
//
// Kernels: the decomposition, the fixed summation orders and the constraints of ksvd.hpp (stream order between atoms,
// no float atomics, nothing waits on another workgroup, plain C++ stores; bitwise reproducible).  The lists, the
// residual product and max|D_new - D_old| are ksvd.hpp's own.  A 1-D mask runs the same kernels with a mask row
// stride of 0, so it and its 2-D broadcast give the same bits.
//   pass 1  as ksvd_pass1_kernel, with two partials per column: part[chunk, :] = sum m conj(g) R (T) and
//           cpart[chunk, :] = sum m |g|^2 (real); each wave a quarter of the chunk in list order, ((w0 + w1) + w2) + w3
//   finish  per column n, c (the partials in chunk order) and u into ubuf, and the tile's share of |u|^2.  The
//           d . u^H and |d|^2 shares of ksvd_finish_kernel have no counterpart: those products are weighted per row.
//   pass 2  one wave per support row: it reads the row of R and the row of M once and forms the three weighted sums
//           in that one pass (per lane in increasing f, then the butterfly), keeps the row of R in its LDS slice,
//           applies the update and writes the row once.  M is not needed after the sums, so it is not kept.  Rows too
//           long for the slice are read a second time, as in ksvd_pass2_kernel.
// An access of V elements of T goes with V reals of the mask (16 bytes for float32 and float64, 8 for complex64); the
// 16-byte path on R and D is taken only where the mask rows are aligned for that share.
// Each atom makes two reads and one write of its support rows of R and two reads of the same rows of M:
// sum_k |I_k| F (3 sizeof(T) + 2 sizeof(real)) bytes per sweep.
//
// This file holds the three kernels only and is included by ksvd.hpp, between its own kernels (whose KsvdPack,
// ksvd_div, ksvd_new_atom and ksvd_lane_sum these use) and the one host path that launches either set: include
// ksvd.hpp, not this file.
#pragma once

namespace dcp {

// the V reals of the mask that go with a KsvdPack<T, V>
template <class R, int V>
struct alignas(V * sizeof(R) >= 16 ? 16 : V * sizeof(R)) KsvdMaskPack {
    R v[V];
};

// ---- pass 1: part[chunk, :] = sum m_i conj(g_i) R[i, :], cpart[chunk, :] = sum m_i |g_i|^2 over the chunk's rows ---
// The grid, the column tiles and the order of ksvd_pass1_kernel.  ms: the mask's row stride in elements (F, or 0
// for a 1-D mask).
template <class T, int V>
__global__ void __launch_bounds__(256) ksvd_mask_pass1_kernel(const T* __restrict__ Rm,
                                                              const real_t<T>* __restrict__ M, long ms,
                                                              const T* __restrict__ X, const int* __restrict__ rows,
                                                              const long long* __restrict__ off, int k, int K, long F,
                                                              int ntiles, T* __restrict__ part,
                                                              real_t<T>* __restrict__ cpart) {
    typedef real_t<T> R;
    typedef KsvdPack<T, V> P;
    typedef KsvdMaskPack<R, V> MP;
    constexpr int kQuarter = kKsvdChunk / 4;
    __shared__ int s_row[kKsvdChunk];
    __shared__ T s_gc[kKsvdChunk];
    __shared__ R s_g2[kKsvdChunk];
    __shared__ T s_acc[3][64 * V];
    __shared__ R s_cacc[3][64 * V];
    const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
    const int chunk = blockIdx.x / ntiles, tile = blockIdx.x - chunk * ntiles;
    const long long base = off[k] + (long long)chunk * kKsvdChunk;
    const long long left = off[k + 1] - base;
    const int n = (int)(left < kKsvdChunk ? left : kKsvdChunk);
    for (int e = tid; e < n; e += 256) {
        const int i = rows[base + e];
        const T g = X[(long)i * K + k];
        s_row[e] = i;
        s_gc[e] = conj_of(g);
        s_g2[e] = abs2(g);
    }
    __syncthreads();
    const long j = ((long)tile * 64 + lane) * V;
    const bool live = j < F;
    T acc[V];
    R cacc[V];
#pragma unroll
    for (int q = 0; q < V; ++q) {
        acc[q] = zero_of<T>();
        cacc[q] = R(0);
    }
    if (live) {
        const int e0 = wave * kQuarter;
        const int e1 = e0 + kQuarter < n ? e0 + kQuarter : n;
#pragma unroll 4
        for (int e = e0; e < e1; ++e) {
            const long i = s_row[e];
            const P r = *reinterpret_cast<const P*>(Rm + i * F + j);
            const MP m = *reinterpret_cast<const MP*>(M + i * ms + j);
            const T gc = s_gc[e];
            const R g2 = s_g2[e];
#pragma unroll
            for (int q = 0; q < V; ++q) {
                acc[q] = fmadd(acc[q], scale(gc, m.v[q]), r.v[q]);
                cacc[q] = fmadd(cacc[q], m.v[q], g2);
            }
        }
    }
    if (wave > 0) {
#pragma unroll
        for (int q = 0; q < V; ++q) {
            s_acc[wave - 1][lane * V + q] = acc[q];
            s_cacc[wave - 1][lane * V + q] = cacc[q];
        }
    }
    __syncthreads();
    if (wave == 0 && live) {
        P o;
        MP c;
#pragma unroll
        for (int q = 0; q < V; ++q) {
            o.v[q] = add(add(add(acc[q], s_acc[0][lane * V + q]), s_acc[1][lane * V + q]), s_acc[2][lane * V + q]);
            c.v[q] = ((cacc[q] + s_cacc[0][lane * V + q]) + s_cacc[1][lane * V + q]) + s_cacc[2][lane * V + q];
        }
        *reinterpret_cast<P*>(part + (long)chunk * F + j) = o;
        *reinterpret_cast<MP*>(cpart + (long)chunk * F + j) = c;
    }
}

// ---- finish: n = the partials in chunk order + c d, u = n / c (d where !(c > 0)) -> ubuf, and this tile's share of
// |u|^2.  grid: ceil(F / 256) workgroups of 256, a thread owns one column. -------------------------------------------
template <class T>
__global__ void __launch_bounds__(256) ksvd_mask_finish_kernel(const T* __restrict__ part,
                                                               const real_t<T>* __restrict__ cpart, int nchunks, int k,
                                                               long F, const T* __restrict__ Dold, T* __restrict__ ubuf,
                                                               real_t<T>* __restrict__ usq) {
    typedef real_t<T> R;
    __shared__ R sh[4];
    const int tid = threadIdx.x;
    const long j = blockIdx.x * 256L + tid;
    R uu = 0;
    if (j < F) {
        T nf = part[j];
        R cf = cpart[j];
#pragma unroll 4
        for (int c = 1; c < nchunks; ++c) {
            nf = add(nf, part[(long)c * F + j]);
            cf += cpart[(long)c * F + j];
        }
        const T dj = Dold[(long)k * F + j];
        nf = add(nf, scale(dj, cf));
        const T u = cf > R(0) ? ksvd_div(nf, cf) : dj;
        ubuf[j] = u;
        uu = abs2(u);
    }
    uu = block_sum_256(uu, sh);
    if (tid == 0) usq[blockIdx.x] = uu;
}

// ---- pass 2: d' = u / |u| (d where !(|u| > 0));  q = sum m |d'|^2;  g' = (sum m R[i, :] conj(d') + g sum m d conj(d'))
// / q (0 where !(q > 0));  R[i, :] += g d - g' d';  X[i, k] = g';  D[k] = d'.  One wave per support row. -------------
// The grid, the LDS slices and the writes of D[k] of ksvd_pass2_kernel.
template <class T, int V>
__global__ void __launch_bounds__(256) ksvd_mask_pass2_kernel(T* __restrict__ Rm, const real_t<T>* __restrict__ M,
                                                              long ms, T* __restrict__ X, const int* __restrict__ rows,
                                                              const long long* __restrict__ off, int k, int K, long F,
                                                              const T* __restrict__ Dold, T* __restrict__ D,
                                                              const T* __restrict__ ubuf,
                                                              const real_t<T>* __restrict__ usq, int nparts,
                                                              int use_lds) {
    typedef real_t<T> R;
    typedef KsvdPack<T, V> P;
    typedef KsvdMaskPack<R, V> MP;
    extern __shared__ __attribute__((aligned(16))) unsigned char ksvd_lds[];
    const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
    const long long e = (long long)blockIdx.x * (blockDim.x >> 6) + wave;
    const long long b = off[k];
    const long long cnt = off[k + 1] - b;
    if (e >= cnt) return;
    const long i = rows[b + e];
    T* r = Rm + i * F;
    const R* m = M + i * ms;
    const T* d = Dold + (long)k * F;
    T* slice = reinterpret_cast<T*>(ksvd_lds) + (use_lds ? (long)wave * F : 0);
    const T g = X[i * K + k];
    const R nrm = sqrt(ksvd_lane_sum(usq, nparts, lane));
    const bool keep_d = !(nrm > R(0));
    T sr = zero_of<T>(), sd = zero_of<T>();
    R sq = 0;
#pragma unroll 4
    for (long j = (long)lane * V; j < F; j += 64 * V) {
        const P rv = *reinterpret_cast<const P*>(r + j);
        const MP mv = *reinterpret_cast<const MP*>(m + j);
        const P uv = *reinterpret_cast<const P*>(ubuf + j);
        const P ov = *reinterpret_cast<const P*>(d + j);
#pragma unroll
        for (int q = 0; q < V; ++q) {
            const T dn = ksvd_new_atom(keep_d, ov, uv, q, nrm);
            const T dc = conj_of(dn);
            sr = fmadd(sr, scale(rv.v[q], mv.v[q]), dc);
            sd = fmadd(sd, scale(ov.v[q], mv.v[q]), dc);
            sq = fmadd(sq, mv.v[q], abs2(dn));
        }
        if (use_lds) *reinterpret_cast<P*>(slice + j) = rv;
    }
    sr = wave_sum_all(sr);
    sd = wave_sum_all(sd);
    sq = wave_sum_all(sq);
    const T gn = sq > R(0) ? ksvd_div(fmadd(sr, g, sd), sq) : zero_of<T>();
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
