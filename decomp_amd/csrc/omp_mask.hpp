// Masked orthogonal matching pursuit: every row y [F] of Y [N, F] has non-negative weights m [F] of its own,
//
//   min_x  sum_f m_f |y_f - (x A)_f|^2   s.t.  |x|_0 <= s        (and / or until that weighted residual <= tol)
//
// i.e. the algorithm of omp.hpp with every inner product weighted, <u, v>_m = sum_f m_f u_f conj(v_f).  The weights
// enter linearly (m, not m^2).  A row with its own weights has its own Gram matrix, so the Gram form of omp.hpp
// (one G = A A^H for all rows) does not apply; this is the RESIDUAL form.  Per row, support I = (), x = 0, r = y:
//   1. tol given and sum m |r|^2 <= tol: stop
//   2. alpha_k = <r, a_k>_m, c_k = |alpha_k| / n_k over k not in I with n_k > 0, n_k^2 = sum_f m_f |a_kf|^2;
//      k* = the LOWEST index attaining the maximum; maximum <= 0 (or NaN): stop
//   3. g_j = <a_Ij, a_k*>_m, g** = <a_k*, a_k*>_m; L w = g, d = g** - |w|^2; d <= eps_dep g**: stop, keeping x
//   4. I <- I + (k*); L gains the row (w^H, sqrt(d)); z gains conj(alpha_k*) / sqrt(d) (r is orthogonal to the
//      support, so alpha_k* is what alpha0_k* - x_I G[I, k*] is in omp.hpp); L^H v = z, x_I = conj(v)
//   5. r = y - sum_j x_j a_Ij, rebuilt from y (never updated incrementally), sum m |r|^2
// A row whose weights are all zero has alpha = 0 and takes no step; an atom whose observed part vanishes in a row
// has n_k = 0 there and is never selected in that row.
//
// mask_ndim == 1 (one [F] mask for all rows) is one shared Gram matrix again: Y and A are scaled by sqrt(m) into
// workspace and omp_solve runs on them; its coefficients are already those for the caller's A.
//
// mask_ndim == 2, in passes of Nc rows.  Once per pass: W [Nc, K] = M (|A|^2)^T (the n_k^2 of every row, a real NT
// product on the GEMM cores; |A|^2 is formed once per call), Rm = m o y, r2 = sum m |y|^2.  Then s steps, enqueued
// without a host round trip:
//   a. alpha [Nc, K] = Rm A^H on the GEMM cores (step 2's correlations: 2 Nc K F flops, where the flops are)
//   b. omp_mask_step_kernel: 64-thread workgroups, a wave owns a row.  It loads the row's state from the workspace
//      (a finished row leaves by a wave-uniform branch), scores alpha / sqrt(W) as omp.hpp does (greedy_lane_best,
//      greedy_wave_best), forms the n + 1 weighted dot products of step 3 from the atom rows and the row of M (lanes
//      stride f: contiguous loads; A stays in L2; four atoms share one pass over m o conj(a_k*)), runs the
//      substitutions of greedy.hpp's OmpFactor on the factor (copied to LDS), appends the factor's new row to the
//      workspace, rebuilds r from y and writes m o r and sum m |r|^2.
// After the last step omp_mask_finish_kernel writes the rows of X (zeros off the support) and the step count.
// Every sum has a fixed order (per lane in increasing f, then the xor butterfly); the only atomic is one integer
// max per row for the step count.  Bitwise reproducible.
//
// Workspace per row: the packed factor s (s + 1) / 2, z [s], x_I [s] (T), sel [s] (int), (n, done) and r2, next to
// the pass's alpha [K], W [K] and Rm [F].  At s = 64, float32 and 65536 rows the factor alone is 545 MB, so Nc is
// chosen from a byte budget, kOmpMaskBudget = 1 GiB of per-row workspace: the fewest passes that fit it, of equal
// size, rounded up to 64 rows.
// Limits: those of omp.hpp (s <= 64 real, s <= 32 complex; any K >= 1).
#pragma once
#include <hip/hip_runtime.h>

#include "omp.hpp"

namespace dcp {

constexpr size_t kOmpMaskBudget = size_t(1) << 30;   // bytes of per-row workspace of one pass
constexpr int kOmpMaskDone = 0x100;                  // stat = n | (done ? kOmpMaskDone : 0)

__host__ __device__ inline long omp_mask_tri(int n) { return (long)n * (n + 1) / 2; }

template <class T>
struct OmpMaskWs {
    typedef real_t<T> R;
    R* A2 = nullptr;       // [K, F] |A|^2
    R* W = nullptr;        // [Nc, K] n_k^2 of every row
    T* Rm = nullptr;       // [Nc, F] m o r
    T* alpha = nullptr;    // [Nc, K] <r, a_k>_m
    T* L = nullptr;        // [Nc, s (s + 1) / 2] the packed factor, row j at j (j + 1) / 2
    T* z = nullptr;        // [Nc, s]
    T* x = nullptr;        // [Nc, s] x_I
    int* sel = nullptr;    // [Nc, s] I
    int* stat = nullptr;   // [Nc] n | done
    R* r2 = nullptr;       // [Nc] sum m |r|^2
    int* it = nullptr;     // the step count
    R* ext1 = nullptr;     // complex: the real extended image of A
};

template <class T>
inline size_t omp_mask_row_bytes(int64_t F, int64_t K, int s) {
    typedef real_t<T> R;
    return (size_t)(omp_mask_tri(s) + 2 * s + K + F) * sizeof(T) + (size_t)(K + 1) * sizeof(R) +
           (size_t)(s + 1) * sizeof(int);
}

// rows per pass: the caller's, or the fewest equal passes within the budget (multiples of 64 rows)
template <class T>
inline int64_t omp_mask_rows_per_pass(int64_t N, int64_t F, int64_t K, int s, int rows_per_pass) {
    if (rows_per_pass > 0) return rows_per_pass < N ? rows_per_pass : N;
    int64_t fit = (int64_t)(kOmpMaskBudget / omp_mask_row_bytes<T>(F, K, s));
    if (fit < 64) fit = 64;
    if (fit >= N) return N;
    const int64_t passes = (N + fit - 1) / fit;
    int64_t nc = (N + passes - 1) / passes;
    nc = (nc + 63) / 64 * 64;
    return nc < N ? nc : N;
}

template <class T>
inline void omp_mask_layout(WsLayout& a, OmpMaskWs<T>& w, int64_t Nc, int64_t F, int64_t K, int s) {
    a.take(w.A2, (size_t)K * F);
    a.take(w.W, (size_t)Nc * K);
    a.take(w.Rm, (size_t)Nc * F);
    a.take(w.alpha, (size_t)Nc * K);
    a.take(w.L, (size_t)Nc * omp_mask_tri(s));
    a.take(w.z, (size_t)Nc * s);
    a.take(w.x, (size_t)Nc * s);
    a.take(w.sel, (size_t)Nc * s);
    a.take(w.stat, (size_t)Nc);
    a.take(w.r2, (size_t)Nc);
    a.take(w.it, 4);
    if (scalar_traits<T>::is_complex) a.take(w.ext1, (size_t)4 * K * F);
}

// out = |a|^2 elementwise; clears *it_zero
template <class T>
__global__ void __launch_bounds__(256) omp_mask_abs2_kernel(const T* __restrict__ a, long n, real_t<T>* __restrict__ out,
                                                            int* __restrict__ it_zero) {
    if (blockIdx.x == 0 && threadIdx.x == 0) *it_zero = 0;
    for (long i = blockIdx.x * 256L + threadIdx.x; i < n; i += (long)gridDim.x * 256L) out[i] = abs2(a[i]);
}

// out[r, c] = a[r, c] sqrt(m[c])  (the 1-D mask folded into Y and A)
template <class T>
__global__ void __launch_bounds__(256) omp_mask_sqrt_scale_kernel(const T* __restrict__ a, const real_t<T>* __restrict__ m,
                                                                  long rows, long cols, T* __restrict__ out) {
    const long n = rows * cols;
    for (long i = blockIdx.x * 256L + threadIdx.x; i < n; i += (long)gridDim.x * 256L)
        out[i] = scale(a[i], sqrt(m[i % cols]));
}

// The start of a pass, one 64-thread workgroup per row: Rm = m o y, r2 = sum m |y|^2, n = 0.
template <class T>
__global__ void __launch_bounds__(64) omp_mask_init_kernel(const T* __restrict__ Y, const real_t<T>* __restrict__ M,
                                                           long F, T* __restrict__ Rm, real_t<T>* __restrict__ r2,
                                                           int* __restrict__ stat) {
    typedef real_t<T> R;
    const long row = blockIdx.x;
    const T* y = Y + row * F;
    const R* m = M + row * F;
    T* rm = Rm + row * F;
    R acc = R(0);
    for (long f = threadIdx.x; f < F; f += 64) {
        const T v = y[f];
        const R mf = m[f];
        rm[f] = scale(v, mf);
        acc += mf * abs2(v);
    }
    const R tot = wave_sum_all(acc);
    if (threadIdx.x == 0) {
        r2[row] = tot;
        stat[row] = 0;
    }
}

// One greedy step of every unfinished row of a pass (steps 1 .. 5 of the header; alpha holds this step's product).
// grid: Nc workgroups of 64 threads; dynamic LDS OmpCarve<T>(s).bytes.  tol < 0: no residual stop.
template <class T>
__global__ void __launch_bounds__(64) omp_mask_step_kernel(const T* __restrict__ Y, const real_t<T>* __restrict__ M,
                                                           const T* __restrict__ A, const T* __restrict__ alpha,
                                                           const real_t<T>* __restrict__ W, T* __restrict__ Rm,
                                                           T* __restrict__ Lg, T* __restrict__ zg, T* __restrict__ xg,
                                                           int* __restrict__ selg, int* __restrict__ stat,
                                                           real_t<T>* __restrict__ r2g, int F, int K, int s,
                                                           real_t<T> tol) {
    typedef real_t<T> R;
    extern __shared__ __attribute__((aligned(16))) unsigned char omp_mask_lds[];
    const int lane = threadIdx.x;
    const long row = blockIdx.x;
    const OmpCarve<T> cv(s);
    const int ld = omp_ld(s);
    T* L = reinterpret_cast<T*>(omp_mask_lds);
    T* xs = reinterpret_cast<T*>(omp_mask_lds + cv.xs);
    int* sel = reinterpret_cast<int*>(omp_mask_lds + cv.sel);

    const int st = __builtin_amdgcn_readfirstlane(stat[row]);
    int n = st & (kOmpMaskDone - 1);
    if ((st & kOmpMaskDone) || n >= s) return;   // finished: wave-uniform
    if (tol >= R(0)) {
        const R r2 = r2g[row];
        if (__builtin_amdgcn_readfirstlane((int)!(r2 > tol))) {   // sum m |r|^2 <= tol (or NaN)
            if (lane == 0) stat[row] = n | kOmpMaskDone;
            return;
        }
    }
    const int lc = lane < s ? lane : s - 1;   // this lane's row / column of L, clamped into the image
    const T* yrow = Y + row * F;
    const R* mrow = M + row * F;
    const T* arow = alpha + row * K;
    const R* wrow = W + row * K;
    T* lrow_g = Lg + row * omp_mask_tri(s);

    // ---- the row's state: sel, z (lane j < n), the factor into LDS ----
    int my_sel = selg[row * s + lc];
    T z = omp_keep(zg[row * s + lc], lane < n);
    if (lane < n) sel[lane] = my_sel;
    for (int j = 0; j < n; ++j)
        if (lane <= j) L[j * ld + lane] = lrow_g[omp_mask_tri(j) + lane];
    __syncthreads();
    R dinv = omp_keep(R(1) / real_part(L[lc * ld + lc]), lane < n);   // lane j < n: 1 / L_jj

    // ---- selection: alpha / sqrt(W) over the atoms outside the support ----
    R bc = R(-1);
    int bk = 0x7fffffff;
    for (int kb = 0; kb < K; kb += 64 * kOmpChunk) {
        T a[kOmpChunk];
        R wv[kOmpChunk];
        int kq[kOmpChunk];
        bool hit[kOmpChunk];
#pragma unroll
        for (int q = 0; q < kOmpChunk; ++q) {
            kq[q] = kb + 64 * q + lane;
            const int kk = kq[q] < K ? kq[q] : K - 1;
            a[q] = arow[kk];
            wv[q] = wrow[kk];
            hit[q] = false;
        }
        for (int j = 0; j < n; ++j) {
            const int ij = sel[j];   // LDS, one address for the wave: a broadcast
#pragma unroll
            for (int q = 0; q < kOmpChunk; ++q) hit[q] = hit[q] || ij == kq[q];
        }
#pragma unroll
        for (int q = 0; q < kOmpChunk; ++q) {
            const R inv = wv[q] > R(0) ? R(1) / sqrt(wv[q]) : R(0);
            greedy_lane_best(bc, bk, omp_mag(a[q]) * inv, !hit[q] && kq[q] < K && inv > R(0), kq[q]);
        }
    }
    greedy_wave_best(bc, bk);
    if (__builtin_amdgcn_readfirstlane((int)!(bc > R(0)))) {   // nothing correlates
        if (lane == 0) stat[row] = n | kOmpMaskDone;
        return;
    }
    const int kstar = __builtin_amdgcn_readfirstlane(bk);
    const T* ak = A + (long)kstar * F;
    const T alk = arow[kstar];

    // ---- the weighted dot products: lane j < n gets g_j = <a_Ij, a_k*>_m, gkk = <a_k*, a_k*>_m ----
    T b = zero_of<T>();
    R gkk = R(0);
    for (int j0 = 0; j0 <= n; j0 += 4) {
        const T* ap[4];
        T acc[4];
#pragma unroll
        for (int u = 0; u < 4; ++u) {
            const int ju = j0 + u < n ? j0 + u : n;
            const int idx = ju < n ? sel[ju] : kstar;
            ap[u] = A + (long)idx * F;
            acc[u] = zero_of<T>();
        }
#pragma unroll 2
        for (int f = lane; f < F; f += 64) {
            const T mk = scale(conj_of(ak[f]), mrow[f]);
#pragma unroll
            for (int u = 0; u < 4; ++u) acc[u] = fmadd(acc[u], ap[u][f], mk);
        }
#pragma unroll
        for (int u = 0; u < 4; ++u) {
            const T tot = wave_sum_all(acc[u]);
            if (j0 + u < n && lane == j0 + u) b = tot;
            if (j0 + u == n) gkk = real_part(tot);
        }
    }

    // ---- the Cholesky pivot: L w = g ----
    const OmpFactor<T> fac{L, ld, lane, lc, n};
    R wn2;
    const T w = fac.forward(b, dinv, wn2);
    const R d = gkk - wn2;
    if (__builtin_amdgcn_readfirstlane((int)fac.dependent(d, gkk))) {   // keep the previous x
        if (lane == 0) stat[row] = n | kOmpMaskDone;
        return;
    }
    // ---- accept: row n of L, z_n, then L^H v = z ----
    const R ldiag = sqrt(d), rdiag = R(1) / ldiag;
    const T wc = omp_keep(conj_of(w), lane < n);
    {
        const T zn = scale(conj_of(alk), rdiag);
        fac.accept(wc, ldiag);
        if (lane < n) lrow_g[omp_mask_tri(n) + lane] = wc;
        if (lane == n) {
            lrow_g[omp_mask_tri(n) + n] = from_real<T>(ldiag);
            sel[n] = kstar;
            selg[row * s + n] = kstar;
            zg[row * s + n] = zn;
            dinv = rdiag;
            z = zn;
        }
    }
    __syncthreads();
    const T x = conj_of(fac.backward(z, dinv, wc));
    if (lane <= n) {
        xs[lane] = x;
        xg[row * s + lane] = x;
    }
    ++n;
    __syncthreads();

    // ---- the residual, rebuilt from y: r = y - sum_j x_j a_Ij; Rm = m o r, r2 = sum m |r|^2 ----
    T* rmrow = Rm + row * F;
    R acc2 = R(0);
    for (int f0 = 0; f0 < F; f0 += 256) {
        T r[4];
        int fc[4];
#pragma unroll
        for (int q = 0; q < 4; ++q) {
            const int f = f0 + 64 * q + lane;
            fc[q] = f < F ? f : F - 1;
            r[q] = yrow[fc[q]];
        }
        for (int j = 0; j < n; ++j) {
            const T xj = xs[j];
            const T* aj = A + (long)sel[j] * F;
#pragma unroll
            for (int q = 0; q < 4; ++q) r[q] = fmsub(r[q], xj, aj[fc[q]]);
        }
#pragma unroll
        for (int q = 0; q < 4; ++q) {
            const int f = f0 + 64 * q + lane;
            const R mf = mrow[fc[q]];
            if (f < F) {
                rmrow[f] = scale(r[q], mf);
                acc2 += mf * abs2(r[q]);
            }
        }
    }
    const R r2 = wave_sum_all(acc2);
    if (lane == 0) {
        r2g[row] = r2;
        stat[row] = n;
    }
}

// The rows of X of a pass, zeros off the support, and the largest support size into *it_max.
template <class T>
__global__ void __launch_bounds__(64) omp_mask_finish_kernel(const T* __restrict__ xg, const int* __restrict__ selg,
                                                             const int* __restrict__ stat, T* __restrict__ X, int K,
                                                             int s, int* __restrict__ it_max) {
    const int lane = threadIdx.x;
    const long row = blockIdx.x;
    const int n = __builtin_amdgcn_readfirstlane(stat[row]) & (kOmpMaskDone - 1);
    omp_scatter_row(selg + row * s, xg + row * s, n, X + row * K, K, lane);
    if (lane == 0 && n > 0) atomicMax(it_max, n);
}

// mask_ndim == 2.  Enqueues only; w.it holds the step count once the stream has run.  Profiling labels (when on):
// DCP_PROF_GRAM the s products of every pass, DCP_PROF_XUPDATE the step kernels, DCP_PROF_MISC everything else.
template <class T>
inline int omp_mask_solve(dcp_handle* h, const T* Y, const real_t<T>* M, const T* A, T* X, int64_t N, int F, int K,
                          int s, double tol, int64_t Nc, OmpMaskWs<T>& w) {
    typedef real_t<T> R;
    hipStream_t st = h->stream;
    const R t = tol >= 0.0 ? (R)tol : R(-1);
    {
        ProfScope ps(h, DCP_PROF_MISC);
        hipLaunchKernelGGL((omp_mask_abs2_kernel<T>), dim3(grid_for((long)K * F)), dim3(256), 0, st, A, (long)K * F, w.A2,
                           w.it);
        DCP_LAUNCH_OK(h, hipGetLastError());
    }
    bool ext_ready = false;
    for (int64_t r0 = 0; r0 < N; r0 += Nc) {
        const int nc = (int)(N - r0 < Nc ? N - r0 : Nc);
        const T* Yp = Y + r0 * F;
        const R* Mp = M + r0 * F;
        {
            ProfScope ps(h, DCP_PROF_MISC);
            GemmArgs<R> g;   // W = M (|A|^2)^T
            g.A = Mp; g.lda = F; g.B = w.A2; g.ldb = F; g.M = nc; g.N = K; g.K = F;
            DCP_LAUNCH_OK(h, (gemm<FORM_NT>(st, g, EpiStore<R>{w.W, K})));
            hipLaunchKernelGGL((omp_mask_init_kernel<T>), dim3(nc), dim3(64), 0, st, Yp, Mp, (long)F, w.Rm, w.r2, w.stat);
            DCP_LAUNCH_OK(h, hipGetLastError());
        }
        for (int step = 0; step < s; ++step) {
            {
                ProfScope ps(h, DCP_PROF_GRAM);
                GemmArgs<T> a;   // alpha = Rm A^H
                a.A = w.Rm; a.lda = F; a.B = A; a.ldb = F; a.M = nc; a.N = K; a.K = F; a.conjB = true;
                a.ext_ws = w.ext1;
                a.ext_ready = ext_ready;
                DCP_LAUNCH_OK(h, (gemm<FORM_NT>(st, a, EpiStore<T>{w.alpha, K})));
                ext_ready = true;
            }
            ProfScope ps(h, DCP_PROF_XUPDATE);
            hipLaunchKernelGGL((omp_mask_step_kernel<T>), dim3(nc), dim3(64), OmpCarve<T>(s).bytes, st, Yp, Mp, A,
                               (const T*)w.alpha, (const R*)w.W, w.Rm, w.L, w.z, w.x, w.sel, w.stat, w.r2, F, K, s, t);
            DCP_LAUNCH_OK(h, hipGetLastError());
        }
        ProfScope ps(h, DCP_PROF_MISC);
        hipLaunchKernelGGL((omp_mask_finish_kernel<T>), dim3(nc), dim3(64), 0, st, (const T*)w.x, (const int*)w.sel,
                           (const int*)w.stat, X + r0 * K, K, s, w.it);
        DCP_LAUNCH_OK(h, hipGetLastError());
    }
    return DCP_OK;
}

// The coder of every entry that codes rows by OMP (dcp_omp_*, dcp_omp_mask_*, the K-SVD steps).  How a mask selects
// the route is decided here and nowhere else:
//   mask_ndim 0  no mask: omp_solve
//   mask_ndim 1  one shared mask, one shared Gram matrix: omp_solve on sqrt(m) y, sqrt(m) A (Ys, As)
//   mask_ndim 2  omp_mask_solve in passes of Nc rows
// layout() takes the route's workspace (a caller appends its own items after it), solve() enqueues only, and
// it_dev() is the device word that holds the step count once the stream has run.
template <class T>
struct OmpCoder {
    typedef real_t<T> R;
    const R* M;
    int mask_ndim, rows_per_pass;
    LassoWs<T> lw;
    OmpMaskWs<T> ow;
    T* Ys = nullptr;
    T* As = nullptr;
    int64_t Nc = 0;

    OmpCoder(const R* M_, int ndim, int rpp) : M(M_), mask_ndim(ndim), rows_per_pass(rpp) {}

    void layout(WsLayout& a, int64_t N, int64_t F, int64_t K, int s) {
        if (mask_ndim == 2) {
            Nc = omp_mask_rows_per_pass<T>(N, F, K, s, rows_per_pass);
            omp_mask_layout<T>(a, ow, Nc, F, K, s);
            return;
        }
        if (mask_ndim == 1) {
            a.take(Ys, (size_t)N * F);
            a.take(As, (size_t)K * F);
        }
        omp_layout<T>(a, lw, N, F, K);
    }

    int sqrt_scale(dcp_handle* h, const T* a, int64_t rows, int64_t F, T* out) const {
        hipLaunchKernelGGL((omp_mask_sqrt_scale_kernel<T>), dim3(grid_for((long)rows * F)), dim3(256), 0, h->stream, a, M,
                           (long)rows, (long)F, out);
        DCP_LAUNCH_OK(h, hipGetLastError());
        return DCP_OK;
    }

    int solve(dcp_handle* h, const T* Y, const T* A, T* X, int64_t N, int64_t F, int64_t K, int s, double tol) {
        if (mask_ndim == 2) return omp_mask_solve<T>(h, Y, M, A, X, N, (int)F, (int)K, s, tol, Nc, ow);
        if (mask_ndim == 1) {
            DCP_TRY(sqrt_scale(h, Y, N, F, Ys));
            DCP_TRY(sqrt_scale(h, A, K, F, As));
            Y = Ys;
            A = As;
        }
        return omp_solve<T>(h, Y, A, X, (int)N, (int)F, (int)K, s, tol, lw);
    }

    const int* it_dev() const { return mask_ndim == 2 ? ow.it : lw.flag; }
};

// What a masked entry refuses about its mask arguments, after the null pointers and before the sizes (`who` is the
// entry's family in the message; an entry without passes gives rows_per_pass = 0).
inline int omp_check_mask(dcp_handle* h, const char* who, int mask_ndim, int rows_per_pass) {
    if (mask_ndim != 1 && mask_ndim != 2)
        return fail(h, DCP_ERR_INVALID, std::string(who) + ": mask_ndim must be 1 or 2");
    if (rows_per_pass < 0) return fail(h, DCP_ERR_INVALID, "omp: rows_per_pass must not be negative");
    return DCP_OK;
}

// dcp_omp_* (masked false: M, mask_ndim and rows_per_pass are nullptr, 0, 0) and dcp_omp_mask_*
template <class T>
inline int omp_api(dcp_handle* h, const T* Y, const real_t<T>* M, int mask_ndim, bool masked, const T* A, T* X,
                   int64_t N, int64_t F, int64_t K, int n_nonzero, double tol, int rows_per_pass, int* it_out) {
    if (!h) return DCP_ERR_INVALID;
    if (!Y || (masked && !M) || !A || !X || !it_out) return fail(h, DCP_ERR_INVALID, "null pointer");
    if (masked) DCP_TRY(omp_check_mask(h, "omp", mask_ndim, rows_per_pass));
    DCP_TRY(omp_check_problem<T>(h, N, F, K, n_nonzero, tol));
    DCP_HIP_OK(h, hipSetDevice(h->device));
    OmpCoder<T> coder(M, mask_ndim, rows_per_pass);
    DCP_TRY(ws_lay_out(h, [&](WsLayout& a) { coder.layout(a, N, F, K, n_nonzero); }));
    DCP_TRY(coder.solve(h, Y, A, X, N, F, K, n_nonzero, tol));
    return omp_read_it(h, coder.it_dev(), it_out);
}

}  // namespace dcp
