// Replacement of unused and duplicate atoms for K-SVD (Aharon, Elad & Bruckstein 2006, section IV-D; "cleardict" in
// Rubinstein's ksvdbox): one cleaning pass on what a sweep of ksvd.hpp leaves behind -- X, D, the maintained
// residual R = Y - X D, the mask m (1 without a mask) and cnt_k, the non-zeros of column k of X.
//   marking      for k = 0 .. K-1 in order, with G = D D^H in the working dtype: atom k is marked if cnt_k == 0, or
//                if a threshold mu is given and there is a j < k, itself not marked, with |G_kj| > mu.  A marked atom
//                never marks another one; of a coherent pair the lower index survives.
//   ranking      e_i = sum_f m_if |R_if|^2 over the entries with m_if > 0; the rows in the order (e descending,
//                i ascending), where a row whose e_i > 0 is false (zero, NaN) counts as e_i = 0.  A total order: the
//                result does not depend on how it is computed.
//   replacement  the j-th marked atom (ascending k) takes the j-th row i of that order: z_f = y_if where m_if > 0,
//                z_f = sum_k x_ik D_kf elsewhere, from the row's own non-zeros in ascending k and the D the sweep
//                left -- never y - R, so y at hidden entries reaches nothing.  D[k] = z / |z| if e_i > 0 and |z| > 0
//                (a NaN keeps the atom); with fewer such rows than marked atoms the remaining atoms are kept.  All
//                z are formed before any atom is written, so no fill sees a new atom.  X is not touched.
//
// Kernels.  No float atomics; every sum has a fixed order that depends on the sizes alone: bitwise reproducible.
//   count    ksvd_count (ksvd.hpp) on the swept X: cnt
//   gram     G = D D^H by gram_kk, the product the OMP coder forms, into workspace (only with a threshold)
//   hot      a wave per atom: hot[k] = any j < k with |G_kj| > mu, whatever j's mark -- necessary for the coherence
//            rule, and false for nearly every atom, so the sequential walk below skips the row
//   mark     ONE workgroup walks k in order; for a hot k, row k of G against the unmarked j < k is a workgroup
//            reduction.  It writes the list of marked atoms (ascending) and its length.
//   energy   a wave per row of R (and of m; row stride F, or 0 for a 1-D mask), per lane in increasing f, then the
//            butterfly; 16-byte loads where the rows are aligned as ksvd_sweep asks; accumulated in the real type
//   select   the first n rows of the order: every workgroup sorts its kKsvdSelBlock rows in LDS (a bitonic network on
//            (e, i) pairs) and leaves its first min(n, kKsvdSelBlock) as candidates;
//   merge    one workgroup merges the sorted candidate lists, one output per round (the best of the list heads).  For a
//            handful of marked atoms both cost a small multiple of one pass over e.
//   build    a wave per marked atom forms z and |z| into a [n, F] scratch
//   write    D[k] = z / |z| for the atoms whose row qualified
#pragma once

namespace dcp {

constexpr int kKsvdSelBlock = 1024;   // rows per workgroup of the selection's first stage

// (e, i) before (f, j) in the order of the ranking; e and f are not NaN
template <class R>
__device__ __forceinline__ bool ksvd_clean_before(R e, int i, R f, int j) {
    return e > f || (e == f && i < j);
}

// ---- energy: e[i] = sum_f m_if |R_if|^2.  grid: ceil(N / 4) workgroups of 256, a wave per row. -------------------
template <class T, int V>
__global__ void __launch_bounds__(256) ksvd_clean_energy_kernel(const T* __restrict__ Rm,
                                                                const real_t<T>* __restrict__ M, long ms, int N,
                                                                long F, real_t<T>* __restrict__ e) {
    typedef real_t<T> R;
    typedef KsvdPack<T, V> P;
    typedef KsvdMaskPack<R, V> MP;
    const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
    const long i = blockIdx.x * 4L + wave;
    if (i >= N) return;
    const T* r = Rm + i * F;
    R a = 0;
    if (M != nullptr) {
        const R* m = M + i * ms;
#pragma unroll 4
        for (long j = (long)lane * V; j < F; j += 64 * V) {
            const P rv = *reinterpret_cast<const P*>(r + j);
            const MP mv = *reinterpret_cast<const MP*>(m + j);
#pragma unroll
            for (int q = 0; q < V; ++q)   // a hidden entry adds nothing, whatever R holds there (0 * inf is NaN)
                if (mv.v[q] > R(0)) a = fmadd(a, mv.v[q], abs2(rv.v[q]));
        }
    } else {
#pragma unroll 4
        for (long j = (long)lane * V; j < F; j += 64 * V) {
            const P rv = *reinterpret_cast<const P*>(r + j);
#pragma unroll
            for (int q = 0; q < V; ++q) a += abs2(rv.v[q]);
        }
    }
    a = wave_sum_all(a);
    if (lane == 0) e[i] = a;
}

// ---- hot[k] = any j < k with |G_kj| > mu.  grid: ceil(K / 4) workgroups of 256, a wave per atom. -----------------
template <class T>
__global__ void __launch_bounds__(256) ksvd_clean_hot_kernel(const T* __restrict__ G, int K, real_t<T> mu,
                                                             int* __restrict__ hot) {
    const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
    const long k = blockIdx.x * 4L + wave;
    if (k >= K) return;
    bool any = false;
    for (long j = lane; j < k; j += 64) any = any || absval(G[k * K + j]) > mu;
    const unsigned long long b = __ballot(any);
    if (lane == 0) hot[k] = b != 0ull ? 1 : 0;
}

// ---- marking: ONE workgroup of 256 walks k = 0 .. K-1.  flag[k] <- marked; list[0 .. n) <- the marked atoms in
// ascending order; nmark[0] <- n.  flag[j] is written and read by thread j & 255 alone, so the walk needs no barrier
// beyond the reduction's own. --------------------------------------------------------------------------------------
template <class T>
__global__ void __launch_bounds__(256) ksvd_clean_mark_kernel(const T* __restrict__ G, const int* __restrict__ cnt,
                                                              const int* __restrict__ hot, int K, real_t<T> mu,
                                                              int use_mu, int* __restrict__ flag,
                                                              int* __restrict__ list, int* __restrict__ nmark) {
    const int tid = threadIdx.x;
    int n = 0;
    for (int k = 0; k < K; ++k) {
        bool mark = cnt[k] == 0;
        if (!mark && use_mu && hot[k] != 0) {   // workgroup-uniform
            int any = 0;
            for (int j = tid; j < k; j += 256) any |= (flag[j] == 0 && absval(G[(long)k * K + j]) > mu) ? 1 : 0;
            mark = __syncthreads_or(any) != 0;
        }
        if (tid == (k & 255)) flag[k] = mark ? 1 : 0;
        if (mark) {
            if (tid == 0) list[n] = k;
            ++n;
        }
    }
    if (tid == 0) nmark[0] = n;
}

// ---- select: workgroup b sorts rows [b SB, (b + 1) SB) by (e descending, i ascending), e taken as 0 where !(e > 0);
// rows past N sort last as (-1, INT_MAX).  cand[b, 0 .. c) <- its first c.  grid: ceil(N / SB) workgroups of 256. ---
template <class R>
__global__ void __launch_bounds__(256) ksvd_clean_select_kernel(const R* __restrict__ e, int N, int c,
                                                                R* __restrict__ cand_e, int* __restrict__ cand_i) {
    __shared__ R se[kKsvdSelBlock];
    __shared__ int si[kKsvdSelBlock];
    const int tid = threadIdx.x;
    const long r0 = (long)blockIdx.x * kKsvdSelBlock;
    for (int t = tid; t < kKsvdSelBlock; t += 256) {
        const long i = r0 + t;
        R v = R(-1);
        int id = 0x7fffffff;
        if (i < N) {
            const R x = e[i];
            v = x > R(0) ? x : R(0);
            id = (int)i;
        }
        se[t] = v;
        si[t] = id;
    }
    __syncthreads();
    for (int k = 2; k <= kKsvdSelBlock; k <<= 1) {
        for (int j = k >> 1; j > 0; j >>= 1) {
            for (int t = tid; t < kKsvdSelBlock; t += 256) {
                const int l = t ^ j;
                if (l > t) {
                    const R ea = se[t], eb = se[l];
                    const int ia = si[t], ib = si[l];
                    const bool first = (t & k) == 0;   // this run is sorted in the ranking's order, or against it
                    const bool swap = first ? ksvd_clean_before(eb, ib, ea, ia) : ksvd_clean_before(ea, ia, eb, ib);
                    if (swap) {
                        se[t] = eb; si[t] = ib;
                        se[l] = ea; si[l] = ia;
                    }
                }
            }
            __syncthreads();
        }
    }
    for (int t = tid; t < c; t += 256) {
        cand_e[(long)blockIdx.x * c + t] = se[t];
        cand_i[(long)blockIdx.x * c + t] = si[t];
    }
}

// ---- merge: ONE workgroup of 256; sel[r] <- the r-th row of the order over the B sorted candidate lists of length
// c, r < n, or -1 once every list is used up.  pos [B] is workspace; pos[b] belongs to thread b & 255. -------------
template <class R>
__global__ void __launch_bounds__(256) ksvd_clean_merge_kernel(const R* __restrict__ cand_e,
                                                               const int* __restrict__ cand_i, int B, int c, int n,
                                                               int* __restrict__ pos, int* __restrict__ sel) {
    __shared__ R we[4];
    __shared__ int wi[4], wb[4];
    const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
    for (int b = tid; b < B; b += 256) pos[b] = 0;
    for (int r = 0; r < n; ++r) {
        R be = R(-1);
        int bi = 0x7fffffff, bb = -1;
        for (int b = tid; b < B; b += 256) {
            const int p = pos[b];
            if (p < c) {
                const R v = cand_e[(long)b * c + p];
                const int id = cand_i[(long)b * c + p];
                if (ksvd_clean_before(v, id, be, bi)) {
                    be = v; bi = id; bb = b;
                }
            }
        }
#pragma unroll
        for (int m = 32; m >= 1; m >>= 1) {
            const R oe = lane_xor(be, m);
            const int oi = lane_xor(bi, m), ob = lane_xor(bb, m);
            if (ksvd_clean_before(oe, oi, be, bi)) {
                be = oe; bi = oi; bb = ob;
            }
        }
        if (lane == 0) {
            we[wave] = be; wi[wave] = bi; wb[wave] = bb;
        }
        __syncthreads();
        R fe = we[0];
        int fi = wi[0], fb = wb[0];
#pragma unroll
        for (int w = 1; w < 4; ++w) {
            if (ksvd_clean_before(we[w], wi[w], fe, fi)) {
                fe = we[w]; fi = wi[w]; fb = wb[w];
            }
        }
        __syncthreads();   // the next round writes we, wi, wb
        if (fb >= 0 && tid == (fb & 255)) pos[fb] += 1;
        if (tid == 0) sel[r] = fb >= 0 ? fi : -1;
    }
}

// ---- build: a wave per marked atom j < n with its row i = sel[j]: Z[j, :] <- z, znorm[j] <- |z|, ok[j] <- whether
// the atom is replaced (i >= 0, e_i > 0, |z| > 0).  64 columns at a time, a lane per column; where a column of the
// tile is hidden the wave walks the row of X in ascending k and every hidden lane adds x_ik D_kf.  |z|^2 per lane in
// increasing f, then the butterfly.  grid: ceil(n / 4) workgroups of 256. -------------------------------------------
template <class T>
__global__ void __launch_bounds__(256) ksvd_clean_build_kernel(const T* __restrict__ Y,
                                                               const real_t<T>* __restrict__ M, long ms,
                                                               const T* __restrict__ X, const T* __restrict__ D,
                                                               const real_t<T>* __restrict__ e,
                                                               const int* __restrict__ sel, int n, int K, long F,
                                                               T* __restrict__ Z, real_t<T>* __restrict__ znorm,
                                                               int* __restrict__ ok) {
    typedef real_t<T> R;
    const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
    const long j = blockIdx.x * 4L + wave;
    if (j >= n) return;
    const long i = sel[j];
    bool use = i >= 0;
    if (use) use = e[i] > R(0);
    if (!use) {   // wave-uniform
        if (lane == 0) {
            ok[j] = 0;
            znorm[j] = R(0);
        }
        return;
    }
    const T* y = Y + i * F;
    const R* m = M != nullptr ? M + i * ms : nullptr;
    const T* x = X + i * K;
    T* z = Z + j * F;
    R a = 0;
    for (long f0 = 0; f0 < F; f0 += 64) {
        const long f = f0 + lane;
        const bool live = f < F;
        const bool hidden = live && m != nullptr && !(m[f] > R(0));
        T v = zero_of<T>();
        if (__ballot(hidden) != 0ull) {
            for (int k0 = 0; k0 < K; k0 += 64) {
                const T xv = k0 + lane < K ? x[k0 + lane] : zero_of<T>();
                unsigned long long nz = __ballot(ksvd_nz(xv));
                while (nz != 0ull) {
                    const int l = __ffsll(nz) - 1;
                    nz &= nz - 1ull;
                    const T c = lane_get(xv, l);
                    if (hidden) v = fmadd(v, c, D[(long)(k0 + l) * F + f]);
                }
            }
        }
        if (live && !hidden) v = y[f];
        if (live) {
            z[f] = v;
            a += abs2(v);
        }
    }
    a = wave_sum_all(a);
    const R nrm = sqrt(a);
    if (lane == 0) {
        znorm[j] = nrm;
        ok[j] = nrm > R(0) ? 1 : 0;
    }
}

// ---- write: D[list[j], :] = Z[j, :] / znorm[j] where ok[j]; grid-stride over the n F elements. -------------------
template <class T>
__global__ void __launch_bounds__(256) ksvd_clean_write_kernel(const T* __restrict__ Z,
                                                               const real_t<T>* __restrict__ znorm,
                                                               const int* __restrict__ ok,
                                                               const int* __restrict__ list, int n, long F,
                                                               T* __restrict__ D) {
    const long total = (long)n * F;
    for (long t = blockIdx.x * 256L + threadIdx.x; t < total; t += (long)gridDim.x * 256L) {
        const long j = t / F, f = t - j * F;
        if (ok[j] != 0) D[(long)list[j] * F + f] = ksvd_div(Z[t], znorm[j]);
    }
}

// ---- workspace: appended after the existing carve, so ksvd_layout lays out what it always did --------------------
template <class T>
struct KsvdCleanWs {
    LassoWs<T> g;                 // AAt [K, K] = G, slabs and (complex) ext1: what gram_kk uses; threshold only
    int* hot = nullptr;           // [K]
    int* flag = nullptr;          // [K] marked
    int* list = nullptr;          // [K] the marked atoms, ascending
    int* nmark = nullptr;         // [4] their number
    real_t<T>* e = nullptr;       // [N] row energies
    real_t<T>* cand_e = nullptr;  // [ceil(N / SB), min(K, SB)] the candidates of the selection
    int* cand_i = nullptr;
    int* pos = nullptr;           // [ceil(N / SB)] the merge's list heads
    int* sel = nullptr;           // [K] the chosen rows
    T* Z = nullptr;               // [K, F] the candidates z
    real_t<T>* znorm = nullptr;   // [K]
    int* ok = nullptr;            // [K]
};

template <class T>
inline void ksvd_clean_layout(WsLayout& a, KsvdCleanWs<T>& c, int64_t N, int64_t F, int64_t K, bool coherence) {
    const size_t nb = (size_t)((N + kKsvdSelBlock - 1) / kKsvdSelBlock);
    const size_t cmax = (size_t)(K < kKsvdSelBlock ? K : kKsvdSelBlock);
    if (coherence) {
        a.take(c.g.AAt, (size_t)K * K);
        c.g.slab_count = (size_t)kMaxSplits * K * K;
        a.take(c.g.slabs, c.g.slab_count);
        if (scalar_traits<T>::is_complex) a.take(c.g.ext1, (size_t)4 * K * F);
    }
    a.take(c.hot, (size_t)K);
    a.take(c.flag, (size_t)K);
    a.take(c.list, (size_t)K);
    a.take(c.nmark, 4);
    a.take(c.e, (size_t)N);
    a.take(c.cand_e, nb * cmax);
    a.take(c.cand_i, nb * cmax);
    a.take(c.pos, nb);
    a.take(c.sel, (size_t)K);
    a.take(c.Z, (size_t)K * F);
    a.take(c.znorm, (size_t)K);
    a.take(c.ok, (size_t)K);
}

// Enqueues the marking on the swept X and D: afterwards c.list holds the marked atoms and c.nmark[0] their number.
// max_coherence <= 0: unused atoms only.  (ksvd_count overwrites the counts and offsets of the sweep's lists, which
// nothing reads after the last atom.)
template <class T>
inline int ksvd_clean_mark(dcp_handle* h, const T* X, const T* D, int N, int F, int K, double max_coherence,
                           KsvdWs<T>& w, KsvdCleanWs<T>& c) {
    typedef real_t<T> R;
    hipStream_t st = h->stream;
    const int use_mu = max_coherence > 0.0 ? 1 : 0;
    DCP_TRY(ksvd_count<T>(h, X, N, K, w));
    if (use_mu) {
        DCP_TRY(gram_kk<T>(h, D, D, K, F, c.g, c.g.AAt));
        hipLaunchKernelGGL((ksvd_clean_hot_kernel<T>), dim3((K + 3) / 4), dim3(256), 0, st, (const T*)c.g.AAt, K,
                           (R)max_coherence, c.hot);
        DCP_LAUNCH_OK(h, hipGetLastError());
    }
    hipLaunchKernelGGL((ksvd_clean_mark_kernel<T>), dim3(1), dim3(256), 0, st, (const T*)c.g.AAt,
                       (const int*)(w.meta + 4), (const int*)c.hot, K, (R)max_coherence, use_mu, c.flag, c.list,
                       c.nmark);
    DCP_LAUNCH_OK(h, hipGetLastError());
    return DCP_OK;
}

// Enqueues energies, selection and replacement for the n > 0 atoms of c.list, on the residual w.R.
template <class T>
inline int ksvd_clean_apply(dcp_handle* h, const T* Y, KsvdMask<real_t<T>> m, const T* X, T* D, int N, int F, int K,
                            int n, KsvdWs<T>& w, KsvdCleanWs<T>& c) {
    typedef real_t<T> R;
    constexpr int V = ksvd_vec<T>();
    hipStream_t st = h->stream;
    // 16-byte accesses under ksvd_sweep's condition, for what is read here: the rows of R and of the mask
    const bool vec = V > 1 && ((size_t)F * sizeof(T)) % 16 == 0 &&
                     (!m.M || reinterpret_cast<uintptr_t>(m.M) % (V * sizeof(R)) == 0);
    const dim3 ge((unsigned)((N + 3) / 4));
    if (vec)
        hipLaunchKernelGGL((ksvd_clean_energy_kernel<T, V>), ge, dim3(256), 0, st, (const T*)w.R, m.M, m.ms, N,
                           (long)F, c.e);
    else
        hipLaunchKernelGGL((ksvd_clean_energy_kernel<T, 1>), ge, dim3(256), 0, st, (const T*)w.R, m.M, m.ms, N,
                           (long)F, c.e);
    DCP_LAUNCH_OK(h, hipGetLastError());
    const int nb = (N + kKsvdSelBlock - 1) / kKsvdSelBlock;
    const int cn = n < kKsvdSelBlock ? n : kKsvdSelBlock;
    hipLaunchKernelGGL((ksvd_clean_select_kernel<R>), dim3(nb), dim3(256), 0, st, (const R*)c.e, N, cn, c.cand_e,
                       c.cand_i);
    DCP_LAUNCH_OK(h, hipGetLastError());
    hipLaunchKernelGGL((ksvd_clean_merge_kernel<R>), dim3(1), dim3(256), 0, st, (const R*)c.cand_e,
                       (const int*)c.cand_i, nb, cn, n, c.pos, c.sel);
    DCP_LAUNCH_OK(h, hipGetLastError());
    hipLaunchKernelGGL((ksvd_clean_build_kernel<T>), dim3((n + 3) / 4), dim3(256), 0, st, Y, m.M, m.ms, X,
                       (const T*)D, (const R*)c.e, (const int*)c.sel, n, K, (long)F, c.Z, c.znorm, c.ok);
    DCP_LAUNCH_OK(h, hipGetLastError());
    hipLaunchKernelGGL((ksvd_clean_write_kernel<T>), dim3(grid_for((long)n * F)), dim3(256), 0, st, (const T*)c.Z,
                       (const R*)c.znorm, (const int*)c.ok, (const int*)c.list, n, (long)F, D);
    DCP_LAUNCH_OK(h, hipGetLastError());
    return DCP_OK;
}

// host <- max|D_new - D_old| (NaN wins) and the number of marked atoms: one synchronisation for both
template <class T>
inline int ksvd_clean_read(dcp_handle* h, const KsvdWs<T>& w, const KsvdCleanWs<T>& c, long n, double* maxdiff_out,
                           int* n_marked_out) {
    void* hostv = nullptr;
    DCP_TRY(host_scratch(h, (kKsvdMdParts + 1) * sizeof(double), &hostv));
    double* hd = reinterpret_cast<double*>(hostv);
    int* hn = reinterpret_cast<int*>(hd + kKsvdMdParts);
    const int parts = grid_for(n, kKsvdMdParts);
    DCP_HIP_OK(h, hipMemcpyAsync(hd, w.mdpart, parts * sizeof(double), hipMemcpyDeviceToHost, h->stream));
    DCP_HIP_OK(h, hipMemcpyAsync(hn, c.nmark, sizeof(int), hipMemcpyDeviceToHost, h->stream));
    DCP_HIP_OK(h, hipStreamSynchronize(h->stream));
    double md = 0.0;
    for (int i = 0; i < parts; ++i) md = max_np(hd[i], md);
    *maxdiff_out = md;
    *n_marked_out = *hn;
    return DCP_OK;
}

// What the cleaning entries refuse about the mask and the two reals, before anything is written
inline int ksvd_clean_check(dcp_handle* h, const void* M, int mask_ndim, double max_coherence, double stop_tol) {
    if (mask_ndim < 0 || mask_ndim > 2) return fail(h, DCP_ERR_INVALID, "ksvd: mask_ndim must be 0, 1 or 2");
    if ((mask_ndim == 0) != (M == nullptr))
        return fail(h, DCP_ERR_INVALID, "ksvd: a mask goes with mask_ndim 1 or 2, no mask with mask_ndim 0");
    if (max_coherence != max_coherence) return fail(h, DCP_ERR_INVALID, "ksvd: max_coherence is NaN");
    if (stop_tol != stop_tol) return fail(h, DCP_ERR_INVALID, "ksvd: stop_tol is NaN");
    return DCP_OK;
}

// dcp_ksvd_clean_*: R = Y - X D as the sweep forms it, then one cleaning pass on the caller's X and D.
template <class T>
inline int ksvd_clean_api(dcp_handle* h, const T* Y, const real_t<T>* M, int mask_ndim, const T* X, T* D, int64_t N,
                          int64_t F, int64_t K, double max_coherence, int* n_marked_out, int* n_replaced_out) {
    if (!h) return DCP_ERR_INVALID;
    if (!Y || !X || !D || !n_marked_out || !n_replaced_out) return fail(h, DCP_ERR_INVALID, "null pointer");
    DCP_TRY(ksvd_clean_check(h, M, mask_ndim, max_coherence, 0.0));
    DCP_TRY(omp_check_sizes(h, N, F, K));
    DCP_HIP_OK(h, hipSetDevice(h->device));
    KsvdWs<T> w;
    KsvdCleanWs<T> c;
    DCP_TRY(ws_lay_out(h, [&](WsLayout& a) {
        ksvd_layout<T>(a, w, N, F, K, 1, false);
        ksvd_clean_layout<T>(a, c, N, F, K, max_coherence > 0.0);
    }));
    DCP_TRY(ksvd_residual<T>(h, Y, X, (const T*)D, (int)N, (int)F, (int)K, w));
    DCP_TRY(ksvd_clean_mark<T>(h, X, (const T*)D, (int)N, (int)F, (int)K, max_coherence, w, c));
    int n = 0;
    DCP_TRY(read_scalar(h, (const int*)c.nmark, &n));
    *n_marked_out = n;
    *n_replaced_out = 0;
    if (n == 0) return DCP_OK;
    const KsvdMask<real_t<T>> m{M, mask_ndim == 2 ? (long)F : 0L};
    DCP_TRY(ksvd_clean_apply<T>(h, Y, m, X, D, (int)N, (int)F, (int)K, n, w, c));
    void* hostv = nullptr;
    DCP_TRY(host_scratch(h, (size_t)n * sizeof(int), &hostv));
    int* ok = reinterpret_cast<int*>(hostv);
    DCP_TRY(read_words(h, (const int*)c.ok, n, ok));
    int rep = 0;
    for (int j = 0; j < n; ++j) rep += ok[j];
    *n_replaced_out = rep;
    return DCP_OK;
}

}  // namespace dcp
