// Orthogonal convolutional pursuit on the template operator (template_matching.orthogonal_pursuit, dcp_tm_omp_*):
// batch OMP (Rubinstein, Zibulevsky & Elad 2008) on the shift-invariant dictionary.  Included from template_impl.hpp
// after template_pursuit.hpp, whose prepare kernels, segment table, table reduction, window, Gram entry and launch
// it uses; the factor is greedy.hpp's OmpFactor.
//
// Per signal y [N], independent of the others, with A[(t, c), n] = D[t, n - s c + Q], rho2[t, c] = |A_(t,c)|^2 and
// G[i, k] = A_i . A_k^H over the samples inside [0, N), alpha0 = y A^H, support I = (), x = 0, E = |y|^2, at most
// n_steps times:
//   1. tol given and E <= tol: stop
//   2. alpha_k = r . A_k^H;  score = |alpha_k|^2 / rho2_k over the atoms with rho2_k > 0 that are not in I;  k* = the
//      LOWEST flat index t C + c attaining the maximum;  maximum not > 0 (or NaN): stop
//   3. L w = G[I, k*] (L: the Cholesky factor of G_II),  d = rho2_k* - |w|^2;  d <= eps_dep rho2_k* (omp_eps_dep, 4096
//      eps: A_k* numerically in the span of A_I): stop, keeping the previous x
//   4. I <- I + (k*);  L gains the row (w^H, sqrt(d));  L z = conj(alpha0_I) (only z's last entry is new),
//      L^H v = z, x_I = conj(v);  E = |y|^2 - Re(x_I . conj(alpha0_I))
// r is never formed.  alpha is kept up to date in Gram form: alpha -= sum_j (x_j - x_j^previous) G[I_j, :], every term
// touching only the T (2 dh + 1) atoms within dh of I_j.  G[i, k] is one read of the lag correlations
// Corr[t_i, t_k, s (c_i - c_k)] when every tap of atom i lies inside the signal, else the explicit sum over the overlap
// inside [0, N) (tm_pursuit_gram); it is an exact zero when |c_i - c_k| > dh.
//
// A support atom that no chain of overlaps connects to k* keeps its coefficient bit for bit: its entry of w is an
// exact zero (its G entry is, and so is every factor entry that couples it to the cluster of k*), so row n of L holds
// a zero in its column and the back substitution subtracts 0 v_n from it.  Terms with x_j == x_j^previous are
// therefore skipped, exactly: a step costs the cluster of overlapping events, not the support.
//
// Prepare: rho2, Corr and alpha0 by the kernels of pursuit (tm_pursuit_prepare).
// Kernel tm_omp_kernel<T, LDS>: one 1024-thread workgroup per signal on the decomposition of tm_pursuit_kernel; no
// waiting between workgroups, no float atomics (one integer max per signal for `it`), every loop bounded by n_steps.
//   arg-max     the 64-atom segment table of template_pursuit.hpp; support atoms score -1 (one bit per atom, a
//               64-bit word per segment, set when the atom is taken).  Ties go to the lower index at every level.
//   factor      wave 0 on greedy.hpp's OmpFactor: L [n][n | 1] in LDS, sel, alpha0_I, z, x_I, the previous x_I and
//               1 / L_jj in LDS beside it, lane j reading and writing entry j alone.
//   alpha       for j = 0 .. n - 1 in order, skipping x_j == x_j^previous (never the new atom): entry (t', c') of
//               window j belongs to thread (t' mod TPB) W + (c' mod W), W the power of two >= 2 dh + 1 (at most
//               1024), TPB = 1024 / W -- a function of the entry alone, so an entry that several windows cover is
//               always updated by the same thread, in one fixed order (that of j; by pass first when T > TPB or
//               2 dh + 1 > 1024), without a barrier between the windows and without an index division.  The G
//               entries of 8 (float) or 4 windows are fetched together.  The thread marks the entry's segment in
//               the table (index -1).
//   refresh     per changed window, the pairs (t', p-th segment of the run) are dealt to the 16 waves; a segment
//               that is still marked is reduced again (two waves meeting on one segment store the same entry).
//   per step    4 workgroup barriers (table result | factor | alpha | refresh).
//   tiers       LDS:    T C <= kTmOmpLdsBytes / sizeof(T) (28672 float, 14336 double / complex64, 7168 complex128):
//                       alpha [T C], the table and the support bits live in LDS beside the factor -- at the
//                       cap 112 KiB + 9 KiB + 36 KiB of the CU's 160 KiB at most.
//               global: above: alpha is a second copy [B, T C] in the workspace (alpha0 itself stays as it is: the
//                       alpha0 entry of an atom is read when the atom is taken), the table and the bits in
//                       per-signal workspace.
// Every value a signal's workgroup computes depends on that signal, D and the geometry alone, in a fixed order:
// results are bitwise reproducible and bitwise independent of the rest of the batch.
#pragma once
#include "omp.hpp"

namespace dcp {

constexpr size_t kTmOmpLdsBytes = 112 * 1024;   // the LDS image of alpha in the LDS tier

// the largest T C whose alpha is kept in LDS
template <class T>
constexpr long tm_omp_lds_atoms() { return (long)(kTmOmpLdsBytes / sizeof(T)); }

// LDS carve for at most n support atoms: L [n][n | 1], alpha0_I, z, x_I, previous x_I [n] (T), 1 / L_jj [n] (real),
// sel, its t and its c [n] (int), then (LDS tier) alpha [K] (T), the table [nseg] and the support bits [nseg] (64 per
// word); every item 16-byte aligned
template <class T>
struct TmOmpCarve {
    size_t a0s, z, xs, xp, dinv, sel, selt, selc, al, tab, taken, bytes;
    static DCP_HD size_t up(size_t b) { return (b + 15) & ~size_t(15); }
    DCP_HD TmOmpCarve(int n, long K, bool lds) {
        const size_t v = up((size_t)n * sizeof(T)), vi = up((size_t)n * sizeof(int));
        const size_t nseg = (size_t)((K + kTmPursuitSeg - 1) / kTmPursuitSeg);
        a0s = up((size_t)n * omp_ld(n) * sizeof(T));
        z = a0s + v;
        xs = z + v;
        xp = xs + v;
        dinv = xp + v;
        sel = dinv + up((size_t)n * sizeof(real_t<T>));
        selt = sel + vi;
        selc = selt + vi;
        al = selc + vi;
        tab = al + (lds ? up((size_t)K * sizeof(T)) : 0);
        taken = tab + (lds ? up(nseg * sizeof(TmBest<T>)) : 0);
        bytes = taken + (lds ? nseg * sizeof(unsigned long long) : 0);
    }
};

template <class T>
__device__ __forceinline__ bool tm_omp_is_zero(T v) {
    if constexpr (scalar_traits<T>::is_complex) return v.re == real_t<T>(0) && v.im == real_t<T>(0);
    else return v == T(0);
}

// lane l of the wave: atom 64 seg + l is in the support (bit i % 64 of taken[i / 64])
__device__ __forceinline__ bool tm_omp_taken(const unsigned long long* taken, int seg) {
    return ((taken[seg] >> (threadIdx.x & 63)) & 1ull) != 0;
}

// grid: B workgroups of kTmPursuitThreads threads; dynamic LDS TmOmpCarve<T>(n_max, K, LDS).bytes.  alpha0 [B, K]
// (K = T C < 2^31) is read only; ws_al [B, K], ws_tab [B, nseg] and ws_taken [B, nseg] are alpha, the table and the
// support bits of the global tier (unused in the LDS tier).  X [B, K] is written entirely.  *it_max (zero on entry)
// receives the largest support.
template <class T, bool LDS>
__global__ void __launch_bounds__(kTmPursuitThreads) tm_omp_kernel(const T* __restrict__ Y, const T* __restrict__ D,
                                                                   const T* __restrict__ corr,
                                                                   const real_t<T>* __restrict__ rho2,
                                                                   const T* __restrict__ alpha0, T* ws_al,
                                                                   TmBest<T>* ws_tab, unsigned long long* ws_taken,
                                                                   T* X, TmGeom g, int n_max, real_t<T> tol,
                                                                   int* __restrict__ it_max) {
    typedef real_t<T> R;
    constexpr int NT = kTmPursuitThreads, NW = kTmPursuitWaves;
    constexpr int U = sizeof(T) <= 4 ? 8 : 4;   // windows whose G entries are in flight together
    extern __shared__ __attribute__((aligned(16))) char tm_smem[];
    __shared__ R shS[NW];
    __shared__ int shI[NW];
    __shared__ R shE;
    __shared__ int shGo;
    const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
    const long b = blockIdx.x;
    const int C = (int)g.C, Tn = (int)g.T, K = Tn * C, nseg = (K + kTmPursuitSeg - 1) / kTmPursuitSeg;
    const int nd = (int)g.nd();
    const TmOmpCarve<T> cv(n_max, K, LDS);
    T* L = reinterpret_cast<T*>(tm_smem);
    T* a0s = reinterpret_cast<T*>(tm_smem + cv.a0s);
    T* zs = reinterpret_cast<T*>(tm_smem + cv.z);
    T* xs = reinterpret_cast<T*>(tm_smem + cv.xs);
    T* xp = reinterpret_cast<T*>(tm_smem + cv.xp);
    R* dinv = reinterpret_cast<R*>(tm_smem + cv.dinv);
    int* sel = reinterpret_cast<int*>(tm_smem + cv.sel);
    int* selt = reinterpret_cast<int*>(tm_smem + cv.selt);
    int* selc = reinterpret_cast<int*>(tm_smem + cv.selc);
    T* al;
    TmBest<T>* tab;
    unsigned long long* taken;
    if constexpr (LDS) {
        al = reinterpret_cast<T*>(tm_smem + cv.al);
        tab = reinterpret_cast<TmBest<T>*>(tm_smem + cv.tab);
        taken = reinterpret_cast<unsigned long long*>(tm_smem + cv.taken);
    } else {
        al = ws_al + b * K;
        tab = ws_tab + b * nseg;
        taken = ws_taken + b * nseg;
    }
    const T* a0row = alpha0 + b * K;
    for (int i = tid; i < K; i += NT) al[i] = a0row[i];
    for (int i = tid; i < nseg; i += NT) taken[i] = 0ull;
    T* x = X + b * K;
    for (int i = tid; i < K; i += NT) x[i] = zero_of<T>();
    const R yn2 = tm_pursuit_ynorm2(Y + b * g.Ch * g.N, g.Ch * g.N, shS, &shE);
    int n = 0;   // the support size
    for (int seg = wave; seg < nseg; seg += NW) tm_pursuit_segment(al, rho2, K, seg, 0, tm_omp_taken(taken, seg), tab);
    __syncthreads();
    // entry (t', c') of any window belongs to thread (t' mod TPB) W + (c' mod W), W = the power of two >= nd (<= NT)
    int W = 1;
    while (W < nd && W < NT) W <<= 1;
    const int TPB = NT / W, t0 = tid / W, r = tid & (W - 1);
    // the refresh deals (t', p-th segment of a run) to the waves: this wave's first pair and its stride
    const int nsp = (nd + kTmPursuitSeg - 2) / kTmPursuitSeg + 1;   // the most segments a run of nd can touch
    const int wq0 = wave / nsp, wp0 = wave - wq0 * nsp, dq = NW / nsp, dr = NW - dq * nsp;

    const bool use_tol = tol >= R(0);
    const int lc = lane < n_max ? lane : n_max - 1;   // this lane's row of the factor, clamped into the image
    R E = yn2;
    for (int it = 0; it < n_max; ++it) {
        if (use_tol && !(E > tol)) break;
        R bs;
        int bi;
        tm_pursuit_table_best(tab, nseg, shS, shI, bs, bi);
        if (!(bs > R(0))) break;
        // ---- wave 0: the Cholesky pivot L w = G[I, k*], then the re-fit ----
        if (wave == 0) {
            const int ts = bi / C, cs = bi - ts * C;
            const R gkk = rho2[bi];
            const T a0k = a0row[bi];
            const int tj = lane < n ? selt[lc] : ts, cj = lane < n ? selc[lc] : cs;
            const T bb = omp_keep(tm_pursuit_gram(D, corr, g, tj, cj, tm_pursuit_inside(g, cj), ts, cs), lane < n);
            const R dv = omp_keep(dinv[lc], lane < n);
            const OmpFactor<T> fac{L, omp_ld(n_max), lane, lc, n};
            R wn2;
            const T w = fac.forward(bb, dv, wn2);
            const R d = gkk - wn2;
            if (fac.dependent(d, gkk)) {   // keep the previous x
                if (lane == 0) shGo = 0;
            } else {
                const R ldiag = sqrt(d), rdiag = R(1) / ldiag;
                const T wc = omp_keep(conj_of(w), lane < n);   // row n of L, left of the diagonal
                const T zj = omp_keep(zs[lc], lane < n);
                const T zn = scale(sub(conj_of(a0k), wave_sum_all(mul(wc, zj))), rdiag);
                fac.accept(wc, ldiag);
                const T xn = conj_of(fac.backward(lane == n ? zn : zj, lane == n ? rdiag : dv, wc));
                const T xo = omp_keep(xs[lc], lane < n);
                const T a0m = lane == n ? a0k : omp_keep(a0s[lc], lane < n);
                if (lane <= n) {
                    xp[lane] = xo;
                    xs[lane] = xn;
                }
                if (lane == n) {
                    sel[n] = bi;
                    selt[n] = ts;
                    selc[n] = cs;
                    taken[bi / kTmPursuitSeg] |= 1ull << (bi & (kTmPursuitSeg - 1));
                    a0s[n] = a0k;
                    dinv[n] = rdiag;
                    zs[n] = zn;
                }
                const R fit = real_part(wave_sum_all(omp_keep(mul(xn, conj_of(a0m)), lane <= n)));
                if (lane == 0) {
                    shE = yn2 - fit;
                    shGo = 1;
                }
            }
        }
        __syncthreads();
        if (!shGo) break;
        E = shE;
        ++n;
        // ---- alpha -= (x_j - x_j^previous) G[I_j, :]: this thread's entries of every window, j in order.  The G
        //      entries of U windows are fetched before the first of them is applied (one at a time the loop is a
        //      chain of n global round trips).  One pass unless T > TPB or nd > NT. ----
        for (int tp = t0; tp < Tn; tp += TPB) {
            for (int cw = 0; cw < nd; cw += W) {
                for (int j0 = 0; j0 < n; j0 += U) {
                    T Gu[U], dxu[U];
                    int iu[U];
#pragma unroll
                    for (int u = 0; u < U; ++u) {
                        const int j = j0 + u < n ? j0 + u : n - 1;
                        const T dx = sub(xs[j], xp[j]);
                        const int tj = selt[j], cj = selc[j];
                        int ca, cb;
                        tm_pursuit_window(g, cj, ca, cb);
                        const int cp = ca + cw + ((r - ca) & (W - 1));   // the c' >= ca + cw with c' = r (mod W)
                        const bool on = j0 + u < n && (j == n - 1 || !tm_omp_is_zero(dx)) && cp <= cb;
                        iu[u] = on ? tp * C + cp : -1;
                        dxu[u] = dx;
                        Gu[u] = zero_of<T>();
                        if (on) Gu[u] = tm_pursuit_gram(D, corr, g, tj, cj, tm_pursuit_inside(g, cj), tp, cp);
                    }
#pragma unroll
                    for (int u = 0; u < U; ++u) {
                        if (iu[u] < 0) continue;
                        al[iu[u]] = fmsub(al[iu[u]], dxu[u], Gu[u]);
                        tab[iu[u] / kTmPursuitSeg].i = -1;
                    }
                }
            }
        }
        __syncthreads();
        // ---- reduce the marked segments again: template t' of window j wrote [t' C + ca, t' C + cb] ----
        for (int j = 0; j < n; ++j) {
            if (j != n - 1 && tm_omp_is_zero(sub(xs[j], xp[j]))) continue;
            int ca, cb;
            tm_pursuit_window(g, selc[j], ca, cb);
            int tq = wq0, p = wp0;
            while (tq < Tn) {
                const int seg = (tq * C + ca) / kTmPursuitSeg + p;
                if (seg <= (tq * C + cb) / kTmPursuitSeg && __builtin_amdgcn_readfirstlane(tab[seg].i) == -1)
                    tm_pursuit_segment(al, rho2, K, seg, 0, tm_omp_taken(taken, seg), tab);
                tq += dq;
                p += dr;
                if (p >= nsp) {
                    p -= nsp;
                    ++tq;
                }
            }
        }
        __syncthreads();
    }
    if (wave == 0 && lane < n) x[sel[lane]] = xs[lane];
    if (tid == 0 && n > 0) atomicMax(it_max, n);
}

// Y [B, N], D [T, S] (mc: Y [B, Ch, N], D [T, Ch, S]) -> X [B, T, C]; *it_out = the largest support a signal reached.
// Synchronises the stream.
template <class T>
inline int tm_omp_solve(dcp_handle* h, const T* Y, const T* D, T* X, const TmGeom& g, int n_steps, double tol,
                        int* it_out, bool mc) {
    typedef real_t<T> R;
    hipStream_t st = h->stream;
    const long K = g.T * g.C, nseg = tm_pursuit_nseg(K);
    const bool lds = K <= tm_omp_lds_atoms<T>();
    R* rho2 = nullptr;
    T* corr = nullptr;     // lag correlations
    T* alpha0 = nullptr;   // y A^H
    T* al = nullptr;       // the global tier's alpha
    TmBest<T>* tab = nullptr;   // the global tier's table
    unsigned long long* taken = nullptr;   // the global tier's support bits
    int* it_dev = nullptr;
    DCP_TRY(ws_lay_out(h, [&](WsLayout& a) {
        a.take(rho2, K);
        a.take(corr, g.T * g.T * (2 * g.S - 1));
        a.take(alpha0, g.B * K);
        a.take(al, lds ? 0 : g.B * K);
        a.take(tab, lds ? 0 : g.B * nseg);
        a.take(taken, lds ? 0 : g.B * nseg);
        a.take(it_dev, 4);
    }));
    DCP_TRY(tm_pursuit_prepare<T>(h, Y, D, g, rho2, corr, alpha0, it_dev, mc));
    const R t = tol >= 0.0 ? (R)tol : R(-1);
    const size_t bytes = TmOmpCarve<T>(n_steps, K, lds).bytes;
    DCP_LAUNCH_OK(h, (tm_pursuit_launch<&tm_omp_kernel<T, true>, &tm_omp_kernel<T, false>>(
                         st, g.B, lds, bytes, TmOmpCarve<T>(omp_cap<T>(), tm_omp_lds_atoms<T>(), true).bytes, Y, D,
                         (const T*)corr, (const R*)rho2, (const T*)alpha0, al, tab, taken, X, g, n_steps, t, it_dev)));
    return read_scalar(h, (const int*)it_dev, it_out);
}

// dcp_tm_omp_* and dcp_tm_mc_omp_*
template <class T>
inline int tm_omp_api(dcp_handle* h, const T* Y, const T* D, T* X, const TmShape& sh, int64_t n_steps, double tol,
                      int* it_out) {
    TmGeom g;
    DCP_TRY(tm_geom_api(h, sh, g));
    if (!Y || !D || !X || !it_out) return fail(h, DCP_ERR_INVALID, "null pointer");
    const int64_t K = (int64_t)g.T * g.C;
    if (K > 0x7fffff00LL) return fail(h, DCP_ERR_INVALID, "orthogonal pursuit: T C exceeds 2^31 - 257");
    DCP_TRY(omp_check_sparsity(h, K, n_steps, omp_cap<T>(), "orthogonal pursuit: n_steps", "T C"));
    if (tol != tol) return fail(h, DCP_ERR_INVALID, "orthogonal pursuit: tol is NaN");
    return tm_omp_solve<T>(h, Y, D, X, g, (int)n_steps, tol, it_out, sh.mc);
}

}  // namespace dcp
