// 1-D convolutional template learning (decomp/template_matching.py) without the im2col matrices.
//
// Geometry (reference _coef_size / _temp2mat / _coef2mat, restated in closed form):
//   C   = floor((S + 2 pad - N) / s) + 1,   pad = N - 1 (SAME) | N - S (VALID),   Q = s (C - 1) - pad
//   A[(t, c), n]     = D[t, n - s c + Q]          when 0 <= n - s c + Q < S     (_temp2mat, [T, C, N])
//   X[b, (t, k), n]  = x[b, t, c]                 when n - s c + Q == k         (_coef2mat, [B, T, S, N])
//
// LASSO (ista / acc_ista / fista, lasso.py:97-189,274-415) on the operator A without forming it.  In the
// reference's scaled variables x' = x rho (rho[t, c] = |A_(t,c)|, the boundary-truncated row norm) one
// iteration is
//   pass 1  r[b, n]    = y[b, n] - sum_(t, c) (v'[b, t, c] / rho[t, c]) D[t, n - s c + Q]          (= y - v'A')
//   pass 2  g[b, t, c] = (1 / rho[t, c]) sum_k r[b, s c - Q + k] conj(D[t, k])                    (= r A'^H)
//           x'_new     = prox(v' + g / L, alpha N / (rho L)),  momentum and the |dx'| - tol rho test fused in
// i.e. (y - v'A')A'^H in place of the reference's yA'^H - v'A'A'^H (the same quantity).  1/L is the
// Gershgorin bound of the banded Gram A'A'^H, built by the prepare kernels from the lag correlations
// Corr[t, t', m] = sum_k D[t, k] conj(D[t', k + m]): an entry whose column's support lies inside the signal
// IS Corr / (rho_i rho_j); only the boundary columns sum their truncated overlap explicitly.
//
// Dictionary statistics (template_matching.py:177-187) without X [B, T S, N]:
//   yX[t, k]                = sum_b sum_c x[b, t, c] y[b, s c - Q + k]                     (no conjugate)
//   XXt[(t, k), (t', k')]   = sum_b sum_(c in W(k, d)) x[b, t, c] conj(x[b, t', c + d]),  d = (k - k') / s
// (zero unless k = k' mod s).  The window W(k, d) of c keeps s c - Q + k inside [0, N); every W(k, d) holds
// the common core [cl(d), ch(d)], so an entry is  M[t, t', d] + head edge terms + tail edge terms  with the
// interior sum M computed once per lag and at most ~S/s edge terms per side: additions only, no prefix
// differences, fixed summation order everywhere (two runs are bitwise identical).
#pragma once
#include "abi.hpp"
#include "lasso_impl.hpp"

namespace dcp {

DCP_HD long tm_floor_div(long a, long b) { return (a >= 0) ? a / b : -((-a + b - 1) / b); }
DCP_HD long tm_ceil_div(long a, long b) { return -tm_floor_div(-a, b); }

struct TmGeom {
    long B = 1, T = 0, S = 0, N = 0, C = 0, s = 1, Q = 0;
    long dh = 0;   // largest |lag| in units of c: floor((S - 1) / s)
    long Ch = 1;   // channels of a template (D [T, Ch, S], y [B, Ch, N]): honoured by the greedy coders' kernels, the
                   // dictionary step on event lists (template_events.hpp) and the Gram-form LASSO (template_mc_lasso.hpp)
    DCP_HD long nd() const { return 2 * dh + 1; }
    // c of the coefficients whose taps cover sample n: [c_first(n), c_last(n)] (clipped to [0, C))
    DCP_HD long c_first(long n) const { long c = tm_ceil_div(n + Q - S + 1, s); return c < 0 ? 0 : c; }
    DCP_HD long c_last(long n) const { long c = tm_floor_div(n + Q, s); return c > C - 1 ? C - 1 : c; }
    // window of c for tap k and lag d:  0 <= s c - Q + k < N,  0 <= c < C,  0 <= c + d < C
    DCP_HD void window(long k, long d, long* lo, long* hi) const {
        long a = tm_ceil_div(Q - k, s), b = tm_floor_div(N - 1 + Q - k, s);
        if (a < 0) a = 0;
        if (a < -d) a = -d;
        if (b > C - 1) b = C - 1;
        if (b > C - 1 - d) b = C - 1 - d;
        *lo = a;
        *hi = b;
    }
    // core shared by every tap (intersection over k) and the union of all windows, for lag d.  An empty
    // core is reported as cl = hi(union) + 1, ch = hi(union): every term is then a head term.
    DCP_HD void core(long d, long* cl, long* ch, long* ul, long* uh) const {
        long l0, h0, l1, h1;
        window(0, d, &l0, &h0);
        window(S - 1, d, &l1, &h1);
        *ul = l1;   // lo(k) decreases with k, hi(k) too
        *uh = h0;
        *cl = l0;
        *ch = h1;
        if (*cl > *ch) { *cl = *uh + 1; *ch = *uh; }
    }
};

// reference _coef_size (template_matching.py:102-112); false when the geometry is out of scope
inline bool tm_geom(TmGeom& g, int64_t B, int64_t T, int64_t S, int64_t N, int64_t stride, int padding) {
    if (B <= 0 || T <= 0 || S <= 0 || N <= 0 || stride <= 0 || S > N) return false;
    if ((B | T | S | N) > 0x7fffffffLL) return false;
    const long pad = padding ? N - 1 : N - S;
    g.B = B; g.T = T; g.S = S; g.N = N; g.s = stride;
    g.C = tm_floor_div(S + 2 * pad - N, stride) + 1;
    if (g.C <= 0) return false;
    g.Q = stride * (g.C - 1) - pad;
    g.dh = (S - 1) / stride;
    return true;
}

// The shape arguments of a dcp_tm_* entry as its signature lists them; the dcp_tm_mc_* entries add Ch and set mc.
struct TmShape {
    int64_t B, T, S, N, stride;
    int padding;
    int64_t Ch = 1;
    bool mc = false;
};

// What every dcp_tm_* entry does first: the handle, the geometry of one channel, the device, then Ch.
inline int tm_geom_api(dcp_handle* h, const TmShape& sh, TmGeom& g) {
    if (!h) return DCP_ERR_INVALID;
    if (!tm_geom(g, sh.B, sh.T, sh.S, sh.N, sh.stride, sh.padding))
        return fail(h, DCP_ERR_INVALID, "template geometry: need 0 < S <= N, stride > 0, C > 0");
    DCP_HIP_OK(h, hipSetDevice(h->device));
    if (sh.Ch < 1 || sh.Ch > 0x7fffffffLL)
        return fail(h, DCP_ERR_INVALID, "multichannel templates: need 1 <= Ch < 2^31");
    g.Ch = sh.Ch;
    return DCP_OK;
}

template <class T>
DCP_HD T div_real(T v, real_t<T> d) {
    if constexpr (scalar_traits<T>::is_complex) return T{v.re / d, v.im / d};
    else return v / d;
}

// ---- dense helpers ------------------------------------------------------------------------------
// out[t, c, n] = A[(t, c), n]   (_temp2mat)
template <class T>
__global__ void __launch_bounds__(256) tm_temp2mat_kernel(const T* __restrict__ D, TmGeom g, T* __restrict__ out) {
    const long total = g.T * g.C * g.N;
    for (long i = blockIdx.x * 256L + threadIdx.x; i < total; i += (long)gridDim.x * 256L) {
        const long n = i % g.N, c = (i / g.N) % g.C, t = i / (g.N * g.C);
        const long k = n - g.s * c + g.Q;
        out[i] = (k >= 0 && k < g.S) ? D[t * g.S + k] : zero_of<T>();
    }
}

// out[b, t, k, n] = X[b, (t, k), n]   (_coef2mat)
template <class T>
__global__ void __launch_bounds__(256) tm_coef2mat_kernel(const T* __restrict__ x, TmGeom g, T* __restrict__ out) {
    const long total = g.B * g.T * g.S * g.N;
    for (long i = blockIdx.x * 256L + threadIdx.x; i < total; i += (long)gridDim.x * 256L) {
        const long n = i % g.N, k = (i / g.N) % g.S, bt = i / (g.N * g.S);
        const long num = n - k + g.Q;   // = s c
        T v = zero_of<T>();
        if (num >= 0 && num % g.s == 0 && num / g.s < g.C) v = x[bt * g.C + num / g.s];
        out[i] = v;
    }
}

// ---- pass 1: r = y - v A'  (y == nullptr: r = x A, i.e. predict) ----------------------------------
// One workgroup per 256 samples of one signal.  Per template, D[t, :] and the coefficients whose taps reach
// the tile (the tile plus an S-wide halo, in units of c) are staged in LDS; lds_ok == 0 (a template too long
// for LDS) reads them from global memory through the same (flat) pointers.
template <class T>
__global__ void __launch_bounds__(256) tm_residual_kernel(const T* __restrict__ y, const T* __restrict__ v,
                                                          const real_t<T>* __restrict__ rinv,
                                                          const T* __restrict__ D, TmGeom g, int lds_ok,
                                                          T* __restrict__ r) {
    extern __shared__ __attribute__((aligned(16))) char tm_smem[];
    T* sD = reinterpret_cast<T*>(tm_smem);
    const long b = blockIdx.y;
    const long n0 = (long)blockIdx.x * 256;
    const long n = n0 + threadIdx.x;
    const long n1 = (n0 + 255 < g.N - 1) ? n0 + 255 : g.N - 1;
    const long clo = g.c_first(n0), chi = g.c_last(n1);
    T* sU = sD + g.S;
    T acc = zero_of<T>();
    for (long t = 0; t < g.T; ++t) {
        const T* dsrc = D + t * g.S;
        const T* vrow = v + (b * g.T + t) * g.C;
        // usrc[c - uoff] = v[b, t, c] (/ rho[t, c] when staged).  The offset stays an index: a pointer rebased below
        // the start of LDS wraps in the 32-bit LDS address space and leaves the aperture once it is used as flat.
        const T* usrc;
        long uoff = 0;
        if (lds_ok) {
            __syncthreads();
            for (long k = threadIdx.x; k < g.S; k += 256) sD[k] = dsrc[k];
            for (long c = clo + threadIdx.x; c <= chi; c += 256) {
                T u = vrow[c];
                if (rinv != nullptr) u = scale(u, rinv[t * g.C + c]);
                sU[c - clo] = u;
            }
            __syncthreads();
            dsrc = sD;
            usrc = sU;
            uoff = clo;
        } else {
            usrc = vrow;
        }
        if (n < g.N) {
            const long c1 = g.c_last(n);
            for (long c = g.c_first(n); c <= c1; ++c) {
                T u = usrc[c - uoff];
                if (!lds_ok && rinv != nullptr) u = scale(u, rinv[t * g.C + c]);
                acc = madd(acc, u, dsrc[n - g.s * c + g.Q]);
            }
        }
    }
    if (n < g.N) r[b * g.N + n] = (y != nullptr) ? sub(y[b * g.N + n], acc) : acc;
}

// ---- pass 2: g = r A'^H with the proximal step in the epilogue -------------------------------------
// One workgroup per 256 coefficients of one (signal, template); the samples they read (the tile's span plus
// the S-wide halo) and conj(D[t, :]) are staged in LDS when they fit.
template <class T, int PROX>
struct TmStep {
    const T* V;          // the point fed to the step (v')
    const T* P;          // the iterate the stop test compares with (x0')
    T* Nw;               // x0'_new
    T* Vn;               // next v' (momentum), nullable
    const real_t<T>* rinv;
    const real_t<T>* alphak;   // alpha N / rho
    const real_t<T>* tolk;     // tol rho
    const real_t<T>* scal;     // scal[0] = 1 / L
    real_t<T> coef;
    int check;
    int* flag;
};

// (r A^H)[b, t, c] for c = 256 blockIdx.x + threadIdx.x, unscaled; zero where c >= C.  The whole workgroup calls it
// (the staging has a barrier).
template <class T>
__device__ __forceinline__ T tm_corr_tile(const T* __restrict__ r, const T* __restrict__ D, const TmGeom& g,
                                          int lds_ok, long t, long b, long c) {
    extern __shared__ __attribute__((aligned(16))) char tm_smem[];
    T* sD = reinterpret_cast<T*>(tm_smem);
    T* sR = sD + g.S;
    const long c0 = (long)blockIdx.x * 256;
    const long c1 = (c0 + 255 < g.C - 1) ? c0 + 255 : g.C - 1;
    long nlo = g.s * c0 - g.Q, nhi = g.s * c1 - g.Q + g.S - 1;
    if (nlo < 0) nlo = 0;
    if (nhi > g.N - 1) nhi = g.N - 1;
    const T* rrow = r + b * g.N;
    const T* dsrc = D + t * g.S;
    const T* rsrc = rrow;   // rsrc[n - roff] = r[b, n] (an index offset, as in tm_residual_kernel)
    long roff = 0;
    if (lds_ok) {
        for (long k = threadIdx.x; k < g.S; k += 256) sD[k] = conj_of(dsrc[k]);
        for (long m = nlo + threadIdx.x; m <= nhi; m += 256) sR[m - nlo] = rrow[m];
        __syncthreads();
        rsrc = sR;
        roff = nlo;
    }
    T acc = zero_of<T>();
    if (c >= g.C) return acc;
    const long base = g.s * c - g.Q;
    long k0 = -base, k1 = g.N - 1 - base;
    if (k0 < 0) k0 = 0;
    if (k1 > g.S - 1) k1 = g.S - 1;
    for (long k = k0; k <= k1; ++k) acc = madd(acc, rsrc[base + k - roff], lds_ok ? sD[k] : conj_of(dsrc[k]));
    return acc;
}

// The proximal step on coefficient (b, t, c < C) from its unscaled gradient grad = (r A^H)[b, t, c]:
//   z = V + grad rinv / L,  x_new = prox(z, alpha_k / L),  the stop test against P,  the momentum point.
// The one place that reads and writes the fields of TmStep (this kernel and the Gram-form step of
// template_mc_lasso.hpp end in it).
template <class T, int PROX>
__device__ __forceinline__ void tm_step_epilogue(const TmStep<T, PROX>& ep, const TmGeom& g, T grad, long t, long b,
                                                 long c) {
    typedef real_t<T> R;
    const long tc = t * g.C + c;
    const long i = (b * g.T + t) * g.C + c;
    const R Linv = ep.scal[0];
    const T z = add(ep.V[i], scale(scale(grad, ep.rinv[tc]), Linv));
    const T xn = prox_apply<PROX>(z, Linv * ep.alphak[tc]);
    const T d = sub(xn, ep.P[i]);
    if (ep.check && !((absval(d) - ep.tolk[tc]) < R(0))) *ep.flag = 1;
    ep.Nw[i] = xn;
    if (ep.Vn != nullptr) ep.Vn[i] = add(xn, scale(d, ep.coef));
}

template <class T, int PROX>
__global__ void __launch_bounds__(256) tm_corr_step_kernel(const T* __restrict__ r, const T* __restrict__ D,
                                                           TmGeom g, int lds_ok, TmStep<T, PROX> ep) {
    const long t = blockIdx.y, b = blockIdx.z;
    const long c = (long)blockIdx.x * 256 + threadIdx.x;
    const T acc = tm_corr_tile(r, D, g, lds_ok, t, b, c);
    if (c >= g.C) return;
    tm_step_epilogue(ep, g, acc, t, b, c);
}

// ---- prepare ------------------------------------------------------------------------------------
// |A_(t,c)|^2 over its taps inside [0, N), over the g.Ch channels of D [T, Ch, S] (ch ascending, k ascending inside)
template <class T>
__device__ __forceinline__ real_t<T> tm_row_norm2(const T* __restrict__ D, const TmGeom& g, long t, long c) {
    const long base = g.s * c - g.Q;
    long k0 = -base, k1 = g.N - 1 - base;
    if (k0 < 0) k0 = 0;
    if (k1 > g.S - 1) k1 = g.S - 1;
    real_t<T> acc = 0;
    for (long ch = 0; ch < g.Ch; ++ch)
        for (long k = k0; k <= k1; ++k) acc += abs2(D[(t * g.Ch + ch) * g.S + k]);
    return acc;
}

// rho[t, c] = |A_(t,c)| over its taps inside [0, N); alpha_k = (alpha / rho) N; tol_k = tol rho; clears the flag
template <class T>
__global__ void __launch_bounds__(256) tm_rownorm_kernel(const T* __restrict__ D, TmGeom g, real_t<T> alpha,
                                                         real_t<T> tol, real_t<T>* __restrict__ rho,
                                                         real_t<T>* __restrict__ rinv, real_t<T>* __restrict__ alphak,
                                                         real_t<T>* __restrict__ tolk, int* __restrict__ flag) {
    typedef real_t<T> R;
    if (blockIdx.x == 0 && threadIdx.x == 0) *flag = 0;
    for (long i = blockIdx.x * 256L + threadIdx.x; i < g.T * g.C; i += (long)gridDim.x * 256L) {
        const R nr = sqrt(tm_row_norm2(D, g, i / g.C, i % g.C));
        rho[i] = nr;
        rinv[i] = R(1) / nr;
        alphak[i] = (alpha / nr) * R(g.N);
        tolk[i] = tol * nr;
    }
}

// out[i] = x[i] * rho[tc]  (mul) or x[i] / rho[tc]
template <class T>
__global__ void __launch_bounds__(256) tm_scale_kernel(const T* __restrict__ x, const real_t<T>* __restrict__ rho,
                                                       long total, long TC, int mul, T* __restrict__ out) {
    for (long i = blockIdx.x * 256L + threadIdx.x; i < total; i += (long)gridDim.x * 256L) {
        const real_t<T> s = rho[i % TC];
        out[i] = mul ? scale(x[i], s) : div_real(x[i], s);
    }
}

// corr[(t * T + t') * (2S - 1) + m + S - 1] = sum_ch sum_k D[t, ch, k] conj(D[t', ch, k + m]) over the g.Ch channels
// of D [T, Ch, S] (ch ascending, k ascending inside)
template <class T>
__global__ void __launch_bounds__(256) tm_lagcorr_kernel(const T* __restrict__ D, TmGeom g, T* __restrict__ corr) {
    const long t = blockIdx.x / g.T, tp = blockIdx.x % g.T;
    const long W = 2 * g.S - 1;
    for (long j = threadIdx.x; j < W; j += 256) {
        const long m = j - (g.S - 1);
        const long k0 = m < 0 ? -m : 0, k1 = m > 0 ? g.S - 1 - m : g.S - 1;
        T acc = zero_of<T>();
        for (long ch = 0; ch < g.Ch; ++ch)
            for (long k = k0; k <= k1; ++k)
                acc = madd(acc, D[(t * g.Ch + ch) * g.S + k], conj_of(D[(tp * g.Ch + ch) * g.S + k + m]));
        corr[blockIdx.x * W + j] = acc;
    }
}

// Columns j = (t', c') with c' in [lo, hi] are Toeplitz: every row c within dh of c' exists and has all its taps
// inside the signal, so their entries are Corr / (|D_t| |D_t'|) (rho of a full row is the same number, bit for bit,
// for every c) and their column sum depends on t' alone.  lo > hi: no such column.
DCP_HD void tm_toeplitz_cols(const TmGeom& g, long* lo, long* hi) {
    long a = tm_ceil_div(g.Q, g.s), b = tm_floor_div(g.N - g.S + g.Q, g.s);   // rows with every tap inside
    if (a < 0) a = 0;
    if (b > g.C - 1) b = g.C - 1;
    *lo = a + g.dh;
    *hi = b - g.dh;
}

// One workgroup per column j = (t', c'):  sum_i |(A'A'^H)[i, j]|  (eigen.py:20 on the banded Gram), the band's
// (t, c) split over the threads and summed by a fixed-order tree.
//   mode 0: block t' sums the representative Toeplitz column (t', lo) into tsum[t'];
//   mode 1: block number e of template t' sums its e-th non-Toeplitz column (c' < lo, then c' > hi) into colsum.
template <class T>
__global__ void __launch_bounds__(256) tm_gram_colsum_kernel(const T* __restrict__ D, const T* __restrict__ corr,
                                                             const real_t<T>* __restrict__ rinv, TmGeom g, long lo,
                                                             long hi, int mode, real_t<T>* __restrict__ tsum,
                                                             real_t<T>* __restrict__ colsum) {
    typedef real_t<T> R;
    __shared__ R sh[4];
    const long W = 2 * g.S - 1;
    long tp, cp;
    if (mode == 0) {
        tp = blockIdx.x;
        cp = lo;
    } else {
        const long nb = lo <= hi ? g.C - (hi - lo + 1) : g.C;
        tp = blockIdx.x / nb;
        const long e = blockIdx.x % nb;
        cp = (lo <= hi && e >= lo) ? hi + 1 + (e - lo) : e;
    }
    const long j = tp * g.C + cp;
    const long bj = g.s * cp - g.Q;                  // first sample of column j's taps
    const bool inside = bj >= 0 && bj + g.S - 1 <= g.N - 1;
    long ca = cp - g.dh, cb = cp + g.dh;
    if (ca < 0) ca = 0;
    if (cb > g.C - 1) cb = g.C - 1;
    const long nc = cb - ca + 1;
    R acc = 0;
    for (long q = threadIdx.x; q < g.T * nc; q += 256) {
        const long t = q / nc, c = ca + q % nc;
        const long m = g.s * (c - cp);               // G_ij = sum_k D[t, k] conj(D[t', k + m]) over n inside
        T v;
        if (inside) {
            v = corr[(t * g.T + tp) * W + m + g.S - 1];
        } else {
            const long bi = g.s * c - g.Q;
            long k0 = m < 0 ? -m : 0, k1 = m > 0 ? g.S - 1 - m : g.S - 1;
            if (k0 < -bi) k0 = -bi;
            if (k1 > g.N - 1 - bi) k1 = g.N - 1 - bi;
            v = zero_of<T>();
            for (long ch = 0; ch < g.Ch; ++ch)   // (D [T, Ch, S]: ch ascending, k ascending inside)
                for (long k = k0; k <= k1; ++k)
                    v = madd(v, D[(t * g.Ch + ch) * g.S + k], conj_of(D[(tp * g.Ch + ch) * g.S + k + m]));
        }
        acc += absval(v) * rinv[t * g.C + c] * rinv[j];
    }
    const R tot = block_sum_256(acc, sh);
    if (threadIdx.x == 0) {
        if (mode == 0) tsum[tp] = tot;
        else colsum[j] = tot;
    }
}

// colsum[(t', c')] = tsum[t'] for the Toeplitz columns c' in [lo, hi]
template <class R>
__global__ void __launch_bounds__(256) tm_gram_fill_kernel(TmGeom g, long lo, long hi, const R* __restrict__ tsum,
                                                           R* __restrict__ colsum) {
    const long w = hi - lo + 1;
    for (long i = blockIdx.x * 256L + threadIdx.x; i < g.T * w; i += (long)gridDim.x * 256L)
        colsum[(i / w) * g.C + lo + i % w] = tsum[i / w];
}

// scal[0] = 1 / max(v) (+ jitter on the max: scal[1] = max + jitter)   (one workgroup, fixed order)
template <class R>
struct FinInvMax {
    R jitter;
    R* scal;
    __device__ __forceinline__ void operator()(R m) const {
        scal[0] = R(1) / (m + jitter);
        scal[1] = m + jitter;
    }
};
template <class R>
inline void launch_tm_max(hipStream_t st, const R* v, long n, R jitter, R* scal) {
    hipLaunchKernelGGL((reduce_vector_kernel<MaxOp, R, FinInvMax<R>>), dim3(1), dim3(256), 0, st, v, n,
                       FinInvMax<R>{jitter, scal});
}

// ---- dictionary statistics ----------------------------------------------------------------------
// acc + a b for the statistics' partial sums, with the complex product spelled out:
//   re = fma(a.re, b.re, -(a.im b.im)),   im = fma(a.im, b.re, a.re b.im).
// Left as madd's plain expression, which of the two products of a part gets fused into the other is the compiler's
// choice and differs from kernel to kernel; kernels that must agree bit for bit on the same sum (the dense ones here
// and those of template_events.hpp) take their terms from this one spelling.
template <class T>
DCP_HD T tm_stat_madd(T acc, T a, T b) {
    if constexpr (scalar_traits<T>::is_complex) {
        typedef real_t<T> R;
        const R re = madd(R(-(a.im * b.im)), a.re, b.re);
        const R im = madd(R(a.re * b.im), a.im, b.re);
        return T{acc.re + re, acc.im + im};
    } else {
        return madd(acc, a, b);
    }
}

// mpart[((b T + t) T + t') nd + (d + dh)] = sum_(c in core(d)) x[b, t, c] conj(x[b, t', c + d])
template <class T>
__global__ void __launch_bounds__(256) tm_stats_core_kernel(const T* __restrict__ x, TmGeom g, T* __restrict__ mpart) {
    const long tp = blockIdx.x, t = blockIdx.y, b = blockIdx.z;
    const T* xa = x + (b * g.T + t) * g.C;
    const T* xb = x + (b * g.T + tp) * g.C;
    const long nd = g.nd();
    for (long j = threadIdx.x; j < nd; j += 256) {
        const long d = j - g.dh;
        long cl, ch, ul, uh;
        g.core(d, &cl, &ch, &ul, &uh);
        T acc = zero_of<T>();
        for (long c = cl; c <= ch; ++c) acc = tm_stat_madd(acc, xa[c], conj_of(xb[c + d]));
        mpart[((b * g.T + t) * g.T + tp) * nd + j] = acc;
    }
}

// Edge terms, summed over the batch in order:  eh[.., e] at c = cl - 1 - e,  et[.., e] at c = ch + 1 + e.
// Grid (T, T, blocks of 256 cells (side, lag, e)): a thread sums one cell over the batch, one signal after the other.
template <class T>
__global__ void __launch_bounds__(256) tm_stats_edge_kernel(const T* __restrict__ x, TmGeom g, long hmax,
                                                            T* __restrict__ eh, T* __restrict__ et) {
    const long tp = blockIdx.x, t = blockIdx.y;
    const long nd = g.nd();
    for (long q = blockIdx.z * 256L + threadIdx.x; q < nd * hmax * 2; q += (long)gridDim.z * 256L) {
        const long side = q / (nd * hmax), j = (q / hmax) % nd, e = q % hmax;
        const long d = j - g.dh;
        long cl, ch, ul, uh;
        g.core(d, &cl, &ch, &ul, &uh);
        const long c = side == 0 ? cl - 1 - e : ch + 1 + e;
        T acc = zero_of<T>();
        if (side == 0 ? (c >= ul) : (c <= uh)) {
            for (long b = 0; b < g.B; ++b)
                acc = madd(acc, x[(b * g.T + t) * g.C + c], conj_of(x[(b * g.T + tp) * g.C + c + d]));
        }
        T* dst = side == 0 ? eh : et;
        dst[((t * g.T + tp) * nd + j) * hmax + e] = acc;
    }
}

// yxpart[(b T + t) S + k] = sum_c x[b, t, c] y[b, s c - Q + k]
template <class T>
__global__ void __launch_bounds__(256) tm_stats_yx_kernel(const T* __restrict__ y, const T* __restrict__ x, TmGeom g,
                                                          T* __restrict__ yxpart) {
    const long t = blockIdx.x, b = blockIdx.y;
    for (long k = threadIdx.x; k < g.S; k += 256) {
        long lo, hi;
        g.window(k, 0, &lo, &hi);
        T acc = zero_of<T>();
        for (long c = lo; c <= hi; ++c)
            acc = tm_stat_madd(acc, x[(b * g.T + t) * g.C + c], y[b * g.N + g.s * c - g.Q + k]);
        yxpart[(b * g.T + t) * g.S + k] = acc;
    }
}

// out[i] = sum_b part[b n + i], b ascending from +0: written (acc_it == 0) or added as sum / acc_it.  One thread per
// cell i, so the reads of a signal's n partial sums coalesce.
template <class T>
__global__ void __launch_bounds__(256) tm_batch_sum_kernel(const T* __restrict__ part, long B, long n, int acc_it,
                                                           T* __restrict__ out) {
    typedef real_t<T> R;
    for (long i = blockIdx.x * 256L + threadIdx.x; i < n; i += (long)gridDim.x * 256L) {
        T s = zero_of<T>();
        for (long b = 0; b < B; ++b) s = add(s, part[b * n + i]);
        out[i] = acc_it ? add(out[i], div_real(s, R(acc_it))) : s;
    }
}

// One workgroup per row i = (t, k):  XXt[i, :], written (acc_it == 0) or added as stat / acc_it.  msum [T, T, nd] is
// mpart summed over the batch (tm_batch_sum_kernel): the S pairs (k, k') of a lag share one number.
template <class T>
__global__ void __launch_bounds__(256) tm_stats_assemble_kernel(const T* __restrict__ msum, const T* __restrict__ eh,
                                                                const T* __restrict__ et, TmGeom g, long hmax,
                                                                int acc_it, T* __restrict__ XXt) {
    typedef real_t<T> R;
    const long t = blockIdx.x / g.S, k = blockIdx.x % g.S;
    const long TS = g.T * g.S, nd = g.nd();
    for (long jcol = threadIdx.x; jcol < TS; jcol += 256) {
        const long tp = jcol / g.S, kp = jcol % g.S;
        T val = zero_of<T>();
        if ((k - kp) % g.s == 0) {
            const long d = (k - kp) / g.s, j = d + g.dh;
            long lo, hi, cl, ch, ul, uh;
            g.window(k, d, &lo, &hi);
            g.core(d, &cl, &ch, &ul, &uh);
            if (lo <= hi) {
                const long base = (t * g.T + tp) * nd + j;
                const long hend = hi < cl - 1 ? hi : cl - 1;
                for (long c = lo; c <= hend; ++c) val = add(val, eh[base * hmax + (cl - 1 - c)]);
                if (cl <= ch && lo <= cl && hi >= ch) val = add(val, msum[base]);
                const long tbeg = lo > ch + 1 ? lo : ch + 1;
                for (long c = tbeg; c <= hi; ++c) val = add(val, et[base * hmax + (c - ch - 1)]);
            }
        }
        const long o = blockIdx.x * TS + jcol;
        XXt[o] = acc_it ? add(XXt[o], div_real(val, R(acc_it))) : val;
    }
}

// ---- D update -------------------------------------------------------------------------------------
// One workgroup per index j = (t, k) of the n = T S rows of XXt and channel ch = blockIdx.y of D [T, Ch, S]:
//   colabs[j] = sum_i |XXt[i, j]|  (XXt has no channels: every workgroup forms it, channel 0's stores it),
//   step[t, ch, k] = yX[t, ch, k] - sum_(i = (t', k')) XXt[j, i] D[t', ch, k']
template <class T>
__global__ void __launch_bounds__(256) tm_dupdate_rows_kernel(const T* __restrict__ XXt, const T* __restrict__ yX,
                                                              const T* __restrict__ D, long n, long S, long Ch,
                                                              real_t<T>* __restrict__ colabs, T* __restrict__ step) {
    typedef real_t<T> R;
    __shared__ R sh[4];
    const long j = blockIdx.x, ch = blockIdx.y;
    R ca = 0, re = 0, im = 0;
    for (long i = threadIdx.x; i < n; i += 256) {
        ca += absval(XXt[i * n + j]);
        const T p = mul(XXt[j * n + i], D[((i / S) * Ch + ch) * S + i % S]);
        re += real_part(p);
        im += imag_part(p);
    }
    const R tca = block_sum_256(ca, sh);
    const T dot = block_sum_256_parts<T>(re, im, sh);
    if (threadIdx.x == 0) {
        if (ch == 0) colabs[j] = tca;
        const long o = ((j / S) * Ch + ch) * S + j % S;
        step[o] = sub(yX[o], dot);
    }
}

// U = D + step / L  with L = scal[1]
template <class T>
__global__ void __launch_bounds__(256) tm_dupdate_apply_kernel(const T* __restrict__ D, const T* __restrict__ step,
                                                               const real_t<T>* __restrict__ scal, long n,
                                                               T* __restrict__ U) {
    for (long i = blockIdx.x * 256L + threadIdx.x; i < n; i += (long)gridDim.x * 256L)
        U[i] = add(D[i], div_real(step[i], scal[1]));
}

// ---- minibatch windows (template_matching.py:219-253) ---------------------------------------------
// yw[j, ch, n] = y[ib[j], ch, in[j] + n] (y [B, Ch, N]; Ch = 1: y [B, N]);  xw[j, t, c] = x[ib[j], t, in[j] + c]
template <class T>
__global__ void __launch_bounds__(256) tm_gather_kernel(const T* __restrict__ y, const T* __restrict__ x,
                                                        const int64_t* __restrict__ ib, const int64_t* __restrict__ in,
                                                        long m, long Ch, long N, long T_, long C, long w, long cw,
                                                        T* __restrict__ yw, T* __restrict__ xw) {
    const long ny = m * Ch * w, nx = m * T_ * cw;
    for (long i = blockIdx.x * 256L + threadIdx.x; i < ny + nx; i += (long)gridDim.x * 256L) {
        if (i < ny) {
            const long j = i / (Ch * w), ch = (i / w) % Ch, n = i % w;
            yw[i] = y[(ib[j] * Ch + ch) * N + in[j] + n];
        } else {
            const long q = i - ny;
            const long j = q / (T_ * cw), t = (q / cw) % T_, c = q % cw;
            xw[q] = x[(ib[j] * T_ + t) * C + in[j] + c];
        }
    }
}

// x[ib[j], t, in[j] + c] = xw[j, t, c], the last window that covers an element wins (sequential write-back)
template <class T>
__global__ void __launch_bounds__(256) tm_scatter_kernel(const T* __restrict__ xw, const int64_t* __restrict__ ib,
                                                         const int64_t* __restrict__ in, long m, long T_, long C,
                                                         long cw, T* __restrict__ x) {
    const long nx = m * T_ * cw;
    for (long q = blockIdx.x * 256L + threadIdx.x; q < nx; q += (long)gridDim.x * 256L) {
        const long j = q / (T_ * cw), t = (q / cw) % T_, c = q % cw;
        const long b = ib[j], pos = in[j] + c;
        bool later = false;
        for (long jj = j + 1; jj < m && !later; ++jj) later = ib[jj] == b && in[jj] <= pos && pos < in[jj] + cw;
        if (!later) x[(b * T_ + t) * C + pos] = xw[q];
    }
}

// =================================================================================================
// Host side
// =================================================================================================
constexpr size_t kTmLdsBytes = 48 * 1024;

inline int tm_grid(long n) {
    long g = (n + 255) / 256;
    if (g > 65536) g = 65536;
    return (int)(g < 1 ? 1 : g);
}

template <class T>
inline int tm_launch_residual(dcp_handle* h, const T* y, const T* v, const real_t<T>* rinv, const T* D,
                              const TmGeom& g, T* r) {
    const long span = (255 + g.S - 1) / g.s + 2;
    size_t bytes = (size_t)(g.S + span) * sizeof(T);
    const int lds_ok = bytes <= kTmLdsBytes;
    if (!lds_ok) bytes = 0;
    hipLaunchKernelGGL((tm_residual_kernel<T>), dim3((g.N + 255) / 256, g.B), dim3(256), bytes, h->stream, y, v,
                       rinv, D, g, lds_ok, r);
    DCP_LAUNCH_OK(h, hipGetLastError());
    return DCP_OK;
}

template <class T, int PROX>
inline int tm_launch_step(dcp_handle* h, const T* r, const T* D, const TmGeom& g, const TmStep<T, PROX>& ep) {
    const long span = 255 * g.s + g.S;
    size_t bytes = (size_t)(g.S + span) * sizeof(T);
    const int lds_ok = bytes <= kTmLdsBytes;
    if (!lds_ok) bytes = 0;
    hipLaunchKernelGGL((tm_corr_step_kernel<T, PROX>), dim3((g.C + 255) / 256, g.T, g.B), dim3(256), bytes,
                       h->stream, r, D, g, lds_ok, ep);
    DCP_LAUNCH_OK(h, hipGetLastError());
    return DCP_OK;
}

// scal[0] = 1 / Gershgorin(A'A'^H) from the lag correlations and 1 / rho (over the g.Ch channels of D): the Toeplitz
// columns once per template, the boundary columns one by one.  tsum [T] and colsum [T C] are workspace.
template <class T>
inline int tm_gram_bound(dcp_handle* h, const T* D, const T* corr, const real_t<T>* rinv, const TmGeom& g,
                         real_t<T>* tsum, real_t<T>* colsum, real_t<T>* scal) {
    typedef real_t<T> R;
    hipStream_t st = h->stream;
    long lo, hi;
    tm_toeplitz_cols(g, &lo, &hi);
    if (lo <= hi) {
        hipLaunchKernelGGL((tm_gram_colsum_kernel<T>), dim3(g.T), dim3(256), 0, st, D, corr, rinv, g, lo, hi, 0, tsum,
                           colsum);
        DCP_LAUNCH_OK(h, hipGetLastError());
        hipLaunchKernelGGL((tm_gram_fill_kernel<R>), dim3(tm_grid(g.T * (hi - lo + 1))), dim3(256), 0, st, g, lo, hi,
                           (const R*)tsum, colsum);
        DCP_LAUNCH_OK(h, hipGetLastError());
    }
    const long nb = lo <= hi ? g.C - (hi - lo + 1) : g.C;
    if (nb > 0) {
        hipLaunchKernelGGL((tm_gram_colsum_kernel<T>), dim3(g.T * nb), dim3(256), 0, st, D, corr, rinv, g, lo, hi, 1,
                           tsum, colsum);
        DCP_LAUNCH_OK(h, hipGetLastError());
    }
    launch_tm_max<R>(st, (const R*)colsum, g.T * g.C, R(0), scal);
    DCP_LAUNCH_OK(h, hipGetLastError());
    return DCP_OK;
}

// Structured solve_fastpath for ista / acc_ista / fista (+ _pos).  Y [B, N], D [T, S], X [B, T, C]
// (in: initial estimate, out: solution).  The outer loop and its lagged stop test are prox_gradient_loop
// (prox_loop.hpp), shared with the dense solver.
template <class T, int PROX>
inline int tm_lasso_solve(dcp_handle* h, const T* Y, const T* D, T* X, const TmGeom& g, real_t<T> alpha,
                          real_t<T> tol, int maxiter, int method, int* it_out) {
    typedef real_t<T> R;
    hipStream_t st = h->stream;
    const long TC = g.T * g.C, BX = g.B * TC;
    R *rho = nullptr, *rinv = nullptr, *alphak = nullptr, *tolk = nullptr, *colsum = nullptr;
    R* tsum = nullptr;   // Toeplitz column sums
    T* corr = nullptr;   // lag correlations
    R* scal = nullptr;
    int* flag = nullptr;
    T* r = nullptr;      // residual
    T* xb[4] = {nullptr, nullptr, nullptr, nullptr};   // iterates
    DCP_TRY(ws_lay_out(h, [&](WsLayout& a) {
        a.take(rho, TC);
        a.take(rinv, TC);
        a.take(alphak, TC);
        a.take(tolk, TC);
        a.take(colsum, TC);
        a.take(tsum, g.T);
        a.take(corr, g.T * g.T * (2 * g.S - 1));
        a.take(scal, 4);
        a.take(flag, 4);
        a.take(r, g.B * g.N);
        for (int q = 0; q < 4; ++q) a.take(xb[q], BX);
    }));
    void* hostv = nullptr;
    DCP_TRY(host_scratch(h, 64, &hostv));
    int* host_flag = reinterpret_cast<int*>(hostv);

    // ---- prepare: row norms, scaled alpha / tol, x' = x rho, 1 / Gershgorin(A'A'^H) ----
    hipLaunchKernelGGL((tm_rownorm_kernel<T>), dim3(tm_grid(TC)), dim3(256), 0, st, D, g, alpha, tol, rho, rinv,
                       alphak, tolk, flag);
    DCP_LAUNCH_OK(h, hipGetLastError());
    hipLaunchKernelGGL((tm_scale_kernel<T>), dim3(tm_grid(BX)), dim3(256), 0, st, (const T*)X, (const R*)rho, BX, TC,
                       1, xb[0]);
    DCP_LAUNCH_OK(h, hipGetLastError());
    hipLaunchKernelGGL((tm_lagcorr_kernel<T>), dim3(g.T * g.T), dim3(256), 0, st, D, g, corr);
    DCP_LAUNCH_OK(h, hipGetLastError());
    DCP_TRY(tm_gram_bound<T>(h, D, corr, rinv, g, tsum, colsum, scal));

    // ---- one iteration: the residual of V, then correlation + prox step into Nw (and Vn) ----
    auto step = [&](int, T* V, T* P, T* Nw, T* Vn, R coef, int check, bool) -> int {
        DCP_TRY(tm_launch_residual<T>(h, Y, V, rinv, D, g, r));
        TmStep<T, PROX> ep{V, P, Nw, Vn, rinv, alphak, tolk, scal, coef, check, flag};
        return tm_launch_step<T, PROX>(h, r, D, g, ep);
    };
    ProxLoopResult<T> res;
    DCP_TRY(prox_gradient_loop<T>(h, xb, method, maxiter, flag, host_flag, step, &res));
    hipLaunchKernelGGL((tm_scale_kernel<T>), dim3(tm_grid(BX)), dim3(256), 0, st, (const T*)res.result, (const R*)rho,
                       BX, TC, 0, X);
    DCP_LAUNCH_OK(h, hipGetLastError());
    DCP_HIP_OK(h, hipStreamSynchronize(st));
    *it_out = res.it;
    return DCP_OK;
}

inline long tm_hmax(const TmGeom& g) {
    long hm = 1;
    for (long d = -g.dh; d <= g.dh; ++d) {
        long cl, ch, ul, uh;
        g.core(d, &cl, &ch, &ul, &uh);
        if (cl - ul > hm) hm = cl - ul;
        if (uh - ch > hm) hm = uh - ch;
    }
    return hm;
}

// The workspace of a dictionary step: the partial statistics and the D update's vectors.
template <class T>
struct TmDstepWs {
    T *mpart = nullptr, *msum = nullptr, *eh = nullptr, *et = nullptr, *yxpart = nullptr, *step = nullptr, *U = nullptr,
      *Dn = nullptr;
    real_t<T>*colabs = nullptr, *rowmax = nullptr, *scal = nullptr;
};

template <class T>
inline void tm_dstep_layout(WsLayout& a, TmDstepWs<T>& w, const TmGeom& g, long hmax) {
    const long nd = g.nd(), TS = g.T * g.S, nD = TS * g.Ch;
    a.take(w.mpart, g.B * g.T * g.T * nd);
    a.take(w.msum, g.T * g.T * nd);
    a.take(w.eh, g.T * g.T * nd * hmax);
    a.take(w.et, g.T * g.T * nd * hmax);
    a.take(w.yxpart, g.B * nD);
    a.take(w.colabs, TS);
    a.take(w.step, nD);
    a.take(w.U, nD);
    a.take(w.Dn, nD);
    a.take(w.rowmax, g.T);
    a.take(w.scal, 4);
}

// A dictionary step around its partial sums: `partials()` enqueues whatever fills mpart and yxpart; then their sums
// over the batch (msum, and yX: written, or added as stat / acc_it to the running sum), the edge terms, the assembly of
// XXt (likewise), the D update D <- l2(D + (yX - XXt D) / (Gershgorin(XXt) + 1e-15)) and the step's one
// synchronisation; *maxdiff = max |D - D_new|.  With g.Ch channels D, yX and yxpart's rows are [T, Ch, S], the product
// XXt D is taken channel by channel (XXt [T S, T S] and its Gershgorin bound are those of one channel: x is shared)
// and a template is normalised over its Ch S entries.
// Timed under DCP_PROF_STATS up to the assembly, the partial sums alone under DCP_PROF_MISC as well.
template <class T, class Partials>
inline int tm_dstep_around(dcp_handle* h, const TmDstepWs<T>& w, const T* X, T* D, T* XXt, T* yX, const TmGeom& g,
                           long hmax, int acc_it, double* maxdiff, Partials&& partials) {
    typedef real_t<T> R;
    hipStream_t st = h->stream;
    const long TS = g.T * g.S, nM = g.T * g.T * g.nd(), F = g.Ch * g.S, nD = g.T * F;
    if (g.Ch > 65535) return fail(h, DCP_ERR_INVALID, "dictionary step: more than 65535 channels");
    {
        ProfScope ps(h, DCP_PROF_STATS);
        {
            ProfScope pp(h, DCP_PROF_MISC);
            DCP_TRY(partials());
        }
        hipLaunchKernelGGL((tm_batch_sum_kernel<T>), dim3(tm_grid(nM)), dim3(256), 0, st, (const T*)w.mpart, g.B, nM,
                           0, w.msum);
        DCP_LAUNCH_OK(h, hipGetLastError());
        hipLaunchKernelGGL((tm_batch_sum_kernel<T>), dim3(tm_grid(nD)), dim3(256), 0, st, (const T*)w.yxpart, g.B, nD,
                           acc_it, yX);
        DCP_LAUNCH_OK(h, hipGetLastError());
        const int eblocks = tm_grid(g.nd() * hmax * 2);
        hipLaunchKernelGGL((tm_stats_edge_kernel<T>), dim3(g.T, g.T, eblocks < 65535 ? eblocks : 65535), dim3(256),
                           0, st, X, g, hmax, w.eh, w.et);
        DCP_LAUNCH_OK(h, hipGetLastError());
        hipLaunchKernelGGL((tm_stats_assemble_kernel<T>), dim3(TS), dim3(256), 0, st, (const T*)w.msum,
                           (const T*)w.eh, (const T*)w.et, g, hmax, acc_it, XXt);
        DCP_LAUNCH_OK(h, hipGetLastError());
    }
    hipLaunchKernelGGL((tm_dupdate_rows_kernel<T>), dim3(TS, g.Ch), dim3(256), 0, st, (const T*)XXt, (const T*)yX,
                       (const T*)D, TS, g.S, g.Ch, w.colabs, w.step);
    DCP_LAUNCH_OK(h, hipGetLastError());
    launch_tm_max<R>(st, w.colabs, TS, R(1.0e-15), w.scal);
    DCP_LAUNCH_OK(h, hipGetLastError());
    hipLaunchKernelGGL((tm_dupdate_apply_kernel<T>), dim3(tm_grid(nD)), dim3(256), 0, st, (const T*)D,
                       (const T*)w.step, (const R*)w.scal, nD, w.U);
    DCP_LAUNCH_OK(h, hipGetLastError());
    // D_new = l2(U) (normalize.py:2-10) into its own buffer (the kernel's ref and out are restrict), rowmax[t] =
    // max |D - D_new| over the row; then D <- D_new
    hipLaunchKernelGGL((row_normalize_kernel<T>), dim3(g.T), dim3(256), 0, st, (const T*)w.U, F, F, 0,
                       (const T*)D, F, w.Dn, F, w.rowmax);
    DCP_LAUNCH_OK(h, hipGetLastError());
    DCP_HIP_OK(h, hipMemcpyAsync(D, w.Dn, (size_t)nD * sizeof(T), hipMemcpyDeviceToDevice, st));
    launch_tm_max<R>(st, w.rowmax, g.T, R(0), w.scal + 2);
    DCP_LAUNCH_OK(h, hipGetLastError());
    void* hostv = nullptr;
    DCP_TRY(host_scratch(h, 64, &hostv));
    DCP_HIP_OK(h, hipMemcpyAsync(hostv, w.scal + 3, sizeof(R), hipMemcpyDeviceToHost, st));
    DCP_HIP_OK(h, hipStreamSynchronize(st));
    *maxdiff = (double)*reinterpret_cast<R*>(hostv);
    return DCP_OK;
}

// Statistics of x and the D update (tm_dstep_around), the partial sums over all C coefficients of every row.
template <class T>
inline int tm_dstep(dcp_handle* h, const T* Y, const T* X, T* D, T* XXt, T* yX, const TmGeom& g, int acc_it,
                    double* maxdiff) {
    hipStream_t st = h->stream;
    const long hmax = tm_hmax(g);
    TmDstepWs<T> w;
    DCP_TRY(ws_lay_out(h, [&](WsLayout& a) { tm_dstep_layout(a, w, g, hmax); }));
    return tm_dstep_around<T>(h, w, X, D, XXt, yX, g, hmax, acc_it, maxdiff, [&]() -> int {
        hipLaunchKernelGGL((tm_stats_core_kernel<T>), dim3(g.T, g.T, g.B), dim3(256), 0, st, X, g, w.mpart);
        DCP_LAUNCH_OK(h, hipGetLastError());
        hipLaunchKernelGGL((tm_stats_yx_kernel<T>), dim3(g.T, g.B), dim3(256), 0, st, Y, X, g, w.yxpart);
        DCP_LAUNCH_OK(h, hipGetLastError());
        return DCP_OK;
    });
}

// The m windows of w samples of a minibatch (tm_gather_kernel): Y [B, Ch, N] -> Yw [m, Ch, w], X [B, T, C] ->
// Xw [m, T, Cw], g the geometry of the signals with its g.Ch channels.  Both dcp_tm_gather_windows_* and
// dcp_tm_mc_gather_windows_* are this function after their geometry.
template <class T>
inline int tm_gather_windows(dcp_handle* h, const T* Y, const T* X, const int64_t* idx_b, const int64_t* idx_n,
                             int64_t m, const TmGeom& g, int64_t w, int padding, T* Yw, T* Xw) {
    TmGeom gw;
    if (!tm_geom(gw, m, g.T, g.S, w, g.s, padding) || w > g.N) return fail(h, DCP_ERR_INVALID, "window geometry");
    if (!Y || !X || !idx_b || !idx_n || !Yw || !Xw) return fail(h, DCP_ERR_INVALID, "null pointer");
    hipLaunchKernelGGL((tm_gather_kernel<T>), dim3(tm_grid(m * (g.Ch * w + g.T * gw.C))), dim3(256), 0, h->stream, Y, X,
                       idx_b, idx_n, (long)m, g.Ch, g.N, g.T, g.C, (long)w, gw.C, Yw, Xw);
    DCP_LAUNCH_OK(h, hipGetLastError());
    return DCP_OK;
}

// ---- the entries of this file's kernels (those of the greedy coders and the event step are in their headers) ----
template <class T>
inline int tm_temp2mat_api(dcp_handle* h, const T* D, const TmShape& sh, T* out) {
    TmGeom g;
    DCP_TRY(tm_geom_api(h, sh, g));
    if (!D || !out) return fail(h, DCP_ERR_INVALID, "null pointer");
    hipLaunchKernelGGL((tm_temp2mat_kernel<T>), dim3(tm_grid(g.T * g.C * g.N)), dim3(256), 0, h->stream, D, g, out);
    DCP_LAUNCH_OK(h, hipGetLastError());
    return DCP_OK;
}

template <class T>
inline int tm_coef2mat_api(dcp_handle* h, const T* X, const TmShape& sh, T* out) {
    TmGeom g;
    DCP_TRY(tm_geom_api(h, sh, g));
    if (!X || !out) return fail(h, DCP_ERR_INVALID, "null pointer");
    hipLaunchKernelGGL((tm_coef2mat_kernel<T>), dim3(tm_grid(g.B * g.T * g.S * g.N)), dim3(256), 0, h->stream, X, g,
                       out);
    DCP_LAUNCH_OK(h, hipGetLastError());
    return DCP_OK;
}

template <class T>
inline int tm_predict_api(dcp_handle* h, const T* X, const T* D, const TmShape& sh, T* out) {
    TmGeom g;
    DCP_TRY(tm_geom_api(h, sh, g));
    if (!X || !D || !out) return fail(h, DCP_ERR_INVALID, "null pointer");
    return tm_launch_residual<T>(h, (const T*)nullptr, X, (const real_t<T>*)nullptr, D, g, out);
}

// The prox is a run-time choice in every dtype (a plain `if`): each dtype's library holds all three step kernels.
template <class T>
inline int tm_lasso_api(dcp_handle* h, const T* Y, const T* D, T* X, const TmShape& sh, double alpha, double tol,
                        int maxiter, int method, int positive, int* it_out) {
    typedef real_t<T> R;
    TmGeom g;
    DCP_TRY(tm_geom_api(h, sh, g));
    if (!Y || !D || !X || !it_out) return fail(h, DCP_ERR_INVALID, "null pointer");
    if (method != DCP_LASSO_ISTA && method != DCP_LASSO_ACC_ISTA && method != DCP_LASSO_FISTA)
        return fail(h, DCP_ERR_INVALID, "structured solver: ista, acc_ista or fista");
    if (positive && scalar_traits<T>::is_complex)
        return fail(h, DCP_ERR_INVALID, "positive solvers need a real dtype (lasso.py:92)");
    if (scalar_traits<T>::is_complex)
        return tm_lasso_solve<T, PROX_COMPLEX>(h, Y, D, X, g, (R)alpha, (R)tol, maxiter, method, it_out);
    if (positive) return tm_lasso_solve<T, PROX_POSITIVE>(h, Y, D, X, g, (R)alpha, (R)tol, maxiter, method, it_out);
    return tm_lasso_solve<T, PROX_REAL>(h, Y, D, X, g, (R)alpha, (R)tol, maxiter, method, it_out);
}

template <class T>
inline int tm_dstep_api(dcp_handle* h, const T* Y, const T* X, T* D, T* XXt, T* yX, const TmShape& sh, int acc_it,
                        double* maxdiff) {
    TmGeom g;
    DCP_TRY(tm_geom_api(h, sh, g));
    if (!Y || !X || !D || !XXt || !yX || !maxdiff) return fail(h, DCP_ERR_INVALID, "null pointer");
    if (acc_it < 0) return fail(h, DCP_ERR_INVALID, "acc_it must be >= 0");
    return tm_dstep<T>(h, Y, X, D, XXt, yX, g, acc_it, maxdiff);
}

template <class T>
inline int tm_gather_windows_api(dcp_handle* h, const T* Y, const T* X, const int64_t* idx_b, const int64_t* idx_n,
                                 int64_t m, const TmShape& sh, int64_t w, T* Yw, T* Xw) {
    TmGeom g;
    DCP_TRY(tm_geom_api(h, sh, g));
    return tm_gather_windows<T>(h, Y, X, idx_b, idx_n, m, g, w, sh.padding, Yw, Xw);
}

template <class T>
inline int tm_scatter_windows_api(dcp_handle* h, const T* Xw, T* X, const int64_t* idx_b, const int64_t* idx_n,
                                  int64_t m, const TmShape& sh, int64_t w) {
    TmGeom g, gw;
    DCP_TRY(tm_geom_api(h, sh, g));
    if (!tm_geom(gw, m, sh.T, sh.S, w, sh.stride, sh.padding) || w > sh.N)
        return fail(h, DCP_ERR_INVALID, "window geometry");
    if (!Xw || !X || !idx_b || !idx_n) return fail(h, DCP_ERR_INVALID, "null pointer");
    hipLaunchKernelGGL((tm_scatter_kernel<T>), dim3(tm_grid(m * g.T * gw.C)), dim3(256), 0, h->stream, Xw, idx_b,
                       idx_n, (long)m, g.T, g.C, gw.C, X);
    DCP_LAUNCH_OK(h, hipGetLastError());
    return DCP_OK;
}

}  // namespace dcp

#include "template_multichannel.hpp"   // the correlation pass and predict for templates D [T, Ch, S]
#include "template_pursuit.hpp"   // matching pursuit on the same operator
#include "template_omp.hpp"       // orthogonal (re-fitting) pursuit on the same operator
#include "template_events.hpp"    // the dictionary step from event lists, for the codes of those two
#include "template_mc_lasso.hpp"  // the proximal-gradient LASSO in Gram form for templates D [T, Ch, S]

// ---- C ABI (one expansion per dtype: template_{f32,f64,c64,c128}.hip).  Every dtype's signature shows void*; the
// shape arguments travel as a TmShape {B, T, S, N, stride, padding[, Ch, mc]}. ----
#define DCP_TM_ABI(SFX, T, P, R)                                                                                     \
    extern "C" int dcp_tm_temp2mat_##SFX(dcp_handle* h, const void* D, int64_t T_, int64_t S, int64_t N,             \
                                         int64_t stride, int padding, void* out) {                                   \
        return dcp::tm_temp2mat_api<T>(h, (const T*)D, {1, T_, S, N, stride, padding}, (T*)out);                     \
    }                                                                                                                \
    extern "C" int dcp_tm_coef2mat_##SFX(dcp_handle* h, const void* X, int64_t B, int64_t T_, int64_t S, int64_t N,  \
                                         int64_t stride, int padding, void* out) {                                   \
        return dcp::tm_coef2mat_api<T>(h, (const T*)X, {B, T_, S, N, stride, padding}, (T*)out);                     \
    }                                                                                                                \
    extern "C" int dcp_tm_predict_##SFX(dcp_handle* h, const void* X, const void* D, int64_t B, int64_t T_,          \
                                        int64_t S, int64_t N, int64_t stride, int padding, void* out) {              \
        return dcp::tm_predict_api<T>(h, (const T*)X, (const T*)D, {B, T_, S, N, stride, padding}, (T*)out);         \
    }                                                                                                                \
    extern "C" int dcp_tm_lasso_##SFX(dcp_handle* h, const void* Y, const void* D, void* X, int64_t B, int64_t T_,   \
                                      int64_t S, int64_t N, int64_t stride, int padding, double alpha, double tol,   \
                                      int maxiter, int method, int positive, int* it_out) {                          \
        return dcp::tm_lasso_api<T>(h, (const T*)Y, (const T*)D, (T*)X, {B, T_, S, N, stride, padding}, alpha, tol,  \
                                    maxiter, method, positive, it_out);                                              \
    }                                                                                                                \
    extern "C" int dcp_tm_mc_lasso_##SFX(dcp_handle* h, const void* Y, const void* D, void* X, int64_t B,            \
                                         int64_t T_, int64_t Ch, int64_t S, int64_t N, int64_t stride, int padding,  \
                                         double alpha, double tol, int maxiter, int method, int positive,            \
                                         int* it_out) {                                                              \
        return dcp::tm_mc_lasso_api<T>(h, (const T*)Y, (const T*)D, (T*)X, {B, T_, S, N, stride, padding, Ch, true}, \
                                       alpha, tol, maxiter, method, positive, it_out);                               \
    }                                                                                                                \
    extern "C" int dcp_tm_pursuit_##SFX(dcp_handle* h, const void* Y, const void* D, void* X, int64_t B,             \
                                        int64_t T_, int64_t S, int64_t N, int64_t stride, int padding,               \
                                        int64_t n_steps, double tol, int positive, int* it_out) {                    \
        return dcp::tm_pursuit_api<T>(h, (const T*)Y, (const T*)D, (T*)X, {B, T_, S, N, stride, padding}, n_steps,   \
                                      tol, positive, it_out);                                                        \
    }                                                                                                                \
    extern "C" int dcp_tm_mc_pursuit_##SFX(dcp_handle* h, const void* Y, const void* D, void* X, int64_t B,          \
                                           int64_t T_, int64_t Ch, int64_t S, int64_t N, int64_t stride,             \
                                           int padding, int64_t n_steps, double tol, int positive, int* it_out) {    \
        return dcp::tm_pursuit_api<T>(h, (const T*)Y, (const T*)D, (T*)X, {B, T_, S, N, stride, padding, Ch, true},  \
                                      n_steps, tol, positive, it_out);                                               \
    }                                                                                                                \
    extern "C" int dcp_tm_pursuit_lds_atoms_##SFX(void) { return (int)dcp::tm_pursuit_lds_atoms<T>(); }              \
    extern "C" int dcp_tm_omp_##SFX(dcp_handle* h, const void* Y, const void* D, void* X, int64_t B, int64_t T_,     \
                                    int64_t S, int64_t N, int64_t stride, int padding, int64_t n_steps, double tol,  \
                                    int* it_out) {                                                                   \
        return dcp::tm_omp_api<T>(h, (const T*)Y, (const T*)D, (T*)X, {B, T_, S, N, stride, padding}, n_steps, tol,  \
                                  it_out);                                                                           \
    }                                                                                                                \
    extern "C" int dcp_tm_mc_omp_##SFX(dcp_handle* h, const void* Y, const void* D, void* X, int64_t B, int64_t T_,  \
                                       int64_t Ch, int64_t S, int64_t N, int64_t stride, int padding,                \
                                       int64_t n_steps, double tol, int* it_out) {                                   \
        return dcp::tm_omp_api<T>(h, (const T*)Y, (const T*)D, (T*)X, {B, T_, S, N, stride, padding, Ch, true},      \
                                  n_steps, tol, it_out);                                                             \
    }                                                                                                                \
    extern "C" int dcp_tm_omp_lds_atoms_##SFX(void) { return (int)dcp::tm_omp_lds_atoms<T>(); }                      \
    extern "C" int dcp_tm_mc_predict_##SFX(dcp_handle* h, const void* X, const void* D, int64_t B, int64_t T_,       \
                                           int64_t Ch, int64_t S, int64_t N, int64_t stride, int padding,            \
                                           void* out) {                                                              \
        return dcp::tm_mc_predict_api<T>(h, (const T*)X, (const T*)D, {B, T_, S, N, stride, padding, Ch, true},      \
                                         (T*)out);                                                                   \
    }                                                                                                                \
    extern "C" int dcp_tm_mc_template_block_##SFX(void) { return dcp::tm_mc_template_block<T>(); }                   \
    extern "C" int dcp_tm_mc_channels_per_pass_##SFX(int64_t S, int64_t stride) {                                    \
        return dcp::tm_mc_channels_per_pass<T>(S, stride);                                                           \
    }                                                                                                                \
    extern "C" int dcp_tm_dstep_##SFX(dcp_handle* h, const void* Y, const void* X, void* D, void* XXt, void* yX,     \
                                      int64_t B, int64_t T_, int64_t S, int64_t N, int64_t stride, int padding,      \
                                      int acc_it, double* maxdiff) {                                                 \
        return dcp::tm_dstep_api<T>(h, (const T*)Y, (const T*)X, (T*)D, (T*)XXt, (T*)yX,                             \
                                    {B, T_, S, N, stride, padding}, acc_it, maxdiff);                                \
    }                                                                                                                \
    extern "C" int dcp_tm_dstep_events_##SFX(dcp_handle* h, const void* Y, const void* X, void* D, void* XXt,        \
                                             void* yX, int64_t B, int64_t T_, int64_t S, int64_t N, int64_t stride,  \
                                             int padding, int acc_it, int64_t max_events, double* maxdiff) {         \
        return dcp::tm_dstep_events_api<T>(h, (const T*)Y, (const T*)X, (T*)D, (T*)XXt, (T*)yX,                      \
                                           {B, T_, S, N, stride, padding}, acc_it, max_events, maxdiff);             \
    }                                                                                                                \
    extern "C" int dcp_tm_mc_dstep_events_##SFX(dcp_handle* h, const void* Y, const void* X, void* D, void* XXt,     \
                                                void* yX, int64_t B, int64_t T_, int64_t Ch, int64_t S, int64_t N,   \
                                                int64_t stride, int padding, int acc_it, int64_t max_events,         \
                                                double* maxdiff) {                                                   \
        return dcp::tm_dstep_events_api<T>(h, (const T*)Y, (const T*)X, (T*)D, (T*)XXt, (T*)yX,                      \
                                           {B, T_, S, N, stride, padding, Ch, true}, acc_it, max_events, maxdiff);   \
    }                                                                                                                \
    extern "C" int dcp_tm_gather_windows_##SFX(dcp_handle* h, const void* Y, const void* X, const int64_t* idx_b,    \
                                               const int64_t* idx_n, int64_t m, int64_t B, int64_t T_, int64_t S,    \
                                               int64_t N, int64_t w, int64_t stride, int padding, void* Yw,          \
                                               void* Xw) {                                                           \
        return dcp::tm_gather_windows_api<T>(h, (const T*)Y, (const T*)X, idx_b, idx_n, m,                           \
                                             {B, T_, S, N, stride, padding}, w, (T*)Yw, (T*)Xw);                     \
    }                                                                                                                \
    extern "C" int dcp_tm_mc_gather_windows_##SFX(dcp_handle* h, const void* Y, const void* X,                       \
                                                  const int64_t* idx_b, const int64_t* idx_n, int64_t m, int64_t B,  \
                                                  int64_t T_, int64_t Ch, int64_t S, int64_t N, int64_t w,           \
                                                  int64_t stride, int padding, void* Yw, void* Xw) {                 \
        return dcp::tm_gather_windows_api<T>(h, (const T*)Y, (const T*)X, idx_b, idx_n, m,                           \
                                             {B, T_, S, N, stride, padding, Ch, true}, w, (T*)Yw, (T*)Xw);           \
    }                                                                                                                \
    extern "C" int dcp_tm_scatter_windows_##SFX(dcp_handle* h, const void* Xw, void* X, const int64_t* idx_b,        \
                                                const int64_t* idx_n, int64_t m, int64_t B, int64_t T_, int64_t S,   \
                                                int64_t N, int64_t w, int64_t stride, int padding) {                 \
        return dcp::tm_scatter_windows_api<T>(h, (const T*)Xw, (T*)X, idx_b, idx_n, m,                               \
                                              {B, T_, S, N, stride, padding}, w);                                    \
    }

