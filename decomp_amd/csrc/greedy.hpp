// What the greedy coders share (omp.hpp, omp_mask.hpp, template_pursuit.hpp, template_omp.hpp), defined once: the
// best-atom comparison and its wave butterfly, the wave-level Cholesky factor of the support's Gram matrix, the LDS
// carve around that factor and the scatter of a support into a row of X.  Everything here is called by a whole wave
// and is free of barriers; where a value lives (a register, LDS, the workspace) is the caller's business, the
// functions take values and return values.
#pragma once
#include <hip/hip_runtime.h>

#include "reduce.hpp"

namespace dcp {

// ---- the best atom: the larger score, the LOWER index on a tie, at every level (lane, wave, segment, table) -------
// The order (score, -index) is total, so the result does not depend on how the candidates are grouped: the same atom
// wins for every K, tier and launch geometry, and it is the one a sequential scan with strict > finds.
// (s, i) <- the better of (s, i) and (s2, i2), by two selects (as a branch around two moves a butterfly step costs
// an exec-mask round trip more: 2 % of omp_greedy_kernel in float32)
template <class R>
__device__ __forceinline__ void greedy_better(R& s, int& i, R s2, int i2) {
    const bool take = s2 > s || (s2 == s && i2 < i);
    s = take ? s2 : s;
    i = take ? i2 : i;
}

// the best (score, index) over the wave, the same in every lane (the order is total: a butterfly is enough)
template <class R>
__device__ __forceinline__ void greedy_wave_best(R& s, int& i) {
#pragma unroll
    for (int m = 32; m >= 1; m >>= 1) {
        const R s2 = lane_xor(s, m);
        const int i2 = lane_xor(i, m);
        greedy_better(s, i, s2, i2);
    }
}

// A lane's own candidates, visited in increasing k (strict >: ties keep the lower k): score c of atom k where ok,
// else -1 (a NaN never wins)
template <class R>
__device__ __forceinline__ void greedy_lane_best(R& bc, int& bk, R c, bool ok, int k) {
    c = (ok && c >= R(0)) ? c : R(-1);
    if (c > bc) {
        bc = c;
        bk = k;
    }
}

// ---- the factor --------------------------------------------------------------------------------------------------
// eps_dep = 4096 eps (2^-11 float, 2^-40 double): the pivot of a duplicated atom is a rounding residue of
// G_kk (1 + O(n eps)) - |w|^2, and G itself carries the rounding of an F-long MFMA sum (O(sqrt(F) eps) relative):
// 4096 eps rejects it in every dtype with s <= 64, while an atom 1.3 degrees (float) off the span still passes.
template <class R> DCP_HD R omp_eps_dep();
template <> DCP_HD float  omp_eps_dep<float>()  { return 4.8828125e-4f; }              // 4096 * 2^-23 = 2^-11
template <> DCP_HD double omp_eps_dep<double>() { return 9.094947017729282e-13; }      // 4096 * 2^-52 = 2^-40

// v where keep, else +0, by a bit mask (a select of a loaded value may be sunk into a branch around the load)
__device__ __forceinline__ float omp_keep(float v, bool keep) { return __int_as_float(__float_as_int(v) & -(int)keep); }
__device__ __forceinline__ double omp_keep(double v, bool keep) {
    return __longlong_as_double(__double_as_longlong(v) & -(long long)keep);
}
template <class R>
__device__ __forceinline__ cx<R> omp_keep(cx<R> v, bool keep) { return cx<R>{omp_keep(v.re, keep), omp_keep(v.im, keep)}; }

// row stride of L in elements: odd, so the column walk L[lane][m] of the forward substitution hits 32 distinct banks
// per half-wave in every dtype
DCP_HD int omp_ld(int s) { return s | 1; }

// The Cholesky factor L of G_II, |I| = n, wave-private in LDS: lane j owns row j (lc: the lane clamped into the
// image; LDS reads are unconditional at clamped addresses and masked afterwards).  Each substitution is n
// broadcast-and-FMA steps (v_readlane of the pivot lane's value).  One step of the support, I <- I + (k*):
//   w = forward(b, dinv, wn2)    L w = b, b_j = G[I_j, k*];  d = G_k*k* - |w|^2;  dependent(d, G_k*k*): stop
//   accept(wc, sqrt(d))          row n of L: wc = conj(w) left of the diagonal
//   v = backward(z, dinv, wc)    L^H v = z over the n + 1 rows;  x_I = conj(v)
// Row n is used from registers in the step that forms it, so L is read only across the caller's barrier.
template <class T>
struct OmpFactor {
    typedef real_t<T> R;
    T* L;
    int ld, lane, lc, n;

    // lane j < n: b = b_j and dinv = 1 / L_jj (other lanes: b = 0).  Lane m < n gets w_m, the others 0; wn2 = |w|^2 in
    // every lane.
    __device__ __forceinline__ T forward(T b, R dinv, R& wn2) const {
        T w = zero_of<T>();
        wn2 = R(0);
        for (int m = 0; m < n; ++m) {
            const T wm = lane_bcast(scale(b, dinv), m);
            wn2 += abs2(wm);
            const T lcol = omp_keep(L[lc * ld + m], lane > m && lane < n);   // column m: odd stride, no conflict
            b = fmsub(b, lcol, wm);
            if (lane == m) w = wm;
        }
        return w;
    }

    // a_k* numerically in the span of A_I (or a NaN): the step is refused and the previous x stands
    static __device__ __forceinline__ bool dependent(R d, R gkk) { return !(d > omp_eps_dep<R>() * gkk); }

    // lane j < n: wc = conj(w_j)
    __device__ __forceinline__ void accept(T wc, R ldiag) const {
        if (lane < n) L[n * ld + lane] = wc;
        if (lane == n) L[n * ld + n] = from_real<T>(ldiag);
    }

    // lane j <= n: z = z_j and dinv = 1 / L_jj, row n included (other lanes: z = 0); lane j < n: wc = conj(w_j), else 0.
    // Lane m <= n gets v_m.
    __device__ __forceinline__ T backward(T z, R dinv, T wc) const {
        T v = zero_of<T>();
        {
            const T vm = lane_bcast(scale(z, dinv), n);
            z = fmsub(z, conj_of(wc), vm);
            if (lane == n) v = vm;
        }
        for (int m = n - 1; m >= 0; --m) {
            const T vm = lane_bcast(scale(z, dinv), m);
            const T lrow = omp_keep(L[m * ld + lc], lane < m);   // row m: contiguous
            z = fmsub(z, conj_of(lrow), vm);
            if (lane == m) v = vm;
        }
        return v;
    }
};

// ---- the LDS image of a wave's state: L [s][s | 1], xs [s], a0s [n_a0] (T), then sel [s] (int), as byte offsets -----
template <class T>
struct OmpCarve {
    size_t xs, a0s, sel, bytes;   // L is at 0
    static DCP_HD size_t up(size_t b) { return (b + 15) & ~size_t(15); }
    DCP_HD OmpCarve(int s, size_t n_a0 = 0) {
        xs = (size_t)s * omp_ld(s) * sizeof(T);
        a0s = xs + (size_t)s * sizeof(T);
        sel = up(a0s + n_a0 * sizeof(T));
        bytes = sel + up((size_t)s * sizeof(int));
    }
};

// ---- xrow[k] = xs[j] where sel[j] == k, else 0: the row of X, zeros off the support -----------------------------
template <class T>
__device__ __forceinline__ void omp_scatter_row(const int* sel, const T* xs, int n, T* xrow, int K, int lane) {
    for (int k = lane; k < K; k += 64) {
        T val = zero_of<T>();
        for (int j = 0; j < n; ++j) {
            const bool here = sel[j] == k;
            const T xj = xs[j];
            val = here ? xj : val;
        }
        xrow[k] = val;
    }
}

}  // namespace dcp
