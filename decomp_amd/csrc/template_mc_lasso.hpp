// The proximal-gradient LASSO (ista / acc_ista / fista and their positive forms) for multichannel templates
// D [T, Ch, S], y [B, Ch, N], x [B, T, C] (template_matching.basis_pursuit with a 3-D D, dcp_tm_mc_lasso_*), in Gram
// form.  Included from template_impl.hpp after the greedy coders, whose tm_mc_corr_pass and tm_madd_conj it uses.
//
// The model shares one coefficient among the channels, so the gradient needs y only once:
//   grad[b, t, c] = alpha0[b, t, c] - sum_t' sum_(|c' - c| <= dh) u[b, t', c'] G[(t', c'), (t, c)],   u = v' / rho,
//   alpha0 = y A^H (tm_mc_corr_pass),   G = A A^H over the samples inside [0, N) and the Ch channels.
// G[(t', c'), (t, c)] is the lag correlation Corr[t', t, s (c' - c)] whenever either atom lies inside the signal (their
// overlap then does); the pairs of which neither does are formed once, by explicit sums, into the edge table.  An
// iteration is one kernel and costs T (2 dh + 1) multiply-adds per coefficient whatever Ch is, against the residual
// form's two passes of Ch S each (tm_lasso_solve).  Everything else is tm_lasso_solve's: the scaled variables
// x' = x rho, the threshold alpha Ch N / rho (the dense operator has Ch N columns), tol rho, 1 / L from the Gershgorin
// bound of the scaled Gram matrix, prox_gradient_loop and the epilogue tm_step_epilogue.
//
// The interior of the sum is a correlation of the T-"channel" signal u[b, :, :] of length C with T filters of
// nd = 2 dh + 1 taps at stride 1, so the step runs tm_mc_corr_accumulate, the loop of the greedy coders' correlation
// pass: its geometry here is {T, Ch = T, S = nd, N = C, s = 1, Q = dh}, its samples are v' rinv, and its taps are
//   F[t, t', j] = Corr[t, t', -s (j - dh)] = conj(G[(t', c + j - dh), (t, c)])          (tm_mc_madd conjugates its tap).
// A coefficient whose own atom does not lie inside the signal discards that sum and forms it again with the taps of
// its own row of the edge table.  Either way the sum of a coefficient is tm_mc_madd over t' ascending, c' ascending
// inside (a partner that does not exist adds an exact zero), whatever the tile, the template block or the rest of the
// batch.
//
// The edge table E [T, T, nd, ne], ne = the atoms that do not lie inside (none for 'VALID', every one when N is so
// short that no atom does, about 2 (S - 1) / s for 'SAME'):  E[t, t', j, e(c)] = conj(G[(t', c + j - dh), (t, c)]), which is
// F[t, t', j] for a partner that lies inside and the sum tm_pursuit_gram states, over the overlap inside [0, N) and the
// channels, for one that does not either.  It is formed once per call (Ch S multiply-adds per entry: in every iteration
// they would cost what the Gram form saves).  A table above kTmMcEdgeBytes is refused before anything is launched.
#pragma once

namespace dcp {

constexpr size_t kTmMcEdgeBytes = size_t(1) << 30;   // the workspace budget of a pass of the masked coder

// The atoms whose every tap lies inside the signal are c in [a, a + nin); the others are numbered e = 0 .. ne - 1 in
// ascending c.
struct TmEdge {
    long a = 0, nin = 0, ne = 0;
    DCP_HD bool inside(long c) const { return c >= a && c < a + nin; }
    DCP_HD long index(long c) const { return c < a ? c : c - nin; }   // of a c that is not inside
    DCP_HD long c_of(long e) const { return e < a ? e : e + nin; }
};

inline TmEdge tm_mc_edge(const TmGeom& g) {
    long a = tm_ceil_div(g.Q, g.s), b = tm_floor_div(g.N - g.S + g.Q, g.s);
    if (a < 0) a = 0;
    if (b > g.C - 1) b = g.C - 1;
    TmEdge e;
    e.nin = b >= a ? b - a + 1 : 0;
    e.a = e.nin > 0 ? a : g.C;
    e.ne = g.C - e.nin;
    return e;
}

// F[(t T + t') nd + j] = Corr[t, t', -s (j - dh)]
template <class T>
__global__ void __launch_bounds__(256) tm_mc_lasso_taps_kernel(const T* __restrict__ corr, TmGeom g, T* __restrict__ F) {
    const long nd = g.nd(), W = 2 * g.S - 1;
    for (long i = blockIdx.x * 256L + threadIdx.x; i < g.T * g.T * nd; i += (long)gridDim.x * 256L)
        F[i] = corr[(i / nd) * W + g.S - 1 - g.s * (i % nd - g.dh)];
}

// E[((t T + t') nd + j) ne + e], the tap of atom c = c_of(e) for its partner c' = c + j - dh (e fastest: the threads of
// a tile read consecutive e):  F[t, t', j] when c' lies inside the signal; when it does not,
// sum_ch sum_k D[t, ch, k] conj(D[t', ch, k + s (c - c')]) over the samples of both atoms inside [0, N) (ch ascending,
// k ascending inside); zero when there is no atom c'.
template <class T>
__global__ void __launch_bounds__(256) tm_mc_lasso_edge_kernel(const T* __restrict__ D, const T* __restrict__ F,
                                                               TmGeom g, TmEdge ed, T* __restrict__ E) {
    const long nd = g.nd();
    for (long i = blockIdx.x * 256L + threadIdx.x; i < ed.ne * g.T * g.T * nd; i += (long)gridDim.x * 256L) {
        const long e = i % ed.ne, f = i / ed.ne;   // f = (t T + t') nd + j
        const long j = f % nd, tp = (f / nd) % g.T, t = f / (nd * g.T);
        const long c = ed.c_of(e), cp = c + j - g.dh;
        T G = zero_of<T>();
        if (cp >= 0 && cp < g.C && ed.inside(cp)) {
            G = F[f];
        } else if (cp >= 0 && cp < g.C) {
            const long m = g.s * (c - cp), bj = g.s * c - g.Q;
            long k0 = m < 0 ? -m : 0, k1 = m > 0 ? g.S - 1 - m : g.S - 1;
            if (k0 < -bj) k0 = -bj;
            if (k1 > g.N - 1 - bj) k1 = g.N - 1 - bj;
            for (long ch = 0; ch < g.Ch; ++ch) {
                const long dt = (t * g.Ch + ch) * g.S, dp = (tp * g.Ch + ch) * g.S + m;
                for (long k = k0; k <= k1; ++k) G = tm_madd_conj(G, D[dt + k], D[dp + k]);
            }
        }
        E[i] = G;
    }
}

// u[t', c'] = v'[b, t', c'] rinv[t', c'] of one signal
template <class T>
struct TmMcScaledIterate {
    const T* v;
    const real_t<T>* rinv;
    long C;
    __device__ __forceinline__ T operator()(long t, long c) const { return scale(v[t * C + c], rinv[t * C + c]); }
};

// One iteration.  grid (ceil(C / 256), ceil(T / TB), B <= 65535), dynamic LDS CP (255 + nd) sizeof(T) when LDS; g the
// geometry of the signals, gs that of the correlation loop (above), ep's pointers those of the grid's first signal.
template <class T, int PROX, int TB, bool LDS>
__global__ void __launch_bounds__(256) tm_mc_lasso_step_kernel(const T* __restrict__ alpha0, const T* __restrict__ F,
                                                               const T* __restrict__ E, TmGeom g, TmGeom gs,
                                                               TmEdge ed, int CP, TmStep<T, PROX> ep) {
    const long b = blockIdx.z, t0 = (long)blockIdx.y * TB;
    const long c = (long)blockIdx.x * 256 + threadIdx.x;
    const long nd = gs.S;
    const TmMcScaledIterate<T> u{ep.V + b * g.T * g.C, ep.rinv, g.C};
    T acc[TB];
    tm_mc_corr_accumulate<T, TB, LDS>(u, F, gs, CP, t0, acc);
    if (c >= g.C) return;
    if (!ed.inside(c)) {   // the same sum with this atom's own taps: per-thread operands, the iterate from global memory
        const T* Et[TB];
#pragma unroll
        for (int j = 0; j < TB; ++j) {
            Et[j] = E + (t0 + j < g.T ? t0 + j : g.T - 1) * g.T * nd * ed.ne + ed.index(c);
            acc[j] = zero_of<T>();
        }
        for (long tp = 0; tp < g.T; ++tp) {
#pragma unroll 4
            for (long q = 0; q < nd; ++q) {
                long cp = c - g.dh + q;   // no atom there: its tap is zero, any coefficient serves
                cp = cp < 0 ? 0 : (cp > g.C - 1 ? g.C - 1 : cp);
                const T v = u(tp, cp);
#pragma unroll
                for (int j = 0; j < TB; ++j) acc[j] = tm_mc_madd(acc[j], v, Et[j][(tp * nd + q) * ed.ne]);
            }
        }
    }
#pragma unroll
    for (int j = 0; j < TB; ++j)
        if (t0 + j < g.T)
            tm_step_epilogue(ep, g, sub(alpha0[(b * g.T + t0 + j) * g.C + c], acc[j]), t0 + j, b, c);
}

template <class T, int PROX>
inline int tm_mc_launch_step(dcp_handle* h, const T* alpha0, const T* F, const T* E, const TmGeom& g, const TmGeom& gs,
                             const TmEdge& ed, TmStep<T, PROX> ep) {
    constexpr int TB = tm_mc_template_block<T>();
    const long TC = g.T * g.C;
    int CP = tm_mc_channels_per_pass<T>(gs.S, 1);
    if (CP > g.T) CP = (int)g.T;
    const size_t bytes = (size_t)CP * (size_t)(255 + gs.S) * sizeof(T);
    const T *V = ep.V, *P = ep.P;
    T *Nw = ep.Nw, *Vn = ep.Vn;
    for (long b0 = 0; b0 < g.B; b0 += 65535) {
        const long nb = g.B - b0 < 65535 ? g.B - b0 : 65535;
        const dim3 grid((g.C + 255) / 256, (g.T + TB - 1) / TB, nb);
        ep.V = V + b0 * TC;
        ep.P = P + b0 * TC;
        ep.Nw = Nw + b0 * TC;
        ep.Vn = Vn != nullptr ? Vn + b0 * TC : nullptr;
        if (CP > 0)
            hipLaunchKernelGGL((tm_mc_lasso_step_kernel<T, PROX, TB, true>), grid, dim3(256), bytes, h->stream,
                               alpha0 + b0 * TC, F, E, g, gs, ed, CP, ep);
        else
            hipLaunchKernelGGL((tm_mc_lasso_step_kernel<T, PROX, TB, false>), grid, dim3(256), 0, h->stream,
                               alpha0 + b0 * TC, F, E, g, gs, ed, 0, ep);
        DCP_LAUNCH_OK(h, hipGetLastError());
    }
    return DCP_OK;
}

// tm_lasso_solve for Y [B, Ch, N], D [T, Ch, S] (g.Ch channels), X [B, T, C] (in: initial estimate, out: solution)
template <class T, int PROX>
inline int tm_mc_lasso_solve(dcp_handle* h, const T* Y, const T* D, T* X, const TmGeom& g, real_t<T> alpha,
                             real_t<T> tol, int maxiter, int method, int* it_out) {
    typedef real_t<T> R;
    hipStream_t st = h->stream;
    const long TC = g.T * g.C, BX = g.B * TC, nd = g.nd();
    const TmEdge ed = tm_mc_edge(g);
    const double edge_bytes = (double)ed.ne * (double)g.T * (double)g.T * (double)nd * (double)sizeof(T);
    if (edge_bytes > (double)kTmMcEdgeBytes)
        return fail(h, DCP_ERR_INVALID,
                    "multichannel LASSO: the edge table of the " + std::to_string(ed.ne) +
                        " atoms that do not lie inside the signal needs " + std::to_string((long long)edge_bytes) +
                        " bytes, the limit is " + std::to_string((long long)kTmMcEdgeBytes));
    if (TC > 0x7fffffffLL) return fail(h, DCP_ERR_INVALID, "multichannel LASSO: T C must be below 2^31");
    const long nE = ed.ne * g.T * g.T * nd;
    TmGeom gs;   // the correlation loop's view of the step: u [T, C] against the taps F [T, T, nd]
    gs.B = g.B; gs.T = g.T; gs.Ch = g.T; gs.S = nd; gs.N = g.C; gs.C = g.C; gs.s = 1; gs.Q = g.dh; gs.dh = nd - 1;
    R *rho = nullptr, *rinv = nullptr, *alphak = nullptr, *tolk = nullptr, *colsum = nullptr, *tsum = nullptr;
    R* scal = nullptr;
    int* flag = nullptr;
    T *corr = nullptr, *F = nullptr, *E = nullptr, *alpha0 = nullptr;
    T* xb[4] = {nullptr, nullptr, nullptr, nullptr};   // iterates
    DCP_TRY(ws_lay_out(h, [&](WsLayout& a) {
        a.take(rho, TC);
        a.take(rinv, TC);
        a.take(alphak, TC);
        a.take(tolk, TC);
        a.take(colsum, TC);
        a.take(tsum, g.T);
        a.take(corr, g.T * g.T * (2 * g.S - 1));
        a.take(F, g.T * g.T * nd);
        a.take(E, nE > 0 ? nE : 1);
        a.take(scal, 4);
        a.take(flag, 4);
        a.take(alpha0, BX);
        for (int q = 0; q < 4; ++q) a.take(xb[q], BX);
    }));
    void* hostv = nullptr;
    DCP_TRY(host_scratch(h, 64, &hostv));
    int* host_flag = reinterpret_cast<int*>(hostv);

    // ---- prepare: row norms over the channels, alpha Ch N / rho, tol rho, x' = x rho, Corr, 1 / Gershgorin, the
    // taps, the edge table, alpha0 ----
    hipLaunchKernelGGL((tm_rownorm_kernel<T>), dim3(tm_grid(TC)), dim3(256), 0, st, D, g, alpha * R(g.Ch), tol, rho,
                       rinv, alphak, tolk, flag);
    DCP_LAUNCH_OK(h, hipGetLastError());
    hipLaunchKernelGGL((tm_scale_kernel<T>), dim3(tm_grid(BX)), dim3(256), 0, st, (const T*)X, (const R*)rho, BX, TC,
                       1, xb[0]);
    DCP_LAUNCH_OK(h, hipGetLastError());
    hipLaunchKernelGGL((tm_lagcorr_kernel<T>), dim3(g.T * g.T), dim3(256), 0, st, D, g, corr);
    DCP_LAUNCH_OK(h, hipGetLastError());
    DCP_TRY(tm_gram_bound<T>(h, D, corr, rinv, g, tsum, colsum, scal));
    hipLaunchKernelGGL((tm_mc_lasso_taps_kernel<T>), dim3(tm_grid(g.T * g.T * nd)), dim3(256), 0, st, (const T*)corr,
                       g, F);
    DCP_LAUNCH_OK(h, hipGetLastError());
    if (nE > 0) {
        hipLaunchKernelGGL((tm_mc_lasso_edge_kernel<T>), dim3(tm_grid(nE)), dim3(256), 0, st, D, (const T*)F, g, ed, E);
        DCP_LAUNCH_OK(h, hipGetLastError());
    }
    DCP_TRY(tm_mc_corr_pass<T>(h, Y, D, g, alpha0));

    // ---- one iteration: one kernel ----
    auto step = [&](int, T* V, T* P, T* Nw, T* Vn, R coef, int check, bool) -> int {
        TmStep<T, PROX> ep{V, P, Nw, Vn, rinv, alphak, tolk, scal, coef, check, flag};
        return tm_mc_launch_step<T, PROX>(h, alpha0, F, E, g, gs, ed, ep);
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

// The checks and messages of tm_lasso_api; the prox is a run-time choice in every dtype.
template <class T>
inline int tm_mc_lasso_api(dcp_handle* h, const T* Y, const T* D, T* X, const TmShape& sh, double alpha, double tol,
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
        return tm_mc_lasso_solve<T, PROX_COMPLEX>(h, Y, D, X, g, (R)alpha, (R)tol, maxiter, method, it_out);
    if (positive)
        return tm_mc_lasso_solve<T, PROX_POSITIVE>(h, Y, D, X, g, (R)alpha, (R)tol, maxiter, method, it_out);
    return tm_mc_lasso_solve<T, PROX_REAL>(h, Y, D, X, g, (R)alpha, (R)tol, maxiter, method, it_out);
}

}  // namespace dcp
