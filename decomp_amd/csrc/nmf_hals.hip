// C ABI: NMF by HALS (exact block coordinate descent, squared loss, no mask), its row-sharded loop and split
// step, the non-negative coordinate sweep on its own, and em-hals (HALS on the data with its missing entries
// imputed from the current model: dcp_nmf_impute_*, dcp_nmf_emhals_*).  Contract in include/decomp_hip.h; the
// sweep kernels in nmf_hals.hpp, the imputing epilogue (EpiImpute) in epilogue.hpp.
#include <cmath>

#include "comm.hpp"
#include "nmf_hals.hpp"
#include "nmf_loop.hpp"

using namespace dcp;

namespace {

int sweep_rc(dcp_handle* h, hipError_t e) {
    if (e != hipSuccess) return fail(h, DCP_ERR_HIP, std::string("launch failed: ") + hipGetErrorString(e));
    return DCP_OK;
}

// The two halves of one HALS iteration from (Xc, Dc) into (Xn, U), split where the sharded loop all-reduces:
// hals_x_side (every term local to this rank's rows, or replicated)
//   G = Dc Dc^T, C = Y Dc^T           (w.G, w.Q)
//   Xn = sweep(Xc, C, G)              vector-major, N vectors
// With the L1/L2 penalty on the codes (dcp_set_nmf_penalty) the x sweep is the exact coordinate minimiser of the
// penalised objective, which is the same sweep on C = Y Dc^T - l1 and G = Dc Dc^T + l2 I: the kernels that write
// w.Q and w.G fold the penalty in (EpiStoreSub / reduce_slabs_affine_kernel), the sweep kernel is unchanged.
//   stats = [Xn^T Y | Xn^T Xn]        the statistics product of the MU loop (nmf_stats, D-side phase)
// hals_d_sweep (from the statistics summed over the ranks)
//   U = sweep(Dc, (Xn^T Y)^T, Xn^T Xn)   coordinate-major, F vectors (the columns of D)
template <class T>
int hals_x_side(dcp_handle* h, const T* Y, const T* Xc, T* Xn, const T* Dc, const NmfShape<T>& s, T* stats,
                NmfStatsWs<T>& w, NmfPenalty pen) {
    hipStream_t st = h->stream;
    const int N = (int)s.N, F = (int)s.F, K = (int)s.K;
    {   // G = D D^T (split over F, partial slabs summed in order), as the MU loop's Gram product
        ProfScope ps(h, DCP_PROF_GRAM);
        GemmArgs<T> g;
        g.A = Dc; g.lda = F; g.B = Dc; g.ldb = F; g.M = K; g.N = K; g.K = F;
        if (!std::is_same<T, float>::value) g.tile = TILE_SMALL_DEEP;
        plan_splits<FORM_NT>(g, 512, kMaxSplits, 16);
        DCP_LAUNCH_OK(h, (gemm<FORM_NT>(st, g, EpiSlab<T>{w.slabs, K, (long)K * K})));
        if (pen.on())   // G + l2 I
            launch_reduce_slabs_affine<T>(st, w.slabs, (long)K * K, g.ksplits, (long)K * K, T(0), (long)K, T(pen.l2),
                                          w.G);
        else
            launch_reduce_slabs_scalar<T>(st, w.slabs, (long)K * K, g.ksplits, (long)K * K, w.G);
        DCP_LAUNCH_OK(h, hipGetLastError());
    }
    {   // C = Y D^T, then the x sweep
        ProfScope ps(h, DCP_PROF_XUPDATE);
        GemmArgs<T> pg;
        pg.A = Y; pg.lda = F; pg.B = Dc; pg.ldb = F; pg.M = N; pg.N = K; pg.K = F;
        const int psplits = nmf_xupdate_splits<T>(s.N, s.F, s.K, pg);
        if (psplits <= 1) {
            pg.ksplits = 1;
            if (pen.on())   // Y D^T - l1
                DCP_LAUNCH_OK(h, (nmf_product<FORM_NT>(h, st, pg, EpiStoreSub<T>{w.Q, K, T(pen.l1)}, true)));
            else
                DCP_LAUNCH_OK(h, (nmf_product<FORM_NT>(h, st, pg, EpiStore<T>{w.Q, K}, true)));
        } else {   // few rows: split the F reduction so that all CUs work, slabs summed in order
            if ((size_t)pg.ksplits * N * K > w.slab_count)
                return fail(h, DCP_ERR_INTERNAL, "hals Y.D^T slab plan mismatch");
            DCP_LAUNCH_OK(h, (nmf_product<FORM_NT>(h, st, pg, EpiSlab<T>{w.slabs, K, (long)N * K}, true)));
            if (pen.on())   // Y D^T - l1
                launch_reduce_slabs_affine<T>(st, w.slabs, (long)N * K, pg.ksplits, (long)N * K, T(pen.l1), 0L, T(0),
                                              w.Q);
            else
                launch_reduce_slabs<T>(st, w.slabs, (long)N * K, pg.ksplits, (long)N * K, w.Q);
            DCP_LAUNCH_OK(h, hipGetLastError());
        }
        DCP_TRY(sweep_rc(h, launch_nn_cd_sweep<T, false>(st, Xc, Xn, K, w.Q, K, w.G, K, N, K)));
    }
    return nmf_stats<T>(h, Y, nullptr, Xn, Xn, Dc, s, stats, w, 2);
}

// Yi = mask o Y + (1 - mask) o (Xc Dc): the E step of em-hals.  One fp32 / fp64-core product with the imputing
// epilogue (EpiImpute); an exact HALS iteration on Yi cannot increase 1/2 sum mask o (Y - x D)^2, which
// 1/2 |Yi - x D|^2 majorises and touches at (Xc, Dc).
template <class T>
int hals_impute(dcp_handle* h, const T* Y, const T* mask, const T* Xc, const T* Dc, int64_t N, int64_t F, int64_t K,
                T* Yi) {
    ProfScope ps(h, DCP_PROF_FWD);
    GemmArgs<T> a;
    a.A = Xc; a.lda = (int)K; a.B = Dc; a.ldb = (int)F; a.M = (int)N; a.N = (int)F; a.K = (int)K;
    DCP_LAUNCH_OK(h, (gemm<FORM_NN>(h->stream, a, EpiImpute<T>{Y, mask, Yi, (long)F})));
    return DCP_OK;
}

template <class T>
int hals_d_sweep(dcp_handle* h, const T* Dc, T* U, int64_t F, int64_t K, const T* stats) {
    ProfScope ps(h, DCP_PROF_DUPDATE);
    const long W = (long)(F + K);
    return sweep_rc(h, launch_nn_cd_sweep<T, true>(h->stream, Dc, U, (long)F, stats, W, stats + F, W, (int)F,
                                                   (int)K));
}

// D_new = U with unit-norm rows, max|Dc - D_new| into *maxdiff_dev (see hals_normalize_kernel), X[:, k] *= ||U_k||
template <class T>
int hals_normalize_rescale(dcp_handle* h, const T* U, const T* Dc, T* Dn, T* X, int64_t N, int64_t F, int64_t K,
                           T* nrm, T* maxdiff_dev, T* maxdiff_next, unsigned int* ticket, T* host_out) {
    ProfScope ps(h, DCP_PROF_DNORM);
    hipLaunchKernelGGL((hals_normalize_kernel<T>), dim3((unsigned)K), dim3(256), 0, h->stream, U, (long)F, Dc, Dn,
                       nrm, maxdiff_dev, maxdiff_next, ticket, host_out);
    DCP_LAUNCH_OK(h, hipGetLastError());
    hipLaunchKernelGGL((hals_rescale_kernel<T>), dim3(grid_for((long)N * K)), dim3(256), 0, h->stream, X,
                       (long)N * K, (int)K, (const T*)nrm);
    DCP_LAUNCH_OK(h, hipGetLastError());
    return DCP_OK;
}

// One HALS iteration for nmf_lagged_loop:  hals_x_side  [all-reduce of `stats`]  hals_d_sweep  normalise + rescale
// With a mask (em-hals) the iteration starts with hals_impute and both half-steps read the imputed data Yi
// instead of Y; without one exactly the kernels above run.
template <class T>
struct HalsStep {
    const T* Y;
    NmfShape<T> s;
    NmfPenalty pen;
    bool sharded;
    const T* mask = nullptr;
    T* Yi = nullptr;    // [N, F] imputed data (mask only)
    NmfStatsWs<T> ws;
    T* stats = nullptr;
    T* U = nullptr;     // the swept, not yet normalised D
    T* nrm = nullptr;   // atom norms

    void layout(WsLayout& a) {
        nmf_stats_layout(a, ws, s, false);
        a.take(stats, (size_t)s.K * (s.F + s.K));
        a.take(U, (size_t)s.K * s.F);
        a.take(nrm, (size_t)s.K);
        if (mask) a.take(Yi, (size_t)s.N * s.F);
    }
    int prepare(dcp_handle*) { return DCP_OK; }
    int iterate(dcp_handle* h, const T* Xc, T* Xn, const T* Dc, T* Dn, const NmfStopSlots<T>& slots) {
        const T* Yd = Y;
        if (mask) {   // one imputation per iteration, from the iterate both half-steps start from
            DCP_TRY(hals_impute<T>(h, Y, mask, Xc, Dc, s.N, s.F, s.K, Yi));
            Yd = Yi;
        }
        DCP_TRY(hals_x_side<T>(h, Yd, Xc, Xn, Dc, s, stats, ws, pen));
        if (sharded) {   // the one exchange of the step: the D sweep reads sums over all ranks' rows
            ProfScope ps(h, DCP_PROF_EXCHANGE);
            DCP_TRY(comm_allreduce_sum(h, stats, (size_t)s.K * (s.F + s.K),
                                       std::is_same<T, float>::value ? COMM_F32 : COMM_F64));
        }
        DCP_TRY(hals_d_sweep<T>(h, Dc, U, s.F, s.K, stats));
        return hals_normalize_rescale<T>(h, U, Dc, Dn, Xn, s.N, s.F, s.K, nrm, slots.md, slots.md_next, slots.ticket,
                                         slots.host);
    }
};

template <class T>
int nmf_hals_solve(dcp_handle* h, const T* Y, T* X, T* D, int64_t N, int64_t F, int64_t K, T tol, int maxiter,
                   int* it_out, T* last_maxdiff, T* resid_trace, bool sharded = false, const T* mask = nullptr) {
    DCP_TRY(check_nmf_dims(h, Y, X, D, N, F, K));
    if (!it_out) return fail(h, DCP_ERR_INVALID, "it_out is null");
    if (sharded && !comm_active(h))
        return fail(h, DCP_ERR_COMM, mask ? "dcp_nmf_emhals_sharded_* needs a communicator (dcp_comm_init)"
                                          : "dcp_nmf_hals_sharded_* needs a communicator (dcp_comm_init)");
    DCP_HIP_OK(h, hipSetDevice(h->device));
    // the shape stays "not masked": the statistics are those of plain HALS on the imputed data
    HalsStep<T> step{Y, NmfShape<T>{N, F, K, DCP_LIK_L2, false}, nmf_penalty(h), sharded, mask};
    return nmf_lagged_loop<T>(h, step, Y, mask, X, D, N, F, K, tol, maxiter, it_out, last_maxdiff, resid_trace);
}

// dcp_nmf_impute_*: the E step on its own, asynchronous (no workspace).
template <class T>
int nmf_impute_api(dcp_handle* h, const T* Y, const T* mask, const T* X, const T* D, int64_t N, int64_t F, int64_t K,
                   T* Y_out) {
    DCP_TRY(check_nmf_dims(h, Y, X, D, N, F, K));
    if (!mask || !Y_out) return fail(h, DCP_ERR_INVALID, "mask / Y_out is null");
    DCP_HIP_OK(h, hipSetDevice(h->device));
    return hals_impute<T>(h, Y, mask, X, D, N, F, K, Y_out);
}

// dcp_nmf_hals_stats_*: the x side of one iteration, up to the exchange point.  Same kernels in the same order
// as the loop above, so that the Python loop (decomp_amd.sharded.mu_loop) reproduces it bit for bit.
template <class T>
int nmf_hals_stats_api(dcp_handle* h, const T* Y, const T* X, T* X_out, const T* D, int64_t N, int64_t F, int64_t K,
                       T* stats) {
    DCP_TRY(check_nmf_dims(h, Y, X, D, N, F, K));
    if (!stats || !X_out) return fail(h, DCP_ERR_INVALID, "stats / X_out is null");
    DCP_HIP_OK(h, hipSetDevice(h->device));
    NmfShape<T> s{N, F, K, DCP_LIK_L2, false};
    NmfStatsWs<T> ws;
    DCP_TRY(ws_lay_out(h, [&](WsLayout& a) { nmf_stats_layout(a, ws, s, false); }));
    return hals_x_side<T>(h, Y, X, X_out, D, s, stats, ws, nmf_penalty(h));
}

// dcp_nmf_hals_update_*: the D sweep from the (all-reduced) statistics, the normalisation and the x rescale.
template <class T>
int nmf_hals_update_api(dcp_handle* h, const T* stats, const T* D, T* D_new, T* X, int64_t N, int64_t F,
                        int64_t K, T* maxdiff_dev, T* maxdiff_next) {
    if (h && (!D_new || !maxdiff_dev)) return fail(h, DCP_ERR_INVALID, "null pointer");
    DCP_TRY(check_nmf_dims(h, stats, D, X, N, F, K, "null pointer"));
    DCP_HIP_OK(h, hipSetDevice(h->device));
    // shares the arena with dcp_nmf_hals_stats_*: its temporaries are dead by now (same stream)
    T* U = nullptr;     // the swept, not yet normalised D
    T* nrm = nullptr;   // atom norms
    DCP_TRY(ws_lay_out(h, [&](WsLayout& a) {
        a.take(U, (size_t)K * F);
        a.take(nrm, (size_t)K);
    }));
    DCP_TRY(hals_d_sweep<T>(h, D, U, F, K, stats));
    // without a ping-pong partner the max is formed from zero here (the kernel's atomic max needs it)
    if (!maxdiff_next) DCP_HIP_OK(h, hipMemsetAsync(maxdiff_dev, 0, sizeof(T), h->stream));
    return hals_normalize_rescale<T>(h, U, D, D_new, X, N, F, K, nrm, maxdiff_dev, maxdiff_next, nullptr, nullptr);
}

template <class T>
int nn_cd_sweep_api(dcp_handle* h, const T* V_in, T* V_out, const T* C, const T* G, int64_t R, int64_t K,
                    int coord_major) {
    if (!h) return DCP_ERR_INVALID;
    if (!V_in || !V_out || !C || !G) return fail(h, DCP_ERR_INVALID, "null array pointer");
    if (R <= 0 || K <= 0) return fail(h, DCP_ERR_INVALID, "sizes must be positive");
    if (R > 0x7fffffffLL || K > 0x7fffffffLL) return fail(h, DCP_ERR_INVALID, "dimension exceeds 2^31-1");
    DCP_HIP_OK(h, hipSetDevice(h->device));
    if (coord_major)
        return sweep_rc(h, launch_nn_cd_sweep<T, true>(h->stream, V_in, V_out, (long)R, C, (long)R, G, (long)K,
                                                          (int)R, (int)K));
    return sweep_rc(h, launch_nn_cd_sweep<T, false>(h->stream, V_in, V_out, (long)K, C, (long)K, G, (long)K,
                                                       (int)R, (int)K));
}

}  // namespace

extern "C" {

int dcp_nmf_hals_f32(dcp_handle* h, const float* Y, float* X, float* D, int64_t N, int64_t F, int64_t K, float tol,
                     int maxiter, int* it_out, float* last_maxdiff, float* resid_trace) {
    return nmf_hals_solve<float>(h, Y, X, D, N, F, K, tol, maxiter, it_out, last_maxdiff, resid_trace);
}
int dcp_nmf_hals_f64(dcp_handle* h, const double* Y, double* X, double* D, int64_t N, int64_t F, int64_t K,
                     double tol, int maxiter, int* it_out, double* last_maxdiff, double* resid_trace) {
    return nmf_hals_solve<double>(h, Y, X, D, N, F, K, tol, maxiter, it_out, last_maxdiff, resid_trace);
}
int dcp_nmf_hals_sharded_f32(dcp_handle* h, const float* Y, float* X, float* D, int64_t N, int64_t F, int64_t K,
                             float tol, int maxiter, int* it_out, float* last_maxdiff) {
    return nmf_hals_solve<float>(h, Y, X, D, N, F, K, tol, maxiter, it_out, last_maxdiff, nullptr, true);
}
int dcp_nmf_hals_sharded_f64(dcp_handle* h, const double* Y, double* X, double* D, int64_t N, int64_t F, int64_t K,
                             double tol, int maxiter, int* it_out, double* last_maxdiff) {
    return nmf_hals_solve<double>(h, Y, X, D, N, F, K, tol, maxiter, it_out, last_maxdiff, nullptr, true);
}
int dcp_nmf_impute_f32(dcp_handle* h, const float* Y, const float* mask, const float* X, const float* D, int64_t N,
                       int64_t F, int64_t K, float* Y_out) {
    return nmf_impute_api<float>(h, Y, mask, X, D, N, F, K, Y_out);
}
int dcp_nmf_impute_f64(dcp_handle* h, const double* Y, const double* mask, const double* X, const double* D,
                       int64_t N, int64_t F, int64_t K, double* Y_out) {
    return nmf_impute_api<double>(h, Y, mask, X, D, N, F, K, Y_out);
}
int dcp_nmf_emhals_f32(dcp_handle* h, const float* Y, const float* mask, float* X, float* D, int64_t N, int64_t F,
                       int64_t K, float tol, int maxiter, int* it_out, float* last_maxdiff, float* resid_trace) {
    return nmf_hals_solve<float>(h, Y, X, D, N, F, K, tol, maxiter, it_out, last_maxdiff, resid_trace, false, mask);
}
int dcp_nmf_emhals_f64(dcp_handle* h, const double* Y, const double* mask, double* X, double* D, int64_t N,
                       int64_t F, int64_t K, double tol, int maxiter, int* it_out, double* last_maxdiff,
                       double* resid_trace) {
    return nmf_hals_solve<double>(h, Y, X, D, N, F, K, tol, maxiter, it_out, last_maxdiff, resid_trace, false, mask);
}
int dcp_nmf_emhals_sharded_f32(dcp_handle* h, const float* Y, const float* mask, float* X, float* D, int64_t N,
                               int64_t F, int64_t K, float tol, int maxiter, int* it_out, float* last_maxdiff) {
    return nmf_hals_solve<float>(h, Y, X, D, N, F, K, tol, maxiter, it_out, last_maxdiff, nullptr, true, mask);
}
int dcp_nmf_emhals_sharded_f64(dcp_handle* h, const double* Y, const double* mask, double* X, double* D, int64_t N,
                               int64_t F, int64_t K, double tol, int maxiter, int* it_out, double* last_maxdiff) {
    return nmf_hals_solve<double>(h, Y, X, D, N, F, K, tol, maxiter, it_out, last_maxdiff, nullptr, true, mask);
}
int dcp_nmf_hals_stats_f32(dcp_handle* h, const float* Y, const float* X, float* X_out, const float* D, int64_t N,
                           int64_t F, int64_t K, float* stats) {
    return nmf_hals_stats_api<float>(h, Y, X, X_out, D, N, F, K, stats);
}
int dcp_nmf_hals_stats_f64(dcp_handle* h, const double* Y, const double* X, double* X_out, const double* D,
                           int64_t N, int64_t F, int64_t K, double* stats) {
    return nmf_hals_stats_api<double>(h, Y, X, X_out, D, N, F, K, stats);
}
int dcp_nmf_hals_update_f32(dcp_handle* h, const float* stats, const float* D, float* D_new, float* X, int64_t N,
                            int64_t F, int64_t K, float* maxdiff_dev, float* maxdiff_next) {
    return nmf_hals_update_api<float>(h, stats, D, D_new, X, N, F, K, maxdiff_dev, maxdiff_next);
}
int dcp_nmf_hals_update_f64(dcp_handle* h, const double* stats, const double* D, double* D_new, double* X,
                            int64_t N, int64_t F, int64_t K, double* maxdiff_dev, double* maxdiff_next) {
    return nmf_hals_update_api<double>(h, stats, D, D_new, X, N, F, K, maxdiff_dev, maxdiff_next);
}
int dcp_nn_cd_sweep_f32(dcp_handle* h, const float* V_in, float* V_out, const float* C, const float* G, int64_t R,
                        int64_t K, int coord_major) {
    return nn_cd_sweep_api<float>(h, V_in, V_out, C, G, R, K, coord_major);
}
int dcp_nn_cd_sweep_f64(dcp_handle* h, const double* V_in, double* V_out, const double* C, const double* G,
                        int64_t R, int64_t K, int coord_major) {
    return nn_cd_sweep_api<double>(h, V_in, V_out, C, G, R, K, coord_major);
}

}  // extern "C"
