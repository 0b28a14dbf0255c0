// C ABI: NMF multiplicative update (see include/decomp_hip.h for the contract and the
// reference lines each entry point replaces).
#include <cmath>

#include "comm.hpp"
#include "nmf_loop.hpp"

using namespace dcp;

namespace {

template <class T>
int check_nmf_args(dcp_handle* h, const T* Y, const T* X, const T* D, int64_t N, int64_t F,
                   int64_t K, int lik) {
    DCP_TRY(check_nmf_dims(h, Y, X, D, N, F, K));
    if (lik != DCP_LIK_L2 && lik != DCP_LIK_KL && lik != DCP_LIK_BETA) return fail(h, DCP_ERR_INVALID, "bad likelihood");
    return DCP_OK;
}

// One MU iteration for nmf_lagged_loop:  stats(...)  [all-reduce of `stats` across ranks]  update(...)
template <class T>
struct MuStep {
    const T* Y;
    const T* mask;
    NmfShape<T> s;
    bool sharded;
    NmfStatsWs<T> ws;
    NmfUpdateWs<T> wu;
    T* stats = nullptr;
    uint32_t* mbits = nullptr;
    int* mflag = nullptr;
    const T* Ypre = nullptr;

    int64_t W() const { return nmf_stats_width(s.F, s.K, s.lik, s.masked); }
    bool want_bits() const { return s.masked && std::is_same<T, float>::value && s.lik == DCP_LIK_L2; }
    void layout(WsLayout& a) {
        nmf_stats_layout(a, ws, s, s.masked);
        nmf_update_layout(a, wu, s.F, s.K);
        a.take(stats, (size_t)s.K * W());
        if (want_bits()) {
            a.take(mbits, mask_bits_words(s.N, s.F));
            a.take(mflag, 4);
        }
    }
    int prepare(dcp_handle* h) {
        Ypre = Y;
        if (!s.masked) return DCP_OK;
        // y * mask is loop invariant (grads.py:114,124 recompute it every call)
        int binary = 0;
        DCP_TRY(nmf_mask_prepare<T>(h, Y, mask, s.N, s.F, ws.Ym, mbits, mflag, &binary));
        Ypre = ws.Ym;
        if (binary) ws.mbits = mbits;
        return DCP_OK;
    }
    int iterate(dcp_handle* h, const T* Xc, T* Xn, const T* Dc, T* Dn, const NmfStopSlots<T>& slots) {
        DCP_TRY(nmf_stats<T>(h, Ypre, mask, Xc, Xn, Dc, s, stats, ws, 3, nmf_penalty(h)));
        if (sharded) {   // the one exchange of the step: sums over rows become sums over ranks
            ProfScope ps(h, DCP_PROF_EXCHANGE);
            DCP_TRY(comm_allreduce_sum(h, stats, (size_t)s.K * W(),
                                       std::is_same<T, float>::value ? COMM_F32 : COMM_F64));
        }
        // max|D - D_new| reaches the host without a copy kernel: the normalisation's last-arriving workgroup stores
        // it into the pinned (device-mapped) slot, which the stop test polls
        return nmf_update<T>(h, stats, Dc, Dn, s.F, s.K, s.lik, s.masked, slots.md, wu, slots.md_next, slots.ticket,
                             slots.host);
    }
};

template <class T>
int nmf_mu_solve(dcp_handle* h, const T* Y, const T* mask, T* X, T* D, int64_t N, int64_t F,
                 int64_t K, int lik, T tol, int maxiter, int* it_out, T* last_maxdiff,
                 T* resid_trace, bool sharded = false) {
    DCP_TRY(check_nmf_args(h, Y, X, D, N, F, K, lik));
    if (!it_out) return fail(h, DCP_ERR_INVALID, "it_out is null");
    if (sharded && !comm_active(h))
        return fail(h, DCP_ERR_COMM, "dcp_nmf_mu_sharded_* needs a communicator (dcp_comm_init)");
    DCP_HIP_OK(h, hipSetDevice(h->device));
    MuStep<T> step{Y, mask, NmfShape<T>{N, F, K, lik, mask != nullptr}, sharded};
    return nmf_lagged_loop<T>(h, step, Y, mask, X, D, N, F, K, tol, maxiter, it_out, last_maxdiff, resid_trace);
}

// [N,F] scratch and per-workgroup double partials of the scalar read-backs (residual, log-likelihood, divergence),
// with the pinned words the partials are summed from.
template <class T>
struct NmfScalarWs {
    static constexpr int blocks = 1024;
    T* tmp = nullptr;
    double* part = nullptr;
    double* host = nullptr;
    int reserve(dcp_handle* h, int64_t N, int64_t F) {
        DCP_TRY(ws_lay_out(h, [&](WsLayout& a) {
            a.take(tmp, (size_t)N * F);
            a.take(part, blocks);
        }));
        void* hostv = nullptr;
        DCP_TRY(host_scratch(h, sizeof(double) * blocks, &hostv));
        host = reinterpret_cast<double*>(hostv);
        return DCP_OK;
    }
    int sum(dcp_handle* h, double* out) const { return read_partial_sum(h, part, blocks, host, out); }
};

template <class T>
int nmf_mu_stats_api(dcp_handle* h, const T* Y, const T* mask, const T* X, T* X_out, const T* D,
                     int64_t N, int64_t F, int64_t K, int lik, T* stats) {
    DCP_TRY(check_nmf_args(h, Y, X, D, N, F, K, lik));
    if (!stats || !X_out) return fail(h, DCP_ERR_INVALID, "stats / X_out is null");
    DCP_HIP_OK(h, hipSetDevice(h->device));
    const bool masked = mask != nullptr;
    NmfShape<T> s{N, F, K, lik, masked};
    NmfStatsWs<T> ws;
    DCP_TRY(ws_lay_out(h, [&](WsLayout& a) { nmf_stats_layout(a, ws, s, masked); }));
    const T* Ypre = nullptr;
    DCP_TRY(nmf_premask<T>(h, Y, mask, N, F, ws.Ym, &Ypre));
    return nmf_stats<T>(h, Ypre, mask, X, X_out, D, s, stats, ws, 3, nmf_penalty(h));
}

// dcp_nmf_mu_stats_* with the loop-invariant mask work done once by dcp_nmf_mask_prepare_*.
template <class T>
int nmf_mu_stats_prepared_api(dcp_handle* h, const T* Ym, const T* mask, const uint32_t* bits, const T* X,
                              T* X_out, const T* D, int64_t N, int64_t F, int64_t K, int lik, T* stats) {
    DCP_TRY(check_nmf_args(h, Ym, X, D, N, F, K, lik));
    if (!stats || !X_out || !mask) return fail(h, DCP_ERR_INVALID, "stats / X_out / mask is null");
    DCP_HIP_OK(h, hipSetDevice(h->device));
    NmfShape<T> s{N, F, K, lik, true};
    NmfStatsWs<T> ws;
    DCP_TRY(ws_lay_out(h, [&](WsLayout& a) { nmf_stats_layout(a, ws, s, false); }));
    ws.mbits = bits;
    return nmf_stats<T>(h, Ym, mask, X, X_out, D, s, stats, ws, 3, nmf_penalty(h));
}

template <class T>
int nmf_mask_prepare_api(dcp_handle* h, const T* Y, const T* mask, int64_t N, int64_t F, T* Ym,
                         uint32_t* bits, int* binary) {
    if (!h) return DCP_ERR_INVALID;
    if (!Y || !mask || !Ym || !binary) return fail(h, DCP_ERR_INVALID, "null pointer");
    if (N <= 0 || F <= 0) return fail(h, DCP_ERR_INVALID, "sizes must be positive");
    DCP_HIP_OK(h, hipSetDevice(h->device));
    int* flag = nullptr;
    DCP_TRY(ws_lay_out(h, [&](WsLayout& a) { a.take(flag, 4); }));
    return nmf_mask_prepare<T>(h, Y, mask, N, F, Ym, bits, flag, binary);
}

template <class T>
int nmf_mu_update_api(dcp_handle* h, const T* stats, const T* D, T* D_new, int64_t F, int64_t K,
                      int lik, int masked, T* maxdiff_dev, T* maxdiff_next) {
    if (!h) return DCP_ERR_INVALID;
    if (!stats || !D || !D_new || !maxdiff_dev) return fail(h, DCP_ERR_INVALID, "null pointer");
    if (F <= 0 || K <= 0) return fail(h, DCP_ERR_INVALID, "sizes must be positive");
    DCP_HIP_OK(h, hipSetDevice(h->device));
    // NOTE: shares the arena with dcp_nmf_mu_stats_*: the stats call's temporaries are dead
    // by now (same stream), `stats` itself is caller memory.
    NmfUpdateWs<T> wu;
    DCP_TRY(ws_lay_out(h, [&](WsLayout& a) { nmf_update_layout(a, wu, F, K); }));
    return nmf_update<T>(h, stats, D, D_new, F, K, lik, masked != 0, maxdiff_dev, wu, maxdiff_next);
}

template <class T>
int nmf_residual_api(dcp_handle* h, const T* Y, const T* mask, const T* X, const T* D, int64_t N,
                     int64_t F, int64_t K, double* out) {
    DCP_TRY(check_nmf_args(h, Y, X, D, N, F, K, DCP_LIK_L2));
    if (!out) return fail(h, DCP_ERR_INVALID, "out is null");
    DCP_HIP_OK(h, hipSetDevice(h->device));
    NmfScalarWs<T> w;
    DCP_TRY(w.reserve(h, N, F));
    DCP_TRY(nmf_residual<T>(h, Y, mask, X, D, N, F, K, w.tmp, w.part, w.blocks));
    DCP_TRY(w.sum(h, out));
    *out = sqrt(*out);
    return DCP_OK;
}

// grads.py:108-125 / 143-160 on a minibatch: optional x update(s), then the two parts of the
// D gradient as explicit [K,F] arrays (what serizel.py / kasai.py accumulate and mix).
template <class T>
int nmf_grads_api(dcp_handle* h, const T* Y, const T* mask, T* X, const T* D, int64_t N, int64_t F,
                  int64_t K, int lik, int n_x_updates, T* grad_pos, T* grad_neg) {
    DCP_TRY(check_nmf_args(h, Y, X, D, N, F, K, lik));
    if (!grad_pos || !grad_neg) return fail(h, DCP_ERR_INVALID, "null gradient pointer");
    if (n_x_updates < 0) return fail(h, DCP_ERR_INVALID, "negative update count");
    DCP_HIP_OK(h, hipSetDevice(h->device));
    const bool masked = mask != nullptr;
    const bool gram = (lik == DCP_LIK_L2 && !masked);
    NmfShape<T> s{N, F, K, lik, masked};
    const int64_t W = nmf_stats_width(F, K, lik, masked);
    NmfStatsWs<T> ws;
    T* stats = nullptr;
    DCP_TRY(ws_lay_out(h, [&](WsLayout& a) {
        nmf_stats_layout(a, ws, s, masked);
        a.take(stats, (size_t)K * W);
    }));
    const T* Ypre = nullptr;
    DCP_TRY(nmf_premask<T>(h, Y, mask, N, F, ws.Ym, &Ypre));
    for (int i = 0; i < n_x_updates; ++i)
        DCP_TRY(nmf_stats<T>(h, Ypre, mask, X, X, D, s, stats, ws, 1));
    DCP_TRY(nmf_stats<T>(h, Ypre, mask, X, X, D, s, stats, ws, 2));
    // stats -> (pos, neg)
    DCP_HIP_OK(h, hipMemcpy2DAsync(grad_pos, sizeof(T) * F, stats, sizeof(T) * W, sizeof(T) * F, K,
                                   hipMemcpyDeviceToDevice, h->stream));
    if (gram) {   // neg = (x^T x) D
        GemmArgs<T> a;
        a.A = stats + F; a.lda = W; a.B = D; a.ldb = F; a.M = (int)K; a.N = (int)F; a.K = (int)K;
        a.tile = TILE_SMALL;
        DCP_LAUNCH_OK(h, (gemm<FORM_NN>(h->stream, a, EpiStore<T>{grad_neg, (long)F})));
    } else {
        DCP_HIP_OK(h, hipMemcpy2DAsync(grad_neg, sizeof(T) * F, stats + F, sizeof(T) * W,
                                       sizeof(T) * F, K, hipMemcpyDeviceToDevice, h->stream));
    }
    return DCP_OK;
}

// Gaussian / Poisson.grad_x (grads.py:108-115, 143-150): the two parts of the x gradient, [N, K] each.
template <class T>
int nmf_grad_x_api(dcp_handle* h, const T* Y, const T* mask, const T* X, const T* D, int64_t N, int64_t F,
                   int64_t K, int lik, T* grad_pos, T* grad_neg) {
    DCP_TRY(check_nmf_args(h, Y, X, D, N, F, K, lik));
    if (!grad_pos || !grad_neg) return fail(h, DCP_ERR_INVALID, "null gradient pointer");
    DCP_HIP_OK(h, hipSetDevice(h->device));
    const bool masked = mask != nullptr;
    NmfShape<T> s{N, F, K, lik, masked};
    NmfStatsWs<T> ws;
    DCP_TRY(ws_lay_out(h, [&](WsLayout& a) { nmf_stats_layout(a, ws, s, masked); }));
    const T* Ypre = nullptr;
    DCP_TRY(nmf_premask<T>(h, Y, mask, N, F, ws.Ym, &Ypre));
    return nmf_grad_x<T>(h, Ypre, mask, X, D, s, grad_pos, grad_neg, ws);
}

// Gaussian.logp (grads.py:127-135): sum((-0.5 ((y - x d) / scale)^2 - log(scale) - pi * 0.5) [* mask]).
template <class T>
int nmf_gauss_logp_api(dcp_handle* h, const T* Y, const T* mask, const T* X, const T* D, int64_t N,
                       int64_t F, int64_t K, double scale, double* out) {
    DCP_TRY(check_nmf_args(h, Y, X, D, N, F, K, DCP_LIK_L2));
    if (!out) return fail(h, DCP_ERR_INVALID, "out is null");
    DCP_HIP_OK(h, hipSetDevice(h->device));
    NmfScalarWs<T> w;
    DCP_TRY(w.reserve(h, N, F));
    GemmArgs<T> a;
    a.A = X; a.lda = K; a.B = D; a.ldb = F; a.M = (int)N; a.N = (int)F; a.K = (int)K;
    DCP_LAUNCH_OK(h, (gemm<FORM_NN>(h->stream, a, EpiResidual<T>{Y, F, nullptr, 0, w.tmp, F})));   // d = y - x D
    hipLaunchKernelGGL((reduce_partial_kernel<SumOp, MapGaussLogp<T>, double>), dim3(w.blocks), dim3(256), 0, h->stream,
                       MapGaussLogp<T>{w.tmp, mask, 1.0 / scale, log(scale) + 3.14159265358979323846 * 0.5},
                       (long)N * F, w.part);
    DCP_LAUNCH_OK(h, hipGetLastError());
    return w.sum(h, out);
}

// sum M o d_beta(Y | X D + 1e-15) with the handle's beta, to the host (accumulated in double).
template <class T>
int nmf_beta_divergence_api(dcp_handle* h, const T* Y, const T* mask, const T* X, const T* D, int64_t N,
                            int64_t F, int64_t K, double* out) {
    DCP_TRY(check_nmf_args(h, Y, X, D, N, F, K, DCP_LIK_BETA));
    if (!out) return fail(h, DCP_ERR_INVALID, "out is null");
    DCP_HIP_OK(h, hipSetDevice(h->device));
    NmfScalarWs<T> w;
    DCP_TRY(w.reserve(h, N, F));
    DCP_TRY(nmf_beta_divergence<T>(h, Y, mask, X, D, N, F, K, h->nmf_beta, w.tmp, w.part, w.blocks));
    return w.sum(h, out);
}

// D_new = l2_strict(rule(D, P, Q)) and max|D - D_new| (host):
//   alpha < 0 : D * max(P,0) / max(Q,eps)                         (grads.py:93)
//   alpha >= 0: max(D * ((1-alpha) + alpha * P / max(Q,eps)), 0)  (kasai.py:77-78)
template <class T>
__global__ void __launch_bounds__(256) nmf_rule_kernel(const T* __restrict__ D, const T* __restrict__ P,
                                                       const T* __restrict__ Q, long n, T alpha,
                                                       T* __restrict__ U) {
    for (long i = blockIdx.x * 256L + threadIdx.x; i < n; i += (long)gridDim.x * 256L) {
        const T q = max_np(Q[i], T(1.0e-15));
        T u;
        if (alpha < T(0)) {
            u = D[i] * max_np(P[i], T(0)) / q;
        } else {
            u = D[i] * ((T(1) - alpha) + alpha * P[i] / q);
            u = max_np(u, T(0));
        }
        U[i] = u;
    }
}

template <class T>
__global__ void __launch_bounds__(256) axpby_kernel(long n, T a, const T* x, T b, T* y) {
    // a zero coefficient means "do not read that operand" (BLAS semantics): y may be
    // uninitialised when b == 0, and 0 * NaN / 0 * Inf must not leak into the result.
    // x and y may alias (no __restrict__).
    for (long i = blockIdx.x * 256L + threadIdx.x; i < n; i += (long)gridDim.x * 256L) {
        T v;
        if (b == T(0)) v = (a == T(0)) ? T(0) : a * x[i];
        else if (a == T(0)) v = b * y[i];
        else v = a * x[i] + b * y[i];
        y[i] = v;
    }
}

template <class T>
int nmf_apply_api(dcp_handle* h, const T* D, const T* P, const T* Q, double alpha, T* D_new, int64_t K,
                  int64_t F, double* maxdiff) {
    if (!h) return DCP_ERR_INVALID;
    if (!D || !P || !Q || !D_new || !maxdiff) return fail(h, DCP_ERR_INVALID, "null pointer");
    if (K <= 0 || F <= 0) return fail(h, DCP_ERR_INVALID, "sizes must be positive");
    DCP_HIP_OK(h, hipSetDevice(h->device));
    NmfUpdateWs<T> wu;
    T* md = nullptr;
    DCP_TRY(ws_lay_out(h, [&](WsLayout& a) {
        nmf_update_layout(a, wu, F, K);
        a.take(md, 2);
    }));
    hipLaunchKernelGGL((nmf_rule_kernel<T>), dim3(grid_for(K * F)), dim3(256), 0, h->stream, D, P, Q,
                       (long)(K * F), (T)alpha, wu.U);
    DCP_HIP_OK(h, hipGetLastError());
    hipLaunchKernelGGL((row_normalize_kernel<T>), dim3((unsigned)K), dim3(256), 0, h->stream,
                       (const T*)wu.U, (long)F, (long)F, 1, D, (long)F, D_new, (long)F, wu.rowmax,
                       (T*)nullptr, (T*)nullptr, (T*)nullptr);
    DCP_HIP_OK(h, hipGetLastError());
    launch_final_max<T>(h->stream, wu.rowmax, (long)K, md);
    DCP_HIP_OK(h, hipGetLastError());
    return read_scalar(h, md, maxdiff);
}

template <class T>
int axpby_api(dcp_handle* h, int64_t n, double a, const T* x, double b, T* y) {
    if (!h) return DCP_ERR_INVALID;
    if (!x || !y) return fail(h, DCP_ERR_INVALID, "null pointer");
    if (n < 0) return fail(h, DCP_ERR_INVALID, "negative size");
    if (n == 0) return DCP_OK;
    DCP_HIP_OK(h, hipSetDevice(h->device));
    hipLaunchKernelGGL((axpby_kernel<T>), dim3(grid_for(n)), dim3(256), 0, h->stream, (long)n, (T)a, x,
                       (T)b, y);
    DCP_HIP_OK(h, hipGetLastError());
    return DCP_OK;
}

}  // namespace

extern "C" {

int dcp_nmf_grads_f32(dcp_handle* h, const float* Y, const float* mask, float* X, const float* D,
                      int64_t N, int64_t F, int64_t K, int likelihood, int n_x_updates,
                      float* grad_pos, float* grad_neg) {
    return nmf_grads_api<float>(h, Y, mask, X, D, N, F, K, likelihood, n_x_updates, grad_pos, grad_neg);
}
int dcp_nmf_grads_f64(dcp_handle* h, const double* Y, const double* mask, double* X, const double* D,
                      int64_t N, int64_t F, int64_t K, int likelihood, int n_x_updates,
                      double* grad_pos, double* grad_neg) {
    return nmf_grads_api<double>(h, Y, mask, X, D, N, F, K, likelihood, n_x_updates, grad_pos, grad_neg);
}
int dcp_nmf_grad_x_f32(dcp_handle* h, const float* Y, const float* mask, const float* X, const float* D,
                       int64_t N, int64_t F, int64_t K, int likelihood, float* grad_pos, float* grad_neg) {
    return nmf_grad_x_api<float>(h, Y, mask, X, D, N, F, K, likelihood, grad_pos, grad_neg);
}
int dcp_nmf_grad_x_f64(dcp_handle* h, const double* Y, const double* mask, const double* X, const double* D,
                       int64_t N, int64_t F, int64_t K, int likelihood, double* grad_pos, double* grad_neg) {
    return nmf_grad_x_api<double>(h, Y, mask, X, D, N, F, K, likelihood, grad_pos, grad_neg);
}
int dcp_nmf_gauss_logp_f32(dcp_handle* h, const float* Y, const float* mask, const float* X, const float* D,
                           int64_t N, int64_t F, int64_t K, double scale, double* out) {
    return nmf_gauss_logp_api<float>(h, Y, mask, X, D, N, F, K, scale, out);
}
int dcp_nmf_gauss_logp_f64(dcp_handle* h, const double* Y, const double* mask, const double* X, const double* D,
                           int64_t N, int64_t F, int64_t K, double scale, double* out) {
    return nmf_gauss_logp_api<double>(h, Y, mask, X, D, N, F, K, scale, out);
}
int dcp_set_nmf_beta(dcp_handle* h, double beta) {
    if (!h) return DCP_ERR_INVALID;
    if (!std::isfinite(beta)) return fail(h, DCP_ERR_INVALID, "beta must be finite");
    h->nmf_beta = beta;
    return DCP_OK;
}
int dcp_set_nmf_penalty(dcp_handle* h, double l1, double l2) {
    if (!h) return DCP_ERR_INVALID;
    if (!std::isfinite(l1) || !std::isfinite(l2) || l1 < 0.0 || l2 < 0.0)
        return fail(h, DCP_ERR_INVALID, "penalties must be finite and >= 0");
    h->nmf_l1 = l1;
    h->nmf_l2 = l2;
    return DCP_OK;
}
int dcp_nmf_beta_divergence_f32(dcp_handle* h, const float* Y, const float* mask, const float* X, const float* D,
                                int64_t N, int64_t F, int64_t K, double* out) {
    return nmf_beta_divergence_api<float>(h, Y, mask, X, D, N, F, K, out);
}
int dcp_nmf_beta_divergence_f64(dcp_handle* h, const double* Y, const double* mask, const double* X,
                                const double* D, int64_t N, int64_t F, int64_t K, double* out) {
    return nmf_beta_divergence_api<double>(h, Y, mask, X, D, N, F, K, out);
}
int dcp_nmf_apply_f32(dcp_handle* h, const float* D, const float* P, const float* Q, double alpha,
                      float* D_new, int64_t K, int64_t F, double* maxdiff) {
    return nmf_apply_api<float>(h, D, P, Q, alpha, D_new, K, F, maxdiff);
}
int dcp_nmf_apply_f64(dcp_handle* h, const double* D, const double* P, const double* Q, double alpha,
                      double* D_new, int64_t K, int64_t F, double* maxdiff) {
    return nmf_apply_api<double>(h, D, P, Q, alpha, D_new, K, F, maxdiff);
}
int dcp_axpby_f32(dcp_handle* h, int64_t n, double a, const float* x, double b, float* y) {
    return axpby_api<float>(h, n, a, x, b, y);
}
int dcp_axpby_f64(dcp_handle* h, int64_t n, double a, const double* x, double b, double* y) {
    return axpby_api<double>(h, n, a, x, b, y);
}

int64_t dcp_nmf_mu_stats_width(int64_t F, int64_t K, int likelihood, int masked) {
    return nmf_stats_width(F, K, likelihood, masked != 0);
}

int dcp_nmf_mu_f32(dcp_handle* h, const float* Y, const float* mask, float* X, float* D, int64_t N,
                   int64_t F, int64_t K, int likelihood, float tol, int maxiter, int* it_out,
                   float* last_maxdiff, float* resid_trace) {
    return nmf_mu_solve<float>(h, Y, mask, X, D, N, F, K, likelihood, tol, maxiter, it_out,
                               last_maxdiff, resid_trace);
}
int dcp_nmf_mu_f64(dcp_handle* h, const double* Y, const double* mask, double* X, double* D,
                   int64_t N, int64_t F, int64_t K, int likelihood, double tol, int maxiter,
                   int* it_out, double* last_maxdiff, double* resid_trace) {
    return nmf_mu_solve<double>(h, Y, mask, X, D, N, F, K, likelihood, tol, maxiter, it_out,
                                last_maxdiff, resid_trace);
}
int dcp_nmf_mu_sharded_f32(dcp_handle* h, const float* Y, const float* mask, float* X, float* D, int64_t N,
                           int64_t F, int64_t K, int likelihood, float tol, int maxiter, int* it_out,
                           float* last_maxdiff) {
    return nmf_mu_solve<float>(h, Y, mask, X, D, N, F, K, likelihood, tol, maxiter, it_out,
                               last_maxdiff, nullptr, true);
}
int dcp_nmf_mu_sharded_f64(dcp_handle* h, const double* Y, const double* mask, double* X, double* D,
                           int64_t N, int64_t F, int64_t K, int likelihood, double tol, int maxiter,
                           int* it_out, double* last_maxdiff) {
    return nmf_mu_solve<double>(h, Y, mask, X, D, N, F, K, likelihood, tol, maxiter, it_out,
                                last_maxdiff, nullptr, true);
}
int dcp_nmf_mu_stats_f32(dcp_handle* h, const float* Y, const float* mask, const float* X,
                         float* X_out, const float* D, int64_t N, int64_t F, int64_t K,
                         int likelihood, float* stats) {
    return nmf_mu_stats_api<float>(h, Y, mask, X, X_out, D, N, F, K, likelihood, stats);
}
int dcp_nmf_mu_stats_f64(dcp_handle* h, const double* Y, const double* mask, const double* X,
                         double* X_out, const double* D, int64_t N, int64_t F, int64_t K,
                         int likelihood, double* stats) {
    return nmf_mu_stats_api<double>(h, Y, mask, X, X_out, D, N, F, K, likelihood, stats);
}
int dcp_nmf_mask_prepare_f32(dcp_handle* h, const float* Y, const float* mask, int64_t N, int64_t F,
                             float* Ym, uint32_t* bits, int* binary) {
    return nmf_mask_prepare_api<float>(h, Y, mask, N, F, Ym, bits, binary);
}
int dcp_nmf_mask_prepare_f64(dcp_handle* h, const double* Y, const double* mask, int64_t N, int64_t F,
                             double* Ym, uint32_t* bits, int* binary) {
    return nmf_mask_prepare_api<double>(h, Y, mask, N, F, Ym, bits, binary);
}
int64_t dcp_nmf_mask_bits_words(int64_t N, int64_t F) { return (int64_t)mask_bits_words(N, F); }
int dcp_nmf_mu_stats_prepared_f32(dcp_handle* h, const float* Ym, const float* mask, const uint32_t* bits,
                                  const float* X, float* X_out, const float* D, int64_t N, int64_t F,
                                  int64_t K, int likelihood, float* stats) {
    return nmf_mu_stats_prepared_api<float>(h, Ym, mask, bits, X, X_out, D, N, F, K, likelihood, stats);
}
int dcp_nmf_mu_stats_prepared_f64(dcp_handle* h, const double* Ym, const double* mask, const uint32_t* bits,
                                  const double* X, double* X_out, const double* D, int64_t N, int64_t F,
                                  int64_t K, int likelihood, double* stats) {
    return nmf_mu_stats_prepared_api<double>(h, Ym, mask, bits, X, X_out, D, N, F, K, likelihood, stats);
}
int dcp_nmf_mu_update_f32(dcp_handle* h, const float* stats, const float* D, float* D_new,
                          int64_t F, int64_t K, int likelihood, int masked, float* maxdiff_dev,
                          float* maxdiff_next) {
    return nmf_mu_update_api<float>(h, stats, D, D_new, F, K, likelihood, masked, maxdiff_dev,
                                    maxdiff_next);
}
int dcp_nmf_mu_update_f64(dcp_handle* h, const double* stats, const double* D, double* D_new,
                          int64_t F, int64_t K, int likelihood, int masked, double* maxdiff_dev,
                          double* maxdiff_next) {
    return nmf_mu_update_api<double>(h, stats, D, D_new, F, K, likelihood, masked, maxdiff_dev,
                                     maxdiff_next);
}
int dcp_nmf_residual_f32(dcp_handle* h, const float* Y, const float* mask, const float* X,
                         const float* D, int64_t N, int64_t F, int64_t K, double* out) {
    return nmf_residual_api<float>(h, Y, mask, X, D, N, F, K, out);
}
int dcp_nmf_residual_f64(dcp_handle* h, const double* Y, const double* mask, const double* X,
                         const double* D, int64_t N, int64_t F, int64_t K, double* out) {
    return nmf_residual_api<double>(h, Y, mask, X, D, N, F, K, out);
}

}  // extern "C"
