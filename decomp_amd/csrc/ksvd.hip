// C ABI: dcp_ksvd_sweep_*, dcp_ksvd_step_* and dcp_ksvd_mask_sweep_*, dcp_ksvd_mask_step_*: one host path (ksvd.hpp)
// over the kernels of ksvd.hpp and, with a mask, of ksvd_mask.hpp; dcp_ksvd_clean_* and dcp_ksvd_clean_step_*: the
// cleaning pass of ksvd_clean.hpp alone and behind that same step; see include/decomp_hip.h.
#include "ksvd.hpp"

using dcp::c64;
using dcp::c128;

extern "C" int dcp_ksvd_sweep_f32(dcp_handle* h, const float* Y, float* X, float* D, int64_t N, int64_t F, int64_t K,
                                  int row_nnz_max, double* maxdiff_out) {
    return dcp::ksvd_sweep_api<float>(h, Y, nullptr, 0, false, X, D, N, F, K, row_nnz_max, maxdiff_out);
}
extern "C" int dcp_ksvd_sweep_f64(dcp_handle* h, const double* Y, double* X, double* D, int64_t N, int64_t F, int64_t K,
                                  int row_nnz_max, double* maxdiff_out) {
    return dcp::ksvd_sweep_api<double>(h, Y, nullptr, 0, false, X, D, N, F, K, row_nnz_max, maxdiff_out);
}
extern "C" int dcp_ksvd_sweep_c64(dcp_handle* h, const void* Y, void* X, void* D, int64_t N, int64_t F, int64_t K,
                                  int row_nnz_max, double* maxdiff_out) {
    return dcp::ksvd_sweep_api<c64>(h, (const c64*)Y, nullptr, 0, false, (c64*)X, (c64*)D, N, F, K, row_nnz_max,
                                    maxdiff_out);
}
extern "C" int dcp_ksvd_sweep_c128(dcp_handle* h, const void* Y, void* X, void* D, int64_t N, int64_t F, int64_t K,
                                   int row_nnz_max, double* maxdiff_out) {
    return dcp::ksvd_sweep_api<c128>(h, (const c128*)Y, nullptr, 0, false, (c128*)X, (c128*)D, N, F, K, row_nnz_max,
                                     maxdiff_out);
}
extern "C" int dcp_ksvd_step_f32(dcp_handle* h, const float* Y, float* X, float* D, int64_t N, int64_t F, int64_t K,
                                 int n_nonzero, double coef_tol, double* maxdiff_out, int* it_out) {
    return dcp::ksvd_step_api<float>(h, Y, nullptr, 0, false, X, D, N, F, K, n_nonzero, coef_tol, 0, maxdiff_out,
                                     it_out);
}
extern "C" int dcp_ksvd_step_f64(dcp_handle* h, const double* Y, double* X, double* D, int64_t N, int64_t F, int64_t K,
                                 int n_nonzero, double coef_tol, double* maxdiff_out, int* it_out) {
    return dcp::ksvd_step_api<double>(h, Y, nullptr, 0, false, X, D, N, F, K, n_nonzero, coef_tol, 0, maxdiff_out,
                                      it_out);
}
extern "C" int dcp_ksvd_step_c64(dcp_handle* h, const void* Y, void* X, void* D, int64_t N, int64_t F, int64_t K,
                                 int n_nonzero, double coef_tol, double* maxdiff_out, int* it_out) {
    return dcp::ksvd_step_api<c64>(h, (const c64*)Y, nullptr, 0, false, (c64*)X, (c64*)D, N, F, K, n_nonzero, coef_tol,
                                   0, maxdiff_out, it_out);
}
extern "C" int dcp_ksvd_step_c128(dcp_handle* h, const void* Y, void* X, void* D, int64_t N, int64_t F, int64_t K,
                                  int n_nonzero, double coef_tol, double* maxdiff_out, int* it_out) {
    return dcp::ksvd_step_api<c128>(h, (const c128*)Y, nullptr, 0, false, (c128*)X, (c128*)D, N, F, K, n_nonzero,
                                    coef_tol, 0, maxdiff_out, it_out);
}
extern "C" int dcp_ksvd_mask_sweep_f32(dcp_handle* h, const float* Y, const float* M, int mask_ndim, float* X, float* D,
                                       int64_t N, int64_t F, int64_t K, int row_nnz_max, double* maxdiff_out) {
    return dcp::ksvd_sweep_api<float>(h, Y, M, mask_ndim, true, X, D, N, F, K, row_nnz_max, maxdiff_out);
}
extern "C" int dcp_ksvd_mask_sweep_f64(dcp_handle* h, const double* Y, const double* M, int mask_ndim, double* X, double* D,
                                       int64_t N, int64_t F, int64_t K, int row_nnz_max, double* maxdiff_out) {
    return dcp::ksvd_sweep_api<double>(h, Y, M, mask_ndim, true, X, D, N, F, K, row_nnz_max, maxdiff_out);
}
extern "C" int dcp_ksvd_mask_sweep_c64(dcp_handle* h, const void* Y, const float* M, int mask_ndim, void* X, void* D,
                                       int64_t N, int64_t F, int64_t K, int row_nnz_max, double* maxdiff_out) {
    return dcp::ksvd_sweep_api<c64>(h, (const c64*)Y, M, mask_ndim, true, (c64*)X, (c64*)D, N, F, K, row_nnz_max,
                                    maxdiff_out);
}
extern "C" int dcp_ksvd_mask_sweep_c128(dcp_handle* h, const void* Y, const double* M, int mask_ndim, void* X, void* D,
                                        int64_t N, int64_t F, int64_t K, int row_nnz_max, double* maxdiff_out) {
    return dcp::ksvd_sweep_api<c128>(h, (const c128*)Y, M, mask_ndim, true, (c128*)X, (c128*)D, N, F, K, row_nnz_max,
                                     maxdiff_out);
}
extern "C" int dcp_ksvd_mask_step_f32(dcp_handle* h, const float* Y, const float* M, int mask_ndim, float* X, float* D,
                                      int64_t N, int64_t F, int64_t K, int n_nonzero, double coef_tol, int rows_per_pass,
                                      double* maxdiff_out, int* it_out) {
    return dcp::ksvd_step_api<float>(h, Y, M, mask_ndim, true, X, D, N, F, K, n_nonzero, coef_tol, rows_per_pass,
                                     maxdiff_out, it_out);
}
extern "C" int dcp_ksvd_mask_step_f64(dcp_handle* h, const double* Y, const double* M, int mask_ndim, double* X, double* D,
                                      int64_t N, int64_t F, int64_t K, int n_nonzero, double coef_tol, int rows_per_pass,
                                      double* maxdiff_out, int* it_out) {
    return dcp::ksvd_step_api<double>(h, Y, M, mask_ndim, true, X, D, N, F, K, n_nonzero, coef_tol, rows_per_pass,
                                      maxdiff_out, it_out);
}
extern "C" int dcp_ksvd_mask_step_c64(dcp_handle* h, const void* Y, const float* M, int mask_ndim, void* X, void* D,
                                      int64_t N, int64_t F, int64_t K, int n_nonzero, double coef_tol, int rows_per_pass,
                                      double* maxdiff_out, int* it_out) {
    return dcp::ksvd_step_api<c64>(h, (const c64*)Y, M, mask_ndim, true, (c64*)X, (c64*)D, N, F, K, n_nonzero, coef_tol,
                                   rows_per_pass, maxdiff_out, it_out);
}
extern "C" int dcp_ksvd_mask_step_c128(dcp_handle* h, const void* Y, const double* M, int mask_ndim, void* X, void* D,
                                       int64_t N, int64_t F, int64_t K, int n_nonzero, double coef_tol, int rows_per_pass,
                                       double* maxdiff_out, int* it_out) {
    return dcp::ksvd_step_api<c128>(h, (const c128*)Y, M, mask_ndim, true, (c128*)X, (c128*)D, N, F, K, n_nonzero,
                                    coef_tol, rows_per_pass, maxdiff_out, it_out);
}
extern "C" int dcp_ksvd_clean_f32(dcp_handle* h, const float* Y, const float* M, int mask_ndim, const float* X,
                                  float* D, int64_t N, int64_t F, int64_t K, double max_coherence, int* n_marked_out,
                                  int* n_replaced_out) {
    return dcp::ksvd_clean_api<float>(h, Y, M, mask_ndim, X, D, N, F, K, max_coherence, n_marked_out, n_replaced_out);
}
extern "C" int dcp_ksvd_clean_f64(dcp_handle* h, const double* Y, const double* M, int mask_ndim, const double* X,
                                  double* D, int64_t N, int64_t F, int64_t K, double max_coherence, int* n_marked_out,
                                  int* n_replaced_out) {
    return dcp::ksvd_clean_api<double>(h, Y, M, mask_ndim, X, D, N, F, K, max_coherence, n_marked_out,
                                       n_replaced_out);
}
extern "C" int dcp_ksvd_clean_c64(dcp_handle* h, const void* Y, const float* M, int mask_ndim, const void* X, void* D,
                                  int64_t N, int64_t F, int64_t K, double max_coherence, int* n_marked_out,
                                  int* n_replaced_out) {
    return dcp::ksvd_clean_api<c64>(h, (const c64*)Y, M, mask_ndim, (const c64*)X, (c64*)D, N, F, K, max_coherence,
                                    n_marked_out, n_replaced_out);
}
extern "C" int dcp_ksvd_clean_c128(dcp_handle* h, const void* Y, const double* M, int mask_ndim, const void* X,
                                   void* D, int64_t N, int64_t F, int64_t K, double max_coherence, int* n_marked_out,
                                   int* n_replaced_out) {
    return dcp::ksvd_clean_api<c128>(h, (const c128*)Y, M, mask_ndim, (const c128*)X, (c128*)D, N, F, K,
                                     max_coherence, n_marked_out, n_replaced_out);
}
extern "C" int dcp_ksvd_clean_step_f32(dcp_handle* h, const float* Y, const float* M, int mask_ndim, float* X,
                                       float* D, int64_t N, int64_t F, int64_t K, int n_nonzero, double coef_tol,
                                       int rows_per_pass, double* maxdiff_out, int* it_out, double max_coherence,
                                       double stop_tol, int* n_marked_out) {
    const dcp::KsvdCleanCall clean{max_coherence, stop_tol, n_marked_out};
    return dcp::ksvd_step_api<float>(h, Y, M, mask_ndim, M != nullptr || mask_ndim != 0, X, D, N, F, K, n_nonzero,
                                     coef_tol, rows_per_pass, maxdiff_out, it_out, &clean);
}
extern "C" int dcp_ksvd_clean_step_f64(dcp_handle* h, const double* Y, const double* M, int mask_ndim, double* X,
                                       double* D, int64_t N, int64_t F, int64_t K, int n_nonzero, double coef_tol,
                                       int rows_per_pass, double* maxdiff_out, int* it_out, double max_coherence,
                                       double stop_tol, int* n_marked_out) {
    const dcp::KsvdCleanCall clean{max_coherence, stop_tol, n_marked_out};
    return dcp::ksvd_step_api<double>(h, Y, M, mask_ndim, M != nullptr || mask_ndim != 0, X, D, N, F, K, n_nonzero,
                                      coef_tol, rows_per_pass, maxdiff_out, it_out, &clean);
}
extern "C" int dcp_ksvd_clean_step_c64(dcp_handle* h, const void* Y, const float* M, int mask_ndim, void* X, void* D,
                                       int64_t N, int64_t F, int64_t K, int n_nonzero, double coef_tol,
                                       int rows_per_pass, double* maxdiff_out, int* it_out, double max_coherence,
                                       double stop_tol, int* n_marked_out) {
    const dcp::KsvdCleanCall clean{max_coherence, stop_tol, n_marked_out};
    return dcp::ksvd_step_api<c64>(h, (const c64*)Y, M, mask_ndim, M != nullptr || mask_ndim != 0, (c64*)X, (c64*)D,
                                   N, F, K, n_nonzero, coef_tol, rows_per_pass, maxdiff_out, it_out, &clean);
}
extern "C" int dcp_ksvd_clean_step_c128(dcp_handle* h, const void* Y, const double* M, int mask_ndim, void* X,
                                        void* D, int64_t N, int64_t F, int64_t K, int n_nonzero, double coef_tol,
                                        int rows_per_pass, double* maxdiff_out, int* it_out, double max_coherence,
                                        double stop_tol, int* n_marked_out) {
    const dcp::KsvdCleanCall clean{max_coherence, stop_tol, n_marked_out};
    return dcp::ksvd_step_api<c128>(h, (const c128*)Y, M, mask_ndim, M != nullptr || mask_ndim != 0, (c128*)X,
                                    (c128*)D, N, F, K, n_nonzero, coef_tol, rows_per_pass, maxdiff_out, it_out,
                                    &clean);
}
