// C ABI: dcp_omp_mask_* (see include/decomp_hip.h; the kernels are omp_mask.hpp).
#include "omp_mask.hpp"

using dcp::c64;
using dcp::c128;

extern "C" int dcp_omp_mask_f32(dcp_handle* h, const float* Y, const float* M, int mask_ndim, const float* A, float* X,
                                int64_t N, int64_t F, int64_t K, int n_nonzero, double tol, int rows_per_pass,
                                int* it_out) {
    return dcp::omp_api<float>(h, Y, M, mask_ndim, true, A, X, N, F, K, n_nonzero, tol, rows_per_pass, it_out);
}
extern "C" int dcp_omp_mask_f64(dcp_handle* h, const double* Y, const double* M, int mask_ndim, const double* A,
                                double* X, int64_t N, int64_t F, int64_t K, int n_nonzero, double tol,
                                int rows_per_pass, int* it_out) {
    return dcp::omp_api<double>(h, Y, M, mask_ndim, true, A, X, N, F, K, n_nonzero, tol, rows_per_pass, it_out);
}
extern "C" int dcp_omp_mask_c64(dcp_handle* h, const void* Y, const float* M, int mask_ndim, const void* A, void* X,
                                int64_t N, int64_t F, int64_t K, int n_nonzero, double tol, int rows_per_pass,
                                int* it_out) {
    return dcp::omp_api<c64>(h, (const c64*)Y, M, mask_ndim, true, (const c64*)A, (c64*)X, N, F, K, n_nonzero, tol,
                             rows_per_pass, it_out);
}
extern "C" int dcp_omp_mask_c128(dcp_handle* h, const void* Y, const double* M, int mask_ndim, const void* A, void* X,
                                 int64_t N, int64_t F, int64_t K, int n_nonzero, double tol, int rows_per_pass,
                                 int* it_out) {
    return dcp::omp_api<c128>(h, (const c128*)Y, M, mask_ndim, true, (const c128*)A, (c128*)X, N, F, K, n_nonzero, tol,
                              rows_per_pass, it_out);
}
