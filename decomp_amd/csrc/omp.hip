// C ABI: dcp_omp_* and dcp_omp_gram_* (see include/decomp_hip.h; the kernel is omp.hpp, the entry omp_mask.hpp).
#include "omp_mask.hpp"

using dcp::c64;
using dcp::c128;

extern "C" int dcp_omp_f32(dcp_handle* h, const float* Y, const float* A, float* X, int64_t N, int64_t F, int64_t K,
                           int n_nonzero, double tol, int* it_out) {
    return dcp::omp_api<float>(h, Y, nullptr, 0, false, A, X, N, F, K, n_nonzero, tol, 0, it_out);
}
extern "C" int dcp_omp_f64(dcp_handle* h, const double* Y, const double* A, double* X, int64_t N, int64_t F,
                           int64_t K, int n_nonzero, double tol, int* it_out) {
    return dcp::omp_api<double>(h, Y, nullptr, 0, false, A, X, N, F, K, n_nonzero, tol, 0, it_out);
}
extern "C" int dcp_omp_c64(dcp_handle* h, const void* Y, const void* A, void* X, int64_t N, int64_t F, int64_t K,
                           int n_nonzero, double tol, int* it_out) {
    return dcp::omp_api<c64>(h, (const c64*)Y, nullptr, 0, false, (const c64*)A, (c64*)X, N, F, K, n_nonzero, tol, 0,
                             it_out);
}
extern "C" int dcp_omp_c128(dcp_handle* h, const void* Y, const void* A, void* X, int64_t N, int64_t F, int64_t K,
                            int n_nonzero, double tol, int* it_out) {
    return dcp::omp_api<c128>(h, (const c128*)Y, nullptr, 0, false, (const c128*)A, (c128*)X, N, F, K, n_nonzero, tol,
                              0, it_out);
}

extern "C" int dcp_omp_gram_f32(dcp_handle* h, const float* alpha0, const float* G, const float* ynorm2, float* X,
                                int64_t N, int64_t K, int n_nonzero, double tol, int* it_out) {
    return dcp::omp_gram_api<float>(h, alpha0, G, ynorm2, X, N, K, n_nonzero, tol, it_out);
}
extern "C" int dcp_omp_gram_f64(dcp_handle* h, const double* alpha0, const double* G, const double* ynorm2, double* X,
                                int64_t N, int64_t K, int n_nonzero, double tol, int* it_out) {
    return dcp::omp_gram_api<double>(h, alpha0, G, ynorm2, X, N, K, n_nonzero, tol, it_out);
}
extern "C" int dcp_omp_gram_c64(dcp_handle* h, const void* alpha0, const void* G, const float* ynorm2, void* X,
                                int64_t N, int64_t K, int n_nonzero, double tol, int* it_out) {
    return dcp::omp_gram_api<c64>(h, (const c64*)alpha0, (const c64*)G, ynorm2, (c64*)X, N, K, n_nonzero, tol, it_out);
}
extern "C" int dcp_omp_gram_c128(dcp_handle* h, const void* alpha0, const void* G, const double* ynorm2, void* X,
                                 int64_t N, int64_t K, int n_nonzero, double tol, int* it_out) {
    return dcp::omp_gram_api<c128>(h, (const c128*)alpha0, (const c128*)G, ynorm2, (c128*)X, N, K, n_nonzero, tol,
                                   it_out);
}
