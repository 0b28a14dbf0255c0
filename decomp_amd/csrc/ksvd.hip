// C ABI: dcp_ksvd_sweep_*, dcp_ksvd_step_* and dcp_ksvd_mask_sweep_*, dcp_ksvd_mask_step_*: one host path (ksvd.hpp)
// over the kernels of ksvd.hpp and, with a mask, of ksvd_mask.hpp; dcp_ksvd_clean_* and dcp_ksvd_clean_step_*: the
// cleaning pass of ksvd_clean.hpp alone and behind that same step; see include/decomp_hip.h.
#include "abi.hpp"
#include "ksvd.hpp"

#define DCP_KSVD_ABI(SFX, T, P, R)                                                                                   \
    extern "C" int dcp_ksvd_sweep_##SFX(dcp_handle* h, const P* Y, P* X, P* D, int64_t N, int64_t F, int64_t K,      \
                                        int row_nnz_max, double* maxdiff_out) {                                      \
        return dcp::ksvd_sweep_api<T>(h, (const T*)Y, nullptr, 0, false, (T*)X, (T*)D, N, F, K, row_nnz_max,         \
                                      maxdiff_out);                                                                  \
    }                                                                                                                \
    extern "C" int dcp_ksvd_step_##SFX(dcp_handle* h, const P* Y, P* X, P* D, int64_t N, int64_t F, int64_t K,       \
                                       int n_nonzero, double coef_tol, double* maxdiff_out, int* it_out) {           \
        return dcp::ksvd_step_api<T>(h, (const T*)Y, nullptr, 0, false, (T*)X, (T*)D, N, F, K, n_nonzero, coef_tol,  \
                                     0, maxdiff_out, it_out);                                                        \
    }                                                                                                                \
    extern "C" int dcp_ksvd_mask_sweep_##SFX(dcp_handle* h, const P* Y, const R* M, int mask_ndim, P* X, P* D,       \
                                             int64_t N, int64_t F, int64_t K, int row_nnz_max,                       \
                                             double* maxdiff_out) {                                                  \
        return dcp::ksvd_sweep_api<T>(h, (const T*)Y, M, mask_ndim, true, (T*)X, (T*)D, N, F, K, row_nnz_max,        \
                                      maxdiff_out);                                                                  \
    }                                                                                                                \
    extern "C" int dcp_ksvd_mask_step_##SFX(dcp_handle* h, const P* Y, const R* M, int mask_ndim, P* X, P* D,        \
                                            int64_t N, int64_t F, int64_t K, int n_nonzero, double coef_tol,         \
                                            int rows_per_pass, double* maxdiff_out, int* it_out) {                   \
        return dcp::ksvd_step_api<T>(h, (const T*)Y, M, mask_ndim, true, (T*)X, (T*)D, N, F, K, n_nonzero, coef_tol, \
                                     rows_per_pass, maxdiff_out, it_out);                                            \
    }                                                                                                                \
    extern "C" int dcp_ksvd_clean_##SFX(dcp_handle* h, const P* Y, const R* M, int mask_ndim, const P* X, P* D,      \
                                        int64_t N, int64_t F, int64_t K, double max_coherence, int* n_marked_out,    \
                                        int* n_replaced_out) {                                                       \
        return dcp::ksvd_clean_api<T>(h, (const T*)Y, M, mask_ndim, (const T*)X, (T*)D, N, F, K, max_coherence,      \
                                      n_marked_out, n_replaced_out);                                                 \
    }                                                                                                                \
    extern "C" int dcp_ksvd_clean_step_##SFX(dcp_handle* h, const P* Y, const R* M, int mask_ndim, P* X, P* D,       \
                                             int64_t N, int64_t F, int64_t K, int n_nonzero, double coef_tol,        \
                                             int rows_per_pass, double* maxdiff_out, int* it_out,                    \
                                             double max_coherence, double stop_tol, int* n_marked_out) {             \
        return dcp::ksvd_clean_step_api<T>(h, (const T*)Y, M, mask_ndim, (T*)X, (T*)D, N, F, K, n_nonzero, coef_tol, \
                                           rows_per_pass, maxdiff_out, it_out, max_coherence, stop_tol,              \
                                           n_marked_out);                                                            \
    }

DCP_FOR_EACH_DTYPE(DCP_KSVD_ABI)
