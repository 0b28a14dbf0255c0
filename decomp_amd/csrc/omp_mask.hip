// C ABI: dcp_omp_mask_* (see include/decomp_hip.h; the kernels are omp_mask.hpp).
#include "abi.hpp"
#include "omp_mask.hpp"

#define DCP_OMP_MASK_ABI(SFX, T, P, R)                                                                               \
    extern "C" int dcp_omp_mask_##SFX(dcp_handle* h, const P* Y, const R* M, int mask_ndim, const P* A, P* X,        \
                                      int64_t N, int64_t F, int64_t K, int n_nonzero, double tol,                    \
                                      int rows_per_pass, int* it_out) {                                              \
        return dcp::omp_api<T>(h, (const T*)Y, M, mask_ndim, true, (const T*)A, (T*)X, N, F, K, n_nonzero, tol,      \
                               rows_per_pass, it_out);                                                               \
    }

DCP_FOR_EACH_DTYPE(DCP_OMP_MASK_ABI)
