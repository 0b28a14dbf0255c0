// C ABI: dcp_omp_* and dcp_omp_gram_* (see include/decomp_hip.h; the kernel is omp.hpp, the entry omp_mask.hpp).
#include "abi.hpp"
#include "omp_mask.hpp"

#define DCP_OMP_ABI(SFX, T, P, R)                                                                                    \
    extern "C" int dcp_omp_##SFX(dcp_handle* h, const P* Y, const P* A, P* X, int64_t N, int64_t F, int64_t K,       \
                                 int n_nonzero, double tol, int* it_out) {                                           \
        return dcp::omp_api<T>(h, (const T*)Y, nullptr, 0, false, (const T*)A, (T*)X, N, F, K, n_nonzero, tol, 0,    \
                               it_out);                                                                              \
    }                                                                                                                \
    extern "C" int dcp_omp_gram_##SFX(dcp_handle* h, const P* alpha0, const P* G, const R* ynorm2, P* X, int64_t N,  \
                                      int64_t K, int n_nonzero, double tol, int* it_out) {                           \
        return dcp::omp_gram_api<T>(h, (const T*)alpha0, (const T*)G, ynorm2, (T*)X, N, K, n_nonzero, tol, it_out);  \
    }

DCP_FOR_EACH_DTYPE(DCP_OMP_ABI)
