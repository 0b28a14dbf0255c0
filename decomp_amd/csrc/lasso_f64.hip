// C ABI: dcp_lasso_*_f64 (see include/decomp_hip.h); the entries are DCP_LASSO_ABI in lasso_api.hpp.
#include "lasso_api.hpp"

DCP_DTYPE_f64(DCP_LASSO_ABI)
