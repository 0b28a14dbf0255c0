// C ABI: dcp_lasso_*_c64 (see include/decomp_hip.h); the entries are DCP_LASSO_ABI in lasso_api.hpp.
#include "lasso_api.hpp"

DCP_DTYPE_c64(DCP_LASSO_ABI)
