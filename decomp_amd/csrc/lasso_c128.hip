// C ABI: dcp_lasso_*_c128 (see include/decomp_hip.h); the entries are DCP_LASSO_ABI in lasso_api.hpp.
#include "lasso_api.hpp"

DCP_DTYPE_c128(DCP_LASSO_ABI)
