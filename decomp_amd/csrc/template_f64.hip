// C ABI: dcp_tm_*_f64, structured template matching (see include/decomp_hip.h and template_impl.hpp;
// reference decomp/template_matching.py).
#include "template_impl.hpp"

DCP_DTYPE_f64(DCP_TM_ABI)
