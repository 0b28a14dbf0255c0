// C ABI: the dictionary-learning step, f64 (see include/decomp_hip.h); the entries are DCP_DICT_ABI in dict_api.hpp.
#include "dict_api.hpp"

DCP_DTYPE_f64(DCP_DICT_ABI)
