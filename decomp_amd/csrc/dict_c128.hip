// C ABI: the dictionary-learning step, c128 (see include/decomp_hip.h); the entries are DCP_DICT_ABI in dict_api.hpp.
#include "dict_api.hpp"

DCP_DTYPE_c128(DCP_DICT_ABI)
