// The dtypes of the C ABI (include/decomp_hip.h), listed once.  A family of entry points that exists in all four is
// defined once, as a macro over one row of this list, and that macro only forwards: the extern "C" signature, the
// element pointers cast to T*, one call of a dcp::..._api<T> template.  Checks and launches live in that template.
// The header stays spelled out by hand and is included by every translation unit, so the compiler rejects a row
// or a family macro that disagrees with it.
//
// A row is X(SFX, T, P, R):
//   SFX  the suffix of the entry point's name
//   T    the element type the templates take
//   P    the pointee the C signature shows for an element pointer (complex data crosses the ABI as void*; the
//        dcp_tm_* families show void* in every dtype and do not use P)
//   R    the real type: masks, norms, device scalars
#pragma once
#include "scalar.hpp"

#define DCP_DTYPE_f32(X) X(f32, float, float, float)
#define DCP_DTYPE_f64(X) X(f64, double, double, double)
#define DCP_DTYPE_c64(X) X(c64, dcp::c64, void, float)
#define DCP_DTYPE_c128(X) X(c128, dcp::c128, void, double)

#define DCP_FOR_EACH_DTYPE(X) DCP_DTYPE_f32(X) DCP_DTYPE_f64(X) DCP_DTYPE_c64(X) DCP_DTYPE_c128(X)
