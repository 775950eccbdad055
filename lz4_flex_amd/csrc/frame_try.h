// frame_try.h -- how frame_many.cpp and frame_index.cpp leave a function of the C ABI early: a HIP error as the ABI's code, a failed
// inner call's code as it is.  (sharded.cpp has variants of its own that say which call failed.)
#pragma once
#include <hip/hip_runtime.h>

#include "../../include/lz4flex_amd.h"

#define TRY_HIP(expr)                                                        \
    do {                                                                     \
        const hipError_t e_ = (expr);                                        \
        if (e_ != hipSuccess) return e_ == hipErrorOutOfMemory ? -LZ4FLEX_E_NOMEM : -LZ4FLEX_E_HIP; \
    } while (0)
#define TRY_RC(expr)                   \
    do {                               \
        const int rc_ = (expr);        \
        if (rc_) return rc_;           \
    } while (0)
