// lookup_half.hip -- ecorr_lookup_as's 16-bit outputs: the lookup kernels (lookup_kernels.h)
// instantiated for IEEE binary16 and bfloat16 elements, in a translation unit of their own (see
// lookup_kernels.h).
#include "lookup_kernels.h"

namespace ecorr {

// launch_lookup's paths and grids (lookup_kernels.h) with 2-byte elements; no qmax / presplit form
int launch_lookup_half(const LookupParams& P, int B, hipStream_t stream, int out_format) {
    if (out_format == ECORR_OUT_F16) return launch_lookup_plain<ECORR_OUT_F16>(P, B, stream);
    if (out_format == ECORR_OUT_BF16) return launch_lookup_plain<ECORR_OUT_BF16>(P, B, stream);
    return ECORR_EINVAL;
}

}  // namespace ecorr
