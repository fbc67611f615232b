// grad_slab.h -- the pixel slabs of the slab-split weight-gradient GEMMs (gru_grad.hip, motion_enc_grad.hip): one
// definition of the slab rule that both workspaces and both headers' formulas state.  Host code; constants only
// besides the function.
#pragma once
#include <stdint.h>

#include "mfma_f32_frame.h"

namespace ecorr {

constexpr int kGradWK = kFrameK;         // weight gradient: pixels per chunk
constexpr int kGradChain = 1024;         // ... and per first-level chain
constexpr int kGradSlabs = 64;           // the slab cap doubles while a launch would have more slabs than this

// slabs of the weight gradient's pixel reduction, within one batch item: a cap of 1024 pixels, doubled while
// the launch would have more than 64 slabs, then balanced slabs of whole chunks under the cap
inline void gru_grad_slab(int B, int HW, int* nsl, int* slab) {
    int64_t cap = kGradChain;
    while (cap < HW && (int64_t)B * ((HW + cap - 1) / cap) > kGradSlabs) cap *= 2;
    const int64_t per = (HW + cap - 1) / cap;
    *slab = (int)(((HW + per - 1) / per + kGradWK - 1) / kGradWK * kGradWK);
    *nsl = (HW + *slab - 1) / *slab;
}

}  // namespace ecorr
