// gru_shape.h -- the sizes and the weight-pack extents of the SepConvGRU kernels: gru.hip (forward and the
// backward's gate recompute) and gru_grad.hip (backward).  Device and host; constants only.
#pragma once
#include <stdint.h>

namespace ecorr {

constexpr int GH = 128;            // hidden channels
constexpr int GX = 256;            // input channels
constexpr int GC = GH + GX;        // K channels per tap
constexpr int GT = 5;              // taps
constexpr int GKC = 16;            // channels per chunk (8 k-steps of v_mfma_f32_32x32x2_f32)
constexpr int GNC = GC / GKC;      // chunks per tap
constexpr int GNK = GT * GNC;      // chunks per GEMM
constexpr int GFL = 12;            // chunks per first-level fmaf chain (192 products)
constexpr int GNT = 256;           // threads (4 waves)
static_assert(GNK % GFL == 0 && GH % GKC == 0, "whole chains; a chunk reads one tensor");

constexpr int64_t kZrFloats = (int64_t)GNK * 2 * GH * GKC;   // packed floats of a z|r matrix (256 rows)
constexpr int64_t kQFloats = (int64_t)GNK * GH * GKC;        // and of a q matrix (128 rows)
constexpr int64_t kHalfFloats = kZrFloats + kQFloats;        // one half-step: z|r then q
constexpr int64_t kPackFloats = 2 * kHalfFloats;             // then the 6 x 128 biases

typedef float f32x16 __attribute__((ext_vector_type(16)));
typedef float f32x4 __attribute__((ext_vector_type(4)));

}  // namespace ecorr
