// motion_enc_shape.h -- the sizes and the weight-pack extents of the motion encoder kernels (motion_enc.hip).
// Device and host; constants only.
#pragma once
#include <stdint.h>

#include "gru_shape.h"   // f32x4, f32x16

namespace ecorr {

constexpr int MEC1 = 256;          // channels of c1 = relu(convc1(corr)): convc2's input
constexpr int MECOR = 192;         // convc2's outputs (cor)
constexpr int MEF1 = 128;          // convf1's outputs (f1)
constexpr int MEFLO = 64;          // convf2's outputs (flo)
constexpr int MECONV = 126;        // conv's outputs
constexpr int MEOUT = 128;         // output channels: conv's 126, then the 2 of flow
constexpr int MET = 9;             // taps of a 3x3 kernel, t = 3 ky + kx
constexpr int MEKC = 16;           // channels per chunk (8 k-steps of v_mfma_f32_32x32x2_f32)
constexpr int MEFL = 12;           // chunks per first-level fmaf chain (192 products)
constexpr int MENT = 256;          // threads (4 waves)
constexpr int MEF1R = 3;           // convf1's reach (7x7)
constexpr int MEF1K = 2 * 7 * 7;   // convf1's K: 98
constexpr int MEF1LD = 100;        // ... and its packed row length (25 x 16 bytes; the last two floats are 0)
static_assert(MECOR % MEKC == 0 && (MET * MEC1 / MEKC) % MEFL == 0 && (MET * MEF1 / MEKC) % MEFL == 0,
              "a chunk reads one tensor; whole chains");

// packed floats: the three tap-GEMM matrices (MET * C / MEKC chunks of M * MEKC floats), convf1's rows, the biases
constexpr int64_t kMeC2Floats = (int64_t)MET * MEC1 * MECOR;             // convc2: M = 192, C = 256
constexpr int64_t kMeF2Floats = (int64_t)MET * MEF1 * MEFLO;             // convf2: M = 64, C = 128
constexpr int64_t kMeCvFloats = (int64_t)MET * (MECOR + MEFLO) * MEOUT;  // conv: M = 128 (126 and two zero rows), C = 256
constexpr int64_t kMeF1Floats = (int64_t)MEF1 * MEF1LD;                  // convf1: [128][100]
constexpr int64_t kMeC2At = 0, kMeF2At = kMeC2At + kMeC2Floats, kMeCvAt = kMeF2At + kMeF2Floats,
                  kMeF1At = kMeCvAt + kMeCvFloats, kMeBiasAt = kMeF1At + kMeF1Floats;
// biases: convc2 [192], convf1 [128], convf2 [64], conv [128] (the last two 0)
constexpr int kMeBiasC2 = 0, kMeBiasF1 = MECOR, kMeBiasF2 = MECOR + MEF1, kMeBiasCv = MECOR + MEF1 + MEFLO;
constexpr int kMeBiasFloats = kMeBiasCv + MEOUT;
constexpr int64_t kMePackFloats = kMeBiasAt + kMeBiasFloats;
static_assert(kMeF2At % 4 == 0 && kMeCvAt % 4 == 0 && kMeF1At % 4 == 0 && kMePackFloats % 4 == 0, "16-byte pieces");

// The backward (motion_enc_grad.hip).  The transposed, tap-flipped pack: conv^T (256 rows [cor | flo], K = 9 x 128:
// go's 126 rows and two zero rows), convc2^T (256 rows, K = 9 x 192), convf2^T (128 rows, K = 9 x 64); a matrix is
// rows / 128 row groups of 9 K / 16 chunks (tap-major) of 128 x 16 floats.  convf1 has no transposed pack: its data
// gradient reads the forward pack's rows.
constexpr int MEDR = 128;                          // rows per workgroup (and row group) of a data gradient
constexpr int MEDCH = MEDR * MEKC;                 // floats of one (row group, chunk)
constexpr int64_t kMeTCvFloats = (int64_t)MET * (MECOR + MEFLO) * MEOUT;   // 2 x 72 chunks
constexpr int64_t kMeTC2Floats = (int64_t)MET * MEC1 * MECOR;              // 2 x 108 chunks
constexpr int64_t kMeTF2Floats = (int64_t)MET * MEF1 * MEFLO;              // 36 chunks
constexpr int64_t kMeTCvAt = 0, kMeTC2At = kMeTCvAt + kMeTCvFloats, kMeTF2At = kMeTC2At + kMeTC2Floats;
constexpr int64_t kMePackTFloats = kMeTF2At + kMeTF2Floats;
static_assert((MET * MEOUT / MEKC) % MEFL == 0 && (MET * MECOR / MEKC) % MEFL == 0 && (MET * MEFLO / MEKC) % MEFL == 0,
              "whole chains of the forward's length in every data gradient");
// bias partials: per (batch item, 64-pixel block) one sum per channel of go [128] | gc2 [192] | gf2 [64] | gf1 [128]
constexpr int kMeGbGo = 0, kMeGbC2 = MEOUT, kMeGbF2 = MEOUT + MECOR, kMeGbF1 = MEOUT + MECOR + MEFLO;
constexpr int MEGB = kMeGbF1 + MEF1;               // 512
// the largest weight gradient (convc2's): floats of one slab's partial; the four gradients take turns in it
constexpr int64_t kMeWPartFloats = (int64_t)MECOR * MEC1 * MET;

}  // namespace ecorr
