// split_f16.h -- the one definition of the split-f16 arithmetic (the <= 1e-5 normwise contracts of
// include/ecorr.h), the static vmcnt wait and the vector types of the MFMA / buffer-builtin kernels.
// The build's operand pass (build.hip), the split convc1 and its weight pack (conv.hip) and the
// presplit column scale (lookup.hip) must agree on the exponent rule bit for bit: they all call
// split_exponent.  Device code only, gfx950.
#pragma once
#include <hip/hip_runtime.h>
#include <math.h>

#include "mfma_f32_frame.h"   // floatx16

namespace ecorr {

typedef float floatx4 __attribute__((ext_vector_type(4)));
typedef float floatx2 __attribute__((ext_vector_type(2)));
typedef _Float16 halfx8 __attribute__((ext_vector_type(8)));
typedef unsigned uint4v __attribute__((ext_vector_type(4)));
typedef unsigned uint2v __attribute__((ext_vector_type(2)));

// 2^e as a float, e in [-126, 127]
__device__ __forceinline__ float exp2i(int e) { return __int_as_float((e + 127) << 23); }

// s_waitcnt vmcnt(N) with lgkmcnt(0) (LGKM0) or left alone; expcnt never waited (gfx9 encoding:
// vmcnt bits 3:0 and 15:14)
template <int N, bool LGKM0 = false>
__device__ __forceinline__ void wait_vm() {
    static_assert(N >= 0 && N < 64, "vmcnt field");
    __builtin_amdgcn_s_waitcnt((N & 15) | ((N >> 4) << 14) | (7 << 4) | (LGKM0 ? 0 : (15 << 8)));
}

// The split exponent of a maximum m = f 2^E, f in [0.5, 1): e = 15 - E, so that m 2^e lies in
// [2^14, 2^15); 0 for a zero or non-finite maximum (NaN inputs then propagate as in the reference);
// clamped to what exp2i can represent.
__device__ __forceinline__ int split_exponent(float m) {
    int E = 0;
    frexpf(m, &E);
    const int e = (m > 0.f && m <= 3.4028235e38f) ? 15 - E : 0;
    return e < -126 ? -126 : (e > 126 ? 126 : e);
}

// x s = hi + lo + O(2^-22 |x s|): hi = f16(x s), lo = f16(x s - hi) (the subtraction is exact)
__device__ __forceinline__ void split_f16(const float (&v)[8], float s, halfx8& hi, halfx8& lo) {
#pragma unroll
    for (int j = 0; j < 8; ++j) {
        const float x = v[j] * s;
        const _Float16 h = (_Float16)x;
        hi[j] = h;
        lo[j] = (_Float16)(x - (float)h);
    }
}

}  // namespace ecorr
