// out_elem.h -- the one definition of a kernel's 16-bit (or fp32) output element and of a 16-bit
// operand element, for every translation unit that stores or loads one: the lookups
// (lookup_kernels.h: ecorr_lookup_as), the split convc1 (conv.hip: ecorr_conv1x1_relu_split_as), the
// fused lookup + convc1 (motion.hip: ecorr_lookup_conv1x1_relu_packed_as) and the split build's
// operand pass (build.hip: ecorr_build_split_pack_as).  Device code, gfx950.
#pragma once
#include "ecorr_device.h"
#include "ecorr_internal.h"

namespace ecorr {

// The output element (include/ecorr.h): FMT = ECORR_OUT_F32 stores the fp32 value itself;
// ECORR_OUT_F16 / ECORR_OUT_BF16 store it rounded once to nearest-even as a 2-byte bit pattern --
// f16: the hardware convert of the fp32 value (overflow -> +-inf, subnormals kept); bf16: NaN stays
// NaN.  The element order of the output is the same, so every offset scales by the element size.
template <int FMT>
struct OutElem {
    static_assert(FMT == ECORR_OUT_F16 || FMT == ECORR_OUT_BF16, "unknown output format");
    using type = unsigned short;
};
template <>
struct OutElem<ECORR_OUT_F32> {
    using type = float;
};
template <int FMT>
__device__ __forceinline__ typename OutElem<FMT>::type out_elem(float v) {
    if constexpr (FMT == ECORR_OUT_F16) {
        // the value as an fp32 register first: without this the compiler folds the last fp32 operation
        // in front (the lookup blend's last fma, a conv's bias add) into the convert
        // (v_fma_mixlo_f16), which rounds the unrounded result -- once, but not the fp32 value: it
        // differs from the fp32 entry's value cast to f16 wherever that value is an exact tie
        asm("" : "+v"(v));
        return __builtin_bit_cast(unsigned short, (_Float16)v);
    }
    else if constexpr (FMT == ECORR_OUT_BF16)
        return __builtin_bit_cast(unsigned short, (__bf16)v);
    else
        return v;
}
// ... and its buffer store at voff + soff (bytes) of rsrc: one dword, or one 2-byte element
template <int FMT, int AUX>
__device__ __forceinline__ void store_out(float v, __amdgpu_buffer_rsrc_t rsrc, int voff, int soff) {
    if constexpr (FMT == ECORR_OUT_F32)
        __builtin_amdgcn_raw_buffer_store_b32(__float_as_uint(v), rsrc, voff, soff, AUX);
    else
        __builtin_amdgcn_raw_buffer_store_b16((short)out_elem<FMT>(v), rsrc, voff, soff, AUX);
}

// The operand element of a kernel that reads fp32, binary16 or bfloat16 values (ECORR_ELEM_*): the
// conversion to fp32 on load is exact in every case.
template <int FMT>
struct InElem {
    static_assert(FMT == ECORR_ELEM_BF16, "unknown element format");
    using type = __bf16;
};
template <>
struct InElem<ECORR_ELEM_F32> {
    using type = float;
};
template <>
struct InElem<ECORR_ELEM_F16> {
    using type = _Float16;
};

}  // namespace ecorr
