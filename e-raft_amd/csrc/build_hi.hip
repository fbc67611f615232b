// build_hi.hip -- the hi-only split build (ecorr_build_split_pack_hi_as / ecorr_build_split_gemm_hi):
// lo_flag_kernel, which records whether any lo half of the operand panels is non-zero, and for D =
// 241 .. 256 the two build_split16_hi_kernel -- in a translation unit of their own so that the
// instantiations they share with build_split16_kernel (the epilogue's lambdas) leave that kernel's
// instructions alone.
//
// The flag: the operand pass is the plain pack_both_kernel (build.hip), so the exponents and panels
// are its bytes; lo_flag_kernel then ORs the lo halves of all panels and stores 1 to the flag word
// (hi_flag: 256 bytes in front of the exponents; the entry zeroed it) where a magnitude bit is set.
// (Taking the bits inside the pass -- from its registers, or read back after its stores -- changed
// the instructions hipcc selects for the split itself, and with them the sign of the zero halves of
// a -0 element: v_fma_mixlo_f16 x, s, 0 gives hi = +0 where v_mul + v_cvt gives -0.)
//
// The GEMM: two kernels launched back to back on the same grid: TERMS = 1 sums hi*hi alone and TERMS
// = 3 is build_split16_kernel's loop.  Every block reads the flag word and the kernel the flag
// does not select returns at once -- flag 0: the one-term kernel builds the pyramid, flag != 0: the
// three-term kernel.  (Both loops in one kernel behind a branch did not fit two blocks per CU: 256
// VGPRs and 456 bytes of scratch per lane.)
//
// Why the pyramid is bitwise build_split16_kernel's either way: with every lo = +-0 and every hi
// finite, the lo*hi and hi*lo MFMAs add sums of +-0 to an accumulator that starts at +0, is never -0
// and never fp32-subnormal (a sum of multiples of 2^-48): acc + (+-0) = acc bit for bit, so both
// loops leave the same accumulators.  A non-finite operand makes its lo a NaN (inf - inf), which
// sets the flag.
#include "build_split16.h"

namespace ecorr {

namespace {

// The lo halves of n_groups 2-KB panel groups from `panels`: in both panel layouts (pack_body,
// build.hip) a group is [hi 1 KB | lo 1 KB].  A wave takes one group's lo KB per step (lane-linear
// 16-byte loads), four steps in flight; every thread that saw a magnitude bit stores the same 1.
__global__ __launch_bounds__(256) void lo_flag_kernel(const char* __restrict__ panels, int64_t n_groups,
                                                      int* __restrict__ flag) {
    const int lane = threadIdx.x & 63;
    const int64_t stride = (int64_t)gridDim.x * 4;
    unsigned bits = 0;
#pragma unroll 4
    for (int64_t g = (int64_t)blockIdx.x * 4 + (threadIdx.x >> 6); g < n_groups; g += stride) {
        const uint4v v = *reinterpret_cast<const uint4v*>(panels + g * 2048 + 1024 + lane * 16);
        bits |= v[0] | v[1] | v[2] | v[3];
    }
    if (bits & 0x7fff7fffu) *flag = 1;
}

template <bool MUL, int TERMS>
__global__ __launch_bounds__(256, 2) void build_split16_hi_kernel(BuildParams P) {
    if ((*hi_flag(P) != 0) != (TERMS == 3)) return;   // block-uniform (a scalar load): the other kernel's launch
#include "build_split16_loop.h"
}

}  // namespace

void launch_lo_flag(const char* panels, int64_t bytes, int* flag, hipStream_t stream) {
    const int64_t n_groups = bytes / 2048;   // whole groups: a panel is 8 KB
    const int64_t want = (n_groups + 3) / 4;
    const unsigned grid = (unsigned)(want < 2048 ? (want > 0 ? want : 1) : 2048);   // 8 blocks per CU, grid-stride
    hipLaunchKernelGGL(lo_flag_kernel, dim3(grid), dim3(256), 0, stream, panels, n_groups, flag);
}

void launch_split16_hi(const BuildParams& P, int64_t ntiles, hipStream_t stream) {
    const dim3 grid((unsigned)ntiles), block(256);
    hipLaunchKernelGGL((P.scale_is_mul ? build_split16_hi_kernel<true, 1> : build_split16_hi_kernel<false, 1>), grid,
                       block, 0, stream, P);
    hipLaunchKernelGGL((P.scale_is_mul ? build_split16_hi_kernel<true, 3> : build_split16_hi_kernel<false, 3>), grid,
                       block, 0, stream, P);
}

}  // namespace ecorr
