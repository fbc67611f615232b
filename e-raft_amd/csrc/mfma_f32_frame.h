// mfma_f32_frame.h -- the one 256 x 64 fp32 GEMM frame on v_mfma_f32_32x32x2_f32: the workgroup of
// build_backward_kernel (grad.hip) and grad_weight_kernel (conv_grad.hip), and the C-fragment row
// of every 32 x 32 MFMA kernel.  A workgroup of 256 threads owns 256 rows (4 waves x 64) x 64
// columns, 2 x 2 tiles of 32 x 32 per wave; the reduction runs in chunks of 32 staged through LDS
// (A tile [256][33]; B tile [64][33] as [n][k], or [32][65] as [k][n]), the next chunk's global
// loads in flight under the current chunk's MFMAs.  Fragments: A lane (m, kh) = A[m][2 s + kh],
// B lane (n, kh) = B[n][2 s + kh], C register r of lane (n, kh) = row mfma_c_row(r, kh) of column n.
// A kernel supplies its addressing (load_chunk: global -> registers, store_chunk: registers -> LDS)
// and its epilogue, and runs ECORR_FRAME_K_LOOP between them.  Device code only; plain C++ apart from
// the MFMA builtin and the vector type, so tools/grad_emul.py compiles it on the CPU with grad.hip.
#pragma once
#include <hip/hip_runtime.h>

namespace ecorr {

typedef float floatx16 __attribute__((ext_vector_type(16)));

constexpr int kFrameM = 256;              // rows per workgroup (per pass)
constexpr int kFrameN = 64;               // columns per workgroup
constexpr int kFrameK = 32;               // reduction chunk
constexpr int kFrameLd = kFrameK + 1;     // row stride (floats) of a [row][k] tile
template <bool BKN> constexpr int kFrameBLd = BKN ? kFrameN + 1 : kFrameK + 1;   // B tile: [k][n] (BKN) or [n][k]

// row, within its 32 x 32 tile, of accumulator register r in a lane of half kh = lane >> 5; base: the
// tile's first row, the sum's first term (signed sums do not reassociate: added to the finished row
// instead, it costs grad_weight_kernel 32 instructions)
__device__ __forceinline__ int mfma_c_row(int r, int kh, int base = 0) {
    return base + (r & 3) + 8 * (r >> 2) + 4 * kh;
}

}  // namespace ecorr

// The frame's steps are macros, not __forceinline__ templates: through a call hipcc emits other
// instruction streams for both kernels (the K loop: 700 instructions and 16 VGPRs fewer in
// build_backward_kernel; the clear alone: other registers in grad_weight_kernel); as text they are the
// instructions they were (profiles/backward_frame/cpu_checks.txt).
//
// floatx16 acc[2][2] = 0
#define ECORR_FRAME_CLEAR(acc)                                                                                        \
    _Pragma("unroll") for (int i = 0; i < 2; ++i)                                                                     \
        _Pragma("unroll") for (int j = 0; j < 2; ++j)                                                                 \
            _Pragma("unroll") for (int r = 0; r < 16; ++r) (acc)[i][j][r] = 0.0f;

// acc += the staged chunk: 16 k pairs x (2 x 2) MFMAs, k ascending.  BKN: the B tile is [k][n].
#define ECORR_FRAME_MFMA_CHUNK(BKN, al, bl, lane, wave, acc)                                                          \
    {                                                                                                                 \
        const int m = (lane) & 31, kh = (lane) >> 5;                                                                  \
        _Pragma("unroll 4") for (int s = 0; s < ecorr::kFrameK / 2; ++s) {                                            \
            const int k = 2 * s + kh;                                                                                 \
            float a[2], bf[2];                                                                                        \
            _Pragma("unroll") for (int i = 0; i < 2; ++i) a[i] = (al)[(64 * (wave) + 32 * i + m) * ecorr::kFrameLd + k]; \
            _Pragma("unroll") for (int j = 0; j < 2; ++j)                                                             \
                bf[j] = (BKN) ? (bl)[k * ecorr::kFrameBLd<(BKN)> + 32 * j + m]                                        \
                              : (bl)[(32 * j + m) * ecorr::kFrameBLd<(BKN)> + k];                                     \
            _Pragma("unroll") for (int i = 0; i < 2; ++i)                                                             \
                _Pragma("unroll") for (int j = 0; j < 2; ++j)                                                         \
                    (acc)[i][j] = __builtin_amdgcn_mfma_f32_32x32x2f32(a[i], bf[j], (acc)[i][j], 0, 0, 0);            \
        }                                                                                                             \
    }

// The staged reduction: chunks 0 .. nchunks - 1 in order, two barriers per chunk.  load_chunk(kc):
// the kernel's global loads of chunk kc into registers; store_chunk(): those registers into al / bl.
#define ECORR_FRAME_K_LOOP(BKN, nchunks, al, bl, lane, wave, acc, load_chunk, store_chunk)                            \
    {                                                                                                                 \
        load_chunk(0);                                                                                                \
        for (int kc = 0; kc < (nchunks); ++kc) {                                                                      \
            __syncthreads(); /* the previous chunk's fragment reads are done */                                      \
            store_chunk();                                                                                            \
            __syncthreads();                                                                                          \
            if (kc + 1 < (nchunks)) load_chunk(kc + 1);                                                               \
            ECORR_FRAME_MFMA_CHUNK(BKN, al, bl, lane, wave, acc)                                                      \
        }                                                                                                             \
    }
