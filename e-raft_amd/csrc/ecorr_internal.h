// ecorr_internal.h -- host-side launch interfaces between abi.hip and the kernel files.
#pragma once
#include <hip/hip_runtime.h>
#include <stdint.h>

#include "../../include/ecorr.h"

namespace ecorr {

// The status every launch_* returns after its launches: the runtime's last error as an ECORR code.
inline int hip_status() {
    const hipError_t e = hipGetLastError();
    return e == hipSuccess ? ECORR_OK : ECORR_EHIP - (int)e;
}

// Pyramid storage geometry (include/ecorr.h), computed once by pyramid_geometry() (abi.hip) and
// shared by the build and the lookup.
struct PyrGeom {
    int levels;
    int h[ECORR_MAX_LEVELS], w[ECORR_MAX_LEVELS];   // true level sizes
    int ntx[ECORR_MAX_LEVELS];                       // tiles per tile row; 0 = compact row-major
    int nty[ECORR_MAX_LEVELS];                       // tile rows (compact: image rows)
    int64_t sz[ECORR_MAX_LEVELS];                    // floats per query image
    int64_t off[ECORR_MAX_LEVELS + 1];               // float offset of each level; off[levels] = total
};

int pyramid_geometry(int64_t rows, int H, int W, int levels, PyrGeom* g);

// The per-level table the kernels read: a pyramid's (or a gradient pyramid's) levels in the storage
// of ecorr_device.h.  The parameter structs below start with it; level_table() fills it.  F: float
// where the kernels write the levels (the build, the backward), const float where they only read.
// One size for all three: the build indexes levels < 4 only and the lookups never read lnty.
template <typename F>
struct LevelTable {
    F* lvl[ECORR_MAX_LEVELS];                          // first float of each level (null past the last)
    int lh[ECORR_MAX_LEVELS], lw[ECORR_MAX_LEVELS];   // true level sizes
    int lntx[ECORR_MAX_LEVELS];                        // > 0 tiles per tile row, < 0 -blocks per block row
                                                       // (interleaved), 0 compact row-major
    int lnty[ECORR_MAX_LEVELS];                        // tile / block rows (compact: image rows)
    int64_t lsz[ECORR_MAX_LEVELS];                     // floats per query image
};
// T = the levels of g in the buffer at base; the entries past g.levels are cleared
template <typename F>
inline void level_table(const PyrGeom& g, F* base, LevelTable<F>* T) {
    *T = LevelTable<F>{};
    for (int i = 0; i < g.levels; ++i) {
        T->lvl[i] = base + g.off[i];
        T->lh[i] = g.h[i];
        T->lw[i] = g.w[i];
        T->lntx[i] = g.ntx[i];
        T->lnty[i] = g.nty[i];
        T->lsz[i] = g.sz[i];
    }
}

struct BuildParams : LevelTable<float> {   // the table: the levels written (those the GEMM epilogue fuses: < fused_levels)
    const float* f1;    // (elements of the launch's fmap_format when that is 16-bit: launch_build)
    const float* f2;
    int D, H, W;
    int q_count;        // query pixels in the fmap1 slab
    float scale;        // sqrt(D) (divide) or 1/sqrt(D) when sqrt(D) is a power of two (multiply)
    int scale_is_mul;
    int scale_shift;    // scale_is_mul: 1/sqrt(D) = 2^-scale_shift
    // split mode (ecorr_build_split): per-pixel power-of-two exponents of fmap1 ([B][q_count]) and
    // fmap2 ([B][H*W]) written by the exponent pass; null = the fp32-MFMA fmaf-chain build
    char* ws;           // split workspace (build_split_workspace_bytes), null = fp32 build
    int* ex1;
    int* ex2;
    const char* pk1;    // f16 hi/lo operand panels of fmap1 / fmap2 (pack_both_kernel)
    const char* pk2;
    // filled by launch_build
    int n_mt;           // 128-query tiles (fp32 blocks; fmap1 panels)
    int n_qt;           // 256-query tiles (split blocks)
    int n_nt, n_ntx;    // n-tiles (target blocks); regular n-tiles per tile row
    int n_reg, band_y0;  // regular (8 x 16) n-tiles per m-tile; first row of the 4-row band tiles
    int fused_levels;   // levels written by the GEMM epilogue (<= 4)
};

// stages (split build only; the fp32 build is one launch): 1 = operand pass, 2 = GEMM + fused
// pyramid (+ levels > 4), 3 = both.  fmap_format (split build, stage 1): ECORR_ELEM_* of P.f1 / P.f2
// hi (split build; the ecorr_build_split_*_hi entries): P.ws is a hi workspace's byte kHiFlagBytes, stage
// 1 zeroes the flag word at P.ws - kHiFlagBytes and, after the operand pass, sets it where a lo half of
// the panels is non-zero (launch_lo_flag); the D = 241 .. 256 GEMM sums hi*hi alone while it is 0
int launch_build(const BuildParams& P, int B, const PyrGeom& g, float* pyramid, hipStream_t stream, int stages = 3,
                 int fmap_format = ECORR_ELEM_F32, bool hi = false);
int64_t build_split_workspace_bytes(int B, int D, int H, int W, int q_count);
// build_hi.hip: *flag = 1 if any lo half of the panels [panels, panels + bytes) has a magnitude bit; and
// the hi-only GEMM of launch_build (hi, D = 241 .. 256) over P's ntiles block tiles
void launch_lo_flag(const char* panels, int64_t bytes, int* flag, hipStream_t stream);
void launch_split16_hi(const BuildParams& P, int64_t ntiles, hipStream_t stream);
constexpr int kHiFlagBytes = 256;   // the flag block in front of a hi workspace: int32 word 0, rest reserved

struct LookupParams : LevelTable<const float> {   // the table: the pyramid (read only)
    const float* coords;  // [B][2][q_count]
    float* out;           // [B][C][q_count]; 2-byte elements in the same order when the launch's
                          // out_format is ECORR_OUT_F16 / ECORR_OUT_BF16 (launch_lookup)
    int H, W;
    int q_count;
    int levels, radius;
    int C;                // levels * (2r+1)^2
    float* qmax;          // null, or [B][3 * levels][q_count]: per-query partial maxima of |out|
                          // (ecorr_lookup_qmax: the split convc1's column exponents)
    const int* scale;     // non-null: ecorr_lookup_presplit, out is the presplit layout and
                          // scale[b][q] the query's column exponent (launch_split_column_scale)
};

// out_format: ECORR_OUT_* (include/ecorr.h); the 16-bit formats have no qmax / presplit form
int launch_lookup(const LookupParams& P, int B, hipStream_t stream, int out_format = ECORR_OUT_F32);
// lookup_half.hip: launch_lookup's paths with ECORR_OUT_F16 / ECORR_OUT_BF16 elements
int launch_lookup_half(const LookupParams& P, int B, hipStream_t stream, int out_format);

// grad.hip: the backward (ecorr_lookup_backward, ecorr_build_backward).  The gradient pyramid has the
// pyramid's storage: the table is the gradient pyramid's.
struct LookupGradParams : LevelTable<float> {
    const float* grad_out;   // [B][C][q_count]
    const float* coords;     // [B][2][q_count]
    int q_count;
    int levels, radius;
    int C;
};
struct BuildGradParams {
    const float* T;          // the folded level 0 of the gradient pyramid: [B * q_count][sz], tiled
    const float* f1;         // [B][D][q_count]
    const float* f2;         // [B][D][H][W]
    float* g1;               // [B][D][q_count] or null
    float* g2;               // [B][D][H][W] or null
    int D, H, W, q_count;
    int ntx, sz;             // level 0: tiles per tile row, stored cells per query image
};
int launch_lookup_backward(const LookupGradParams& P, int B, hipStream_t stream);
// the fold over L's levels, then the GEMMs whose output is non-null
int launch_build_backward(const LookupGradParams& L, const BuildGradParams& P, int B, hipStream_t stream);

// out_format: ECORR_OUT_* of out (the 16-bit formats: the packed form only)
int launch_lookup_conv(const LookupParams& P, int B, const float* wt, const float* bias, int O, float* out,
                       hipStream_t stream, bool packed, int out_format = ECORR_OUT_F32);
int64_t conv1x1_packed_floats(int O, int C);
int launch_conv1x1_pack(const float* wt, int O, int C, float* packed, hipStream_t stream);
// conv.hip: split-f16 1x1 conv + ReLU on an NCHW tensor (ecorr_conv1x1_relu_split)
int64_t conv1x1_split_bytes(int O, int C);
// perm_levels > 0: the weight columns in the presplit channel order of that many radius-4 levels
int launch_conv1x1_split_pack(const float* wt, int O, int C, void* packed, hipStream_t stream, int perm_levels = 0);
// the presplit pack's byte count (its K = presplit_positions(levels))
int64_t conv1x1_presplit_bytes(int O, int levels);
// out_format: ECORR_OUT_* of out ([B][O][Q] elements of it)
int launch_conv1x1_relu_split(const float* in, int B, int C, int Q, const float* qmax, int G, const void* packed,
                              const float* bias, int O, float* out, hipStream_t stream,
                              int out_format = ECORR_OUT_F32);
// the same product without bias and ReLU, qmax required (grad_in of the backward: in = the masked
// gradient, packed = the transposed weight's pack); and whether a geometry is within both kernels'
// limits (G partial maxima, 0 = none)
int launch_conv1x1_split_linear(const float* in, int B, int C, int Q, const float* qmax, int G, const void* packed,
                                int O, float* out, hipStream_t stream);
bool conv1x1_split_geometry_ok(int B, int C, int Q, int O, int G);
// conv_grad.hip: the backward of relu(conv1x1) (ecorr_conv1x1_relu_backward); a null grad_in /
// grad_weight / grad_bias is not computed.  The size query returns the geometry's status.
int conv1x1_relu_backward_workspace_bytes(int B, int C, int Q, int O, int64_t* bytes);
int launch_conv1x1_relu_backward(const float* grad_out, const float* out, const float* in, const void* packed_t, int B,
                                 int C, int Q, int O, float* grad_in, float* grad_weight, float* grad_bias,
                                 void* workspace, hipStream_t stream);

// Presplit corr (ecorr_lookup_presplit -> ecorr_conv1x1_relu_presplit), radius 4, L <= 4 levels,
// C = 81 L channels at K = 88 L positions.  Channel ch = 81 lv + 27 part + k (lookup_cols_reg: wave
// `part` owns the 27 channels 9 ai + bb, k < 27) sits at K position
//   72 lv + 24 part + k               for k < 24 (three whole 8-channel groups of one wave)
//   72 L + 16 lv + 3 part + (k - 24)  for k >= 24 (the level's 9 last channels, 2 groups per level:
//                                      positions 9 .. 15 of them are zeros)
// so every group is written whole by one wave (the leftovers through LDS, by waves 0 and 1 of the
// level's workgroup): 2-byte stores shared between waves cost the lookup 7.5 us per call
// (profiles/r06_lab/ab_presplit_stores.json).  The conv's weight columns are permuted the same way
// (the channel sum is order-free up to rounding).  Layout per batch item: [group g][hi | lo][query]
// [8 halves], 16 B per (g, hi|lo, query), presplit_groups(K) groups (even: whole 16-channel K
// chunks); groups from 11 L on are never written (the conv reads them out of range: zeros).
__host__ __device__ inline int presplit_positions(int L) { return 88 * L; }
__host__ __device__ inline int presplit_groups(int K) { return 2 * ((K + 15) / 16); }
__host__ __device__ inline int presplit_pos(int ch, int L) {
    const int lv = ch / 81, r = ch - 81 * lv, part = r / 27, k = r - 27 * part;
    return k < 24 ? 72 * lv + 24 * part + k : 72 * L + 16 * lv + 3 * part + (k - 24);
}
__host__ __device__ inline int presplit_chan(int pos, int L) {   // inverse; -1 for a zero position
    if (pos < 72 * L) {
        const int lv = pos / 72, r = pos - 72 * lv, part = r / 24;
        return 81 * lv + 27 * part + (r - 24 * part);
    }
    const int j = pos - 72 * L, lv = j / 16, r = j - 16 * lv;
    if (lv >= L || r >= 9) return -1;
    const int part = r / 3;
    return 81 * lv + 27 * part + 24 + (r - 3 * part);
}
// bytes of one batch item's presplit corr at K positions
__host__ __device__ inline int64_t presplit_bytes_per_item(int K, int Q) { return (int64_t)presplit_groups(K) * 2 * Q * 16; }
int launch_conv1x1_relu_presplit(const void* in, int B, int levels, int Q, const int* scale, const void* packed,
                                 const float* bias, int O, float* out, hipStream_t stream);
// scale[b][q] (+ B trailing scratch entries): the presplit column exponents from the fmaps (lookup.hip)
int launch_split_column_scale(const float* f1, const float* f2, int B, int D, int H, int W, int* scale,
                              hipStream_t stream);

// alt.hip: the volume-free lookup (ecorr_alt_*, include/ecorr.h).  The feature buffer's geometry,
// computed once by alt_geometry() and shared by the pack and the lookup.
struct AltGeom {
    int levels, Dp;                                  // Dp: D rounded up to a multiple of 4
    int h[ECORR_MAX_LEVELS], w[ECORR_MAX_LEVELS];   // pooled fmap2 level sizes
    int64_t off[ECORR_MAX_LEVELS + 1];               // float offset of each fmap2 level (fmap1 at 0); off[levels] = total
};
int alt_geometry(int B, int D, int H, int W, int levels, AltGeom* g);
struct AltParams {
    const float* f1;                   // [B][Q][Dp]
    const float* lvl[ECORR_MAX_LEVELS];   // [B][h w][Dp]
    int lh[ECORR_MAX_LEVELS], lw[ECORR_MAX_LEVELS];
    const float* coords;               // [B][2][Q]
    void* out;                         // [B][C][Q] elements of the launch's out_format
    int B, Dp, Q, levels, radius, C;
    float scale;                       // the scale step (abi.hip scale_step_of)
    int scale_is_mul;
};
int launch_alt_pack(const void* f1, const void* f2, int fmap_format, int B, int D, int H, int W, const AltGeom& g,
                    float* feat, hipStream_t stream);
int launch_alt_lookup(const AltParams& P, int out_format, hipStream_t stream);

// alt_grad.hip: the backward of the volume-free lookup (ecorr_alt_lookup_backward,
// ecorr_alt_pack_backward).  The gradient feature buffer has the feature buffer's layout (AltGeom).
// Workspace of one lookup backward, per (batch item, level, query): the window origin (two ints, x =
// kAltNoWindow: the query has no window on that level) and, after all origins, its (2r+3)^2 window
// gradient.
constexpr int kAltNoWindow = INT32_MIN;
int64_t alt_backward_workspace_bytes(int B, int64_t Q, int levels, int radius);
struct AltGradParams {
    const float* f1;                      // the features: [B][Q][Dp]
    const float* lvl[ECORR_MAX_LEVELS];   // [B][h w][Dp]
    float* g1;                            // their gradients, same layout
    float* glvl[ECORR_MAX_LEVELS];
    int lh[ECORR_MAX_LEVELS], lw[ECORR_MAX_LEVELS];
    int lt0[ECORR_MAX_LEVELS + 1];        // first target pixel of each level in a batch item's list of all levels' pixels
    const float* coords;                  // [B][2][Q]
    const float* grad_out;                // [B][C][Q]
    int2* org;                            // workspace: [B][levels][Q] origins
    float* win;                           //            [B][levels][Q][(2r+3)^2] windows
    int B, Dp, Q, levels, radius, C;
    float scale;                          // the scale step (abi.hip scale_step_of)
    int scale_is_mul;
};
int launch_alt_lookup_backward(const AltGradParams& P, hipStream_t stream);
// folds the pooled levels of grad_feat onto level 0, then transposes into the non-null outputs
int launch_alt_pack_backward(float* grad_feat, int B, int D, int H, int W, const AltGeom& g, float* grad_fmap1,
                             float* grad_fmap2, hipStream_t stream);

// gru.hip: SepConvGRU (ecorr_sepconv_gru*, include/ecorr.h).  gru_sizes_ok: the (hidden, input) the kernels
// are built for; gru_geometry_ok: B, H, W within their 32-bit offsets and grid limits.
bool gru_sizes_ok(int hidden, int input);
bool gru_geometry_ok(int B, int H, int W);
int64_t gru_packed_bytes();
int64_t gru_workspace_bytes(int B, int H, int W);
int launch_gru_pack(const float* const weight[6], const float* const bias[6], void* packed, hipStream_t stream);
int launch_gru(const float* h, const float* x, int B, int H, int W, const void* packed, float* h_out, void* workspace,
               hipStream_t stream);
// the forward with every gate kept, for the backward: g = [h1 z1 r1 q1 z2 r2 q2 h'] and rh, each [B][128][H W]
int launch_gru_gates(const float* h, const float* x, int B, int H, int W, const void* packed, float* g, float* rh,
                     hipStream_t stream);
// gru_grad.hip: its backward (ecorr_sepconv_gru_backward*).  grad_h / grad_x may be null; grad_weight and
// grad_bias (six pointers each, z1 r1 q1 z2 r2 q2) are both null or both complete.
int64_t gru_packed_t_bytes();
int64_t gru_backward_workspace_bytes(int B, int H, int W);
int launch_gru_pack_t(const float* const weight[6], void* packed_t, hipStream_t stream);
int launch_gru_backward(const float* h, const float* x, const float* grad_out, int B, int H, int W, const void* packed,
                        const void* packed_t, float* grad_h, float* grad_x, float* const* grad_weight,
                        float* const* grad_bias, void* workspace, hipStream_t stream);

// motion_enc.hip: the motion encoder behind convc1 (ecorr_motion_encoder*, include/ecorr.h).  weight / bias in the
// order convc2 convf1 convf2 conv; out [b] at out + b out_batch_stride floats, [128][H W].
bool menc_geometry_ok(int B, int H, int W);
int64_t menc_packed_bytes();
int64_t menc_workspace_bytes(int B, int H, int W);
int launch_menc_pack(const float* const weight[4], const float* const bias[4], void* packed, hipStream_t stream);
int launch_menc(const float* c1, const float* flow, int B, int H, int W, const void* packed, float* out,
                int64_t out_batch_stride, void* workspace, hipStream_t stream);
// the forward's first three launches into cor [B][192][H W], f1 [B][128][H W] and flo [B][64][H W], then conv's GEMM
// writing go = relu'(conv's result) grad_out[:126] (two zero rows behind) [B][128][H W] instead of the result;
// grad_out item b at grad_out + b grad_out_bs
int launch_menc_recompute(const float* c1, const float* flow, const float* grad_out, int64_t grad_out_bs, int B, int H,
                          int W, const void* packed, float* cor, float* f1, float* flo, float* go, hipStream_t stream);
// motion_enc_grad.hip: its backward (ecorr_motion_encoder_backward*).  grad_c1 / grad_flow may be null; grad_weight
// and grad_bias (four pointers each, convc2 convf1 convf2 conv) are both null or both complete.
int64_t menc_packed_t_bytes();
int64_t menc_backward_workspace_bytes(int B, int H, int W);
int launch_menc_pack_t(const float* const weight[4], void* packed_t, hipStream_t stream);
int launch_menc_backward(const float* c1, const float* flow, const float* grad_out, int64_t grad_out_bs, int B, int H,
                         int W, const void* packed, const void* packed_t, float* grad_c1, float* grad_flow,
                         float* const* grad_weight, float* const* grad_bias, void* workspace, hipStream_t stream);

int launch_bilinear_sampler(const float* img, int N, int C, int h, int w, const float* coords,
                            int Hg, int Wg, float* out, float* mask, hipStream_t stream);

int launch_coords_grid(int B, int H, int W, float* out, hipStream_t stream);

// rows.hip: [world][chunk] all-gathered row chunks -> [B][C][H][W] (include/ecorr.h)
int launch_rows_assemble(const float* chunks, int64_t chunk, int world, int B, int C, int H, int W, float* out,
                         hipStream_t stream);

int launch_upsample_flow(const float* flow, const float* mask, int N, int H, int W, float* out, hipStream_t stream);
// the backward: t = float[N][18][H*W] in the workspace, then the 9-tap gather into grad_flow; a null
// grad_flow / grad_mask is not computed
int64_t upsample_backward_workspace_bytes(int N, int H, int W);
int launch_upsample_flow_backward(const float* grad_out, const float* flow, const float* mask, int N, int H, int W,
                                  float* grad_flow, float* grad_mask, void* workspace, hipStream_t stream);
int launch_png16_encode(const float* flow, int B, int h, int w, uint16_t* out, hipStream_t stream);
int launch_png16_decode(const uint16_t* in, int B, int h, int w, float* flow, uint8_t* valid, int* bad,
                        hipStream_t stream);

uint32_t voxel_key_range(bool dsec, int C, int H, int W);
int voxel_workspace_bytes(bool dsec, int64_t n, int C, int H, int W, int64_t* bytes);
int launch_voxel(bool dsec, const float* p, const float* t, const float* x, const float* y, const double* ev,
                 int64_t n, int C, int H, int W, int normalize, float* voxel, int* bad, void* workspace,
                 hipStream_t stream);

int64_t splat_workspace_bytes(int B, int64_t n, int h, int w);
int launch_splat(bool flow_mode, const float* pts, int B, int64_t n, int h, int w, float* values, uint8_t* valid,
                 void* workspace, hipStream_t stream);

}  // namespace ecorr
