/*
 * ecorr.h -- C ABI of the MI355X-native E-RAFT correlation hot path (libecorr.so, gfx950).
 *
 * Drop-in boundary for wzygzlm/E-RAFT's model/corr.py CorrBlock and the model/utils.py helpers.
 * Every entry point is stream-ordered and asynchronous on `stream` (a hipStream_t passed as
 * void*, e.g. torch.cuda.current_stream().cuda_stream); all buffers are device pointers owned by
 * the caller (PyTorch's caching allocator); the library allocates nothing and keeps no global
 * mutable state.  Return value: ECORR_OK (0) or a negative code; ecorr_strerror() names it.  No
 * C++ exception crosses this boundary.
 *
 * Pyramid storage (what ecorr_build writes, ecorr_lookup reads) -- a layout chosen for the gather:
 * `levels` blocks concatenated at float offsets off_i (each a multiple of 32 floats, i.e. 128-byte
 * aligned); level i holds rows = B * q_count query images of h_i x w_i (h_0 = H, w_0 = W,
 * h_{i+1} = h_i / 2, w_{i+1} = w_i / 2, floor -- the shapes of the reference's corr_pyramid[i],
 * corr.py:16-27).  Each level is stored in one of three formats (ecorr_pyramid_formats):
 *   tiled (ntx_i > 0; levels 0 and >= 4): row-major ECORR_TILE_H x ECORR_TILE_W tiles of 32
 *     floats (128 bytes, one L2 line); image r starts at off_i + r * hp_i * wp_i,
 *     hp_i = roundup(h_i, 4), wp_i = roundup(w_i, 8) = 8 * ntx_i, and pixel (y, x) sits at
 *     ((y / 4) * ntx_i + x / 8) * 32 + (y % 4) * 8 + x % 8.  A radius-4 window then touches ~7
 *     lines per level instead of ~13 with row-major images; padding cells are never read.
 *   interleaved (ntx_i = -nbx < 0; levels 1, 2 and 3): blocks of bh x bw = 2 x 4 (levels 1 and 2)
 *     or 1 x 2 (level 3) pixels (at levels 2 and 3 what one 8 x 16 block of level 0 pools to),
 *     nby = ceil(h_i / bh) by nbx =
 *     ceil(w_i / bw) of them per image, sz = nby * nbx * bh * bw floats per image; the rows are
 *     taken in groups of ECORR_ROW_GROUP = 64 (the level holds roundup(rows, 64) * sz floats) and
 *     pixel (y, x) of row r sits at (r / 64) * 64 * sz + (((y / bh) * nbx + x / bw) * 64 + r % 64)
 *     * bh * bw + (y % bh) * bw + x % bw: a block's pixels of 64 consecutive rows are contiguous,
 *     so the build stores them as whole lines and adjacent queries' window reads share lines.
 *   compact (ntx_i = 0): plain row-major h_i x w_i, image r at off_i + r * h_i * w_i.  Used for
 *     levels i >= 4 whose tile padding would exceed half the image (2 hp wp > 3 h w).
 * The Python shim materializes reference-layout corr_pyramid views on demand.
 *
 * Query slabs (multi-GPU query-row sharding): fmap1, coords and the lookup output hold
 * the q_count query pixels being served -- all H*W of them for the plain CorrBlock, a contiguous
 * block of image rows on a query-row shard.  fmap2 is always the whole [B][D][H][W] target map.
 */
#ifndef ECORR_H
#define ECORR_H

#include <stdint.h>

#ifdef __cplusplus
extern "C" {
#endif

#define ECORR_ABI_VERSION 17
#define ECORR_MAX_LEVELS 16
#define ECORR_TILE_H 4
#define ECORR_TILE_W 8
#define ECORR_ROW_GROUP 64

enum ecorr_status {
    ECORR_OK = 0,
    ECORR_EINVAL = -1,   /* null pointer, non-positive size, q_count outside [1, H*W] */
    ECORR_ESHAPE = -2,   /* a pyramid level would be 0 pixels tall or wide (reference: avg_pool2d
                            raises "Output size is too small", corr.py:26) */
    ECORR_ERADIUS = -3,  /* radius < 0 or > 32 */
    ECORR_ELEVELS = -4,  /* levels < 1 or > ECORR_MAX_LEVELS */
    ECORR_EHIP = -1000   /* HIP error e is reported as ECORR_EHIP - e */
};

/* Layout of the pyramid for `rows` query rows (rows = B * q_count).  Writes h[levels],
 * w[levels] (true level sizes), off[levels + 1] (float offsets including tile padding and the
 * 128-byte alignment of each level; off[levels] = total floats).
 * Replaces: the shapes produced by CorrBlock.__init__'s reshape + avg_pool2d loop, corr.py:21-27. */
int ecorr_pyramid_layout(int64_t rows, int H, int W, int levels, int* h, int* w, int64_t* off);

/* Build the correlation pyramid: level 0 = fmap1^T fmap2 / sqrt(D), levels 1.. = 2x2 floor-mode
 * average pools.  fmap1: float[B][D][q_count] (the query slab; = [B][D][H][W] when q_count = H*W),
 * fmap2: float[B][D][H][W], both contiguous.  pyramid: ecorr_pyramid_layout(B*q_count, ...) floats.
 * Replaces: CorrBlock.__init__ (corr.py:13-27) and CorrBlock.corr (corr.py:52-60). */
int ecorr_build(const float* fmap1, const float* fmap2, int B, int D, int H, int W, int q_count,
                int levels, float* pyramid, void* stream);

/* Same result contract as ecorr_build (level 0 within the 1e-5 normwise bar of the reference's
 * fp32 GEMM, levels 1.. pooled bit-exactly from it), computed on the f16 matrix cores: each fp32
 * operand is scaled by a per-pixel power of two and split into f16 hi + lo, and every product is
 * summed as lo*hi + hi*lo + hi*hi in fp32 -- error vs fp64 below the fp32-MFMA path's.  Per-pixel
 * scales depend only on that pixel's D values, so row-sharded and whole builds agree bit for bit.
 * workspace: ecorr_build_split_workspace_size() bytes of device memory, 256-byte aligned (the
 * exponents and the pre-split operands in MFMA-fragment order, about the two fmaps' size; free
 * once the call has completed on `stream`).  B <= 65535.
 * Replaces: CorrBlock.__init__ (corr.py:13-27) and CorrBlock.corr (corr.py:52-60). */
int ecorr_build_split_workspace_size(int B, int D, int H, int W, int q_count, int64_t* bytes);
int ecorr_build_split(const float* fmap1, const float* fmap2, int B, int D, int H, int W, int q_count,
                      int levels, float* pyramid, void* workspace, void* stream);

/* ecorr_build_split as its two stream-ordered stages, for callers that overlap or time them:
 * _pack = the operand pass (per-pixel exponents + f16 hi/lo panels into the workspace; reads
 * fmap1/fmap2), _gemm = the correlation GEMM with the fused pyramid (reads only the workspace).
 * pack then gemm on one stream == ecorr_build_split, bit for bit.  Contract: both stages take the
 * SAME workspace and IDENTICAL geometry (B, D, H, W, q_count), gemm stream-ordered after pack.  The
 * workspace carries no header (a check would need a host read of device memory, i.e. a sync), so a
 * gemm on a workspace packed for other geometry, or never packed, yields garbage exponents and
 * panels rather than an error. */
int ecorr_build_split_pack(const float* fmap1, const float* fmap2, int B, int D, int H, int W, int q_count,
                           void* workspace, void* stream);
int ecorr_build_split_gemm(int B, int D, int H, int W, int q_count, int levels, float* pyramid,
                           void* workspace, void* stream);

/* Radius-r lookup: out float[B][levels*(2r+1)^2][q_count] (= [B][C][H][W] when q_count = H*W),
 * channel 81*i + 9*a + b (r = 4) = bilinear sample of level i at (x/2^i + a - r, y/2^i + b - r),
 * zeros padding.  coords: float[B][2][q_count] contiguous (channel 0 = x, 1 = y, pixel units of
 * the H x W map).  Bit-exact with the reference on CPU.
 * Replaces: CorrBlock.__call__ (corr.py:29-50) incl. bilinear_sampler (utils.py:7-21). */
int ecorr_lookup(const float* pyramid, const float* coords, int B, int H, int W, int q_count,
                 int levels, int radius, float* out, void* stream);

/* ecorr_lookup with a chosen output element (added within ABI 17: purely additive, the version
 * stays 17): out holds B*levels*(2r+1)^2*q_count elements of out_format in ecorr_lookup's order
 * [B][C][q_count] -- float (ECORR_OUT_F32: ecorr_lookup's launch, bit for bit), IEEE binary16
 * (ECORR_OUT_F16) or bfloat16 (ECORR_OUT_BF16), 2-byte aligned.  Rounding contract: the element is
 * the fp32 sample ecorr_lookup computes, rounded ONCE to nearest-even -- binary16 as the hardware
 * convert does (|x| past 65504 + half an ulp gives +-inf, subnormals are kept, NaN stays NaN);
 * bfloat16 to nearest-even on the upper 16 bits (NaN stays NaN, +-inf stays +-inf) -- so it equals a
 * cast of ecorr_lookup's output, which a mixed-precision consumer (autocast's convc1) would otherwise
 * make in a kernel of its own.  Same argument validation and error codes as ecorr_lookup; an unknown
 * out_format gives ECORR_EINVAL.  Replaces: corr.py:29-50 followed by autocast's cast (eraft.py:131-132). */
#define ECORR_OUT_F32 0
#define ECORR_OUT_F16 1
#define ECORR_OUT_BF16 2
int ecorr_lookup_as(const float* pyramid, const float* coords, int B, int H, int W, int q_count,
                    int levels, int radius, int out_format, void* out, void* stream);

/* The same three element codes under a name that also reads sensibly for an INPUT format (the
 * values are the ECORR_OUT_* ones: either spelling may be passed to any *_as entry). */
#define ECORR_ELEM_F32 ECORR_OUT_F32
#define ECORR_ELEM_F16 ECORR_OUT_F16
#define ECORR_ELEM_BF16 ECORR_OUT_BF16

/* 16-bit feature maps in (added within ABI 17: purely additive, the version stays 17):
 * ecorr_build_split_pack / ecorr_build_split reading fmap1 and fmap2 as elements of fmap_format --
 * float (ECORR_ELEM_F32: the existing launch), IEEE binary16 (ECORR_ELEM_F16) or bfloat16
 * (ECORR_ELEM_BF16); both fmaps have the same format, the same shapes and order as the fp32 entries
 * take, and need only the element's alignment (a 16-bit query slab view may be 2-byte aligned only).
 * Same workspace size (ecorr_build_split_workspace_size), same geometry contract;
 * ecorr_build_split_gemm follows ecorr_build_split_pack_as unchanged.
 * Bitwise contract: the kernel converts each element to fp32 on load, which is exact, and runs the
 * fp32 operand pass on it, so the workspace contents -- exponents and hi/lo panels -- are bitwise
 * those of ecorr_build_split_pack on the fmaps converted to fp32; the pyramid of the gemm that follows
 * is therefore bitwise equal too, and a +-inf or NaN element behaves as the same fp32 value does
 * (+-inf -> NaN in its level-0 row / column, NaN -> NaN).
 * Same argument validation and error codes as the fp32 entries; an unknown fmap_format gives
 * ECORR_EINVAL after those checks and before any launch.  ecorr_build_split_as is pack_as then gemm,
 * as ecorr_build_split is pack then gemm.  (The fp32-MFMA build, ecorr_build, takes fp32 only.)
 * Replaces: the .float() of both fmaps (eraft.py:104-105) + CorrBlock.__init__ (corr.py:13-27). */
int ecorr_build_split_pack_as(const void* fmap1, const void* fmap2, int fmap_format, int B, int D, int H, int W,
                              int q_count, void* workspace, void* stream);
int ecorr_build_split_as(const void* fmap1, const void* fmap2, int fmap_format, int B, int D, int H, int W,
                         int q_count, int levels, float* pyramid, void* workspace, void* stream);

/* The hi-only split build (added within ABI 17: purely additive, the version stays 17): the split
 * build for fmaps whose elements fit the split's hi half -- every finite binary16 or bfloat16 value,
 * and every fp32 value with at most 11 significant bits in binary16's range once scaled.  For such
 * fmaps every lo half of the operand panels is +-0, two of the three MFMAs per product add zeros, and
 * the GEMM sums hi*hi alone: one MFMA per product and half the panel bytes read.
 *   _pack_hi_as  ecorr_build_split_pack_as's pass, then a scan of the panels' lo halves that records on
 *                the device whether any has a magnitude bit (any non-finite element's does: a NaN);
 *   _gemm_hi     ecorr_build_split_gemm; at D = 241 .. 256 it runs the one-term loop when that record
 *                is clear and the three-term loop otherwise.  At any other D it is
 *                ecorr_build_split_gemm's kernel and the record is unused;
 *   _hi_as       pack_hi_as then gemm_hi.
 * Bitwise contract: the pyramid is bitwise that of ecorr_build_split_as on the same inputs, whichever
 * loop ran -- with every lo = +-0 and every hi finite the dropped MFMAs add sums of +-0 to an
 * accumulator that starts at +0, is never -0 and never subnormal, which leaves its bits alone.  The
 * caller never learns which loop ran and need not.
 * workspace: ecorr_build_split_hi_workspace_size() bytes = ecorr_build_split_workspace_size() + 256,
 * 256-byte aligned.  Its first 256 bytes are the record (int32 word 0: 0 = every lo half is +-0, 1 =
 * not; the rest reserved); from byte 256 on it is, byte for byte, the workspace ecorr_build_split_pack_as
 * writes.  _pack_hi_as zeroes word 0 on `stream` (a memset node under graph capture) before its pass.
 * The two stages take the same workspace and geometry, gemm stream-ordered after pack, as the plain
 * stages do.  All three ECORR_ELEM_* formats are accepted.  Same argument validation, order and
 * error codes as the *_as entries; an unknown fmap_format gives ECORR_EINVAL before any launch. */
int ecorr_build_split_hi_workspace_size(int B, int D, int H, int W, int q_count, int64_t* bytes);
int ecorr_build_split_pack_hi_as(const void* fmap1, const void* fmap2, int fmap_format, int B, int D, int H, int W,
                                 int q_count, void* workspace, void* stream);
int ecorr_build_split_gemm_hi(int B, int D, int H, int W, int q_count, int levels, float* pyramid,
                              void* workspace, void* stream);
int ecorr_build_split_hi_as(const void* fmap1, const void* fmap2, int fmap_format, int B, int D, int H, int W,
                            int q_count, int levels, float* pyramid, void* workspace, void* stream);

/* ---- The backward (ABI 17): gradients of a loss through ecorr_lookup and ecorr_build, coordinates detached ----
 * Deterministic: a query row's gradient images are owned by one workgroup per launch and summed in
 * a fixed order; there are no float atomics, so equal inputs give bitwise equal gradients. */

/* dL/d(pyramid) += one lookup's contribution.  grad_pyramid: ecorr_pyramid_layout(B*q_count, ...) floats in the
 * pyramid's own storage, zeroed by the caller before the block's first call.  grad_out float[B][levels*(2r+1)^2][q_count].
 * The pixels that receive gradient are exactly the in-range corners the forward read (same coordinate
 * arithmetic, same float in-range test: NaN, +-inf and huge coordinates add nothing).  Calls on one
 * grad_pyramid must be stream-ordered.  B <= 65535.
 * Same argument validation and error codes as ecorr_lookup.  Replaces: autograd of corr.py:29-50 / utils.py:7-21. */
int ecorr_lookup_backward(const float* grad_out, const float* coords, int B, int H, int W, int q_count,
                          int levels, int radius, float* grad_pyramid, void* stream);
/* Consumes grad_pyramid (level 0 is overwritten by the fold of levels 1.. onto it: the backward of the
 * 2x2 floor-mode average pools).  grad_fmap1 float[B][D][q_count] (the query slab),
 * grad_fmap2 float[B][D][H][W] = this slab's contribution (the whole gradient when q_count = H*W); either may be NULL.
 * fp32 matrix cores, fp32 accumulation, no workspace.
 * Replaces: autograd of corr.py:13-27,52-60. */
int ecorr_build_backward(float* grad_pyramid, const float* fmap1, const float* fmap2, int B, int D, int H, int W,
                         int q_count, int levels, float* grad_fmap1, float* grad_fmap2, void* stream);

/* ecorr_lookup + per-query partial maxima for ecorr_conv1x1_relu_split (ABI 15): qmax
 * float[B][3*levels][q_count], max over its 3*levels entries of query p = max_c |out[b][c][p]|
 * (fmaxf: NaN ignored); out bitwise what ecorr_lookup writes.  Replaces: corr.py:29-50 as above. */
int ecorr_lookup_qmax(const float* pyramid, const float* coords, int B, int H, int W, int q_count,
                      int levels, int radius, float* out, float* qmax, void* stream);

/* Lookup fused with its consumer, BasicMotionEncoder's convc1 + ReLU:
 * out float[B][O][q_count] = relu(bias[o] + sum_c weight[o][c] * corr[b][c][p]), where corr is
 * exactly what ecorr_lookup would return (C = levels*(2r+1)^2 channels) and never leaves the chip.
 * weight: float[O][C] (the conv weight [O][C][1][1] as stored), bias: float[O] or NULL.
 * radius must be 4 (else ECORR_ERADIUS), levels <= 4 (else ECORR_ELEVELS), O a positive multiple
 * of 64 (else ECORR_EINVAL).
 * Replaces: CorrBlock.__call__ (corr.py:29-50) + F.relu(self.convc1(corr)) (update.py:67,74). */
int ecorr_lookup_conv1x1_relu(const float* pyramid, const float* coords, int B, int H, int W, int q_count,
                              int levels, int radius, const float* weight, const float* bias, int O,
                              float* out, void* stream);

/* The same with the weight re-laid once in the fused kernel's MFMA fragment order (ABI 14): each
 * wave load of the weight stream is then one contiguous 1-KB piece.  ecorr_conv1x1_packed_size
 * gives the packed float count for O output and C = levels*(2r+1)^2 input channels (O a positive
 * multiple of 64); ecorr_conv1x1_pack writes it from weight float[O][C] (stream-ordered);
 * ecorr_lookup_conv1x1_relu_packed takes it in place of the weight -- bitwise the same result as
 * ecorr_lookup_conv1x1_relu with that weight.  The packed weight stays valid until the weight
 * changes (the Python binding re-packs on every in-place update of the weight tensor). */
int ecorr_conv1x1_packed_size(int O, int C, int64_t* floats);
int ecorr_conv1x1_pack(const float* weight, int O, int C, float* packed, void* stream);
int ecorr_lookup_conv1x1_relu_packed(const float* pyramid, const float* coords, int B, int H, int W, int q_count,
                                     int levels, int radius, const float* packed, const float* bias, int O,
                                     float* out, void* stream);

/* convc1 + ReLU on a materialized lookup (ABI 15; SURVEY §8f row 1 as two launches: ecorr_lookup,
 * then this): out float[B][O][Q] = relu(bias[o] + sum_c weight[o][c] * in[b][c][p]) for any
 * in float[B][C][Q] (the lookup's [B][C][H][W] with Q = H*W or a q_count slab), on the f16 matrix
 * cores with split operands (each fp32 value as hi + lo f16 under a per-query / per-output-row
 * power-of-two scale; three MFMAs per product): normwise within 1e-5 of the fp32 conv, not bitwise.
 * ecorr_conv1x1_split_size gives the packed weight's byte count, ecorr_conv1x1_split_pack writes it
 * from weight float[O][C] (stream-ordered); valid until the weight changes.  bias float[O] or NULL;
 * in and out must not overlap (ECORR_EINVAL when they are the same pointer, or when the 32-bit
 * buffer offsets, about (2C + 64) * Q * 4 bytes, would overflow).  qmax: NULL (the kernel finds each
 * query's largest |in| itself, one extra pass over in) or float[B][G][Q] partial maxima whose max
 * over g is max_c |in[b][c][p]| (fmaxf semantics, NaN ignored) -- what ecorr_lookup_qmax writes
 * with G = 3 * levels; the result is bitwise the same either way.
 * Non-finite input (the contract, tests/test_conv_split_gpu.py): a single +-inf or NaN value in a
 * query column in[b][.][p] makes EVERY output out[b][.][p] of that query NaN (the split's lo half
 * of an inf is inf - inf), where the reference's fp32 conv + ReLU gives +-inf / 0 / NaN per output;
 * the other queries are unaffected.  The split CorrBlock build never produces +-inf samples; the
 * fused entry (ecorr_lookup_conv1x1_relu_packed, fp32 sums) keeps the reference's pattern.
 * Replaces: F.relu(self.convc1(corr)) (update.py:67,74). */
int ecorr_conv1x1_split_size(int O, int C, int64_t* bytes);
int ecorr_conv1x1_split_pack(const float* weight, int O, int C, void* packed, void* stream);
int ecorr_conv1x1_relu_split(const float* in, int B, int C, int Q, const float* qmax, int G, const void* packed,
                             const float* bias, int O, float* out, void* stream);

/* 16-bit convc1 output (added within ABI 17: purely additive, the version stays 17):
 * ecorr_conv1x1_relu_split / ecorr_lookup_conv1x1_relu_packed with a chosen output element.  out holds
 * B*O*Q (B*O*q_count) elements of out_format (ECORR_OUT_* / ECORR_ELEM_*) in the same [B][O][Q] order,
 * 2-byte aligned for the 16-bit formats.  Bitwise contract: each element is the fp32 value the fp32
 * entry writes -- after bias and ReLU -- rounded ONCE to nearest-even by the rules of ecorr_lookup_as
 * (binary16: the hardware convert, overflow to +-inf, subnormals kept; bfloat16: on the upper 16 bits),
 * so the result is bitwise a cast of the fp32 entry's output, which autocast would otherwise make in a
 * kernel of its own in front of convc2 (update.py:75).  The non-finite contract is unchanged (a NaN
 * stays NaN).  ECORR_OUT_F32 is the existing launch.  in != out still holds, and the 32-bit offset
 * limit of the stores scales with the element size.  Same argument validation and error codes as the
 * fp32 entries; an unknown out_format gives ECORR_EINVAL after those checks and before any launch.
 * (The presplit conv and the unpacked fused entry have no _as form.)
 * Replaces: F.relu(self.convc1(corr)) (update.py:67,74) followed by autocast's cast. */
int ecorr_conv1x1_relu_split_as(const float* in, int B, int C, int Q, const float* qmax, int G, const void* packed,
                                const float* bias, int O, int out_format, void* out, void* stream);
int ecorr_lookup_conv1x1_relu_packed_as(const float* pyramid, const float* coords, int B, int H, int W,
                                        int q_count, int levels, int radius, const float* packed,
                                        const float* bias, int O, int out_format, void* out, void* stream);

/* The backward of ecorr_conv1x1_relu_split's function (added within ABI 17), for any in float[B][C][Q]:
 * with grad_out, out float[B][O][Q] (out: the forward's post-ReLU result) and the masked gradient
 *   gm[b][o][p] = out[b][o][p] <= 0 ? 0 : grad_out[b][o][p]     (ATen threshold_backward: a NaN in
 *                                                                 out passes the gradient through)
 *   grad_in     float[B][C][Q] = sum_o W[o][c] * gm[b][o][p]
 *   grad_weight float[O][C]    = sum_{b,p} gm[b][o][p] * in[b][c][p]
 *   grad_bias   float[O]       = sum_{b,p} gm[b][o][p]
 * Each output may be NULL and is then not computed (all three NULL: ECORR_EINVAL); every element of
 * a non-null output is overwritten, never accumulated into; nothing else is written but the
 * workspace (ecorr_conv1x1_relu_backward_workspace_size bytes, required; contents undefined before
 * and after).  packed_t: what ecorr_conv1x1_split_pack writes for the TRANSPOSED weight float[C][O],
 * called as (wT, C, O) (size: ecorr_conv1x1_split_size(C, O)); needed only for grad_in.  in: needed
 * only for grad_weight.  grad_in must not be grad_out, out or in.
 * grad_in runs on the f16 matrix cores with split operands like the forward: normwise within 1e-5
 * of fp64, and a non-finite gm value makes that query's whole grad_in column NaN.  grad_weight sums
 * fp32 products on v_mfma_f32_32x32x2_f32 in slabs of at most 1024 queries of one batch item, the
 * slab partials added in ascending order; grad_bias likewise from per-block partial sums.
 * Deterministic: no atomics, one writer per cell, summation orders fixed by the shape; equal inputs
 * give bitwise equal gradients.
 * ECORR_EINVAL before any launch: a NULL required pointer, B outside [1, 65535], C, Q or O < 1, or
 * the 32-bit offset limits of ecorr_conv1x1_relu_split with the roles of C and O swapped; the size
 * query returns the same status for the same geometry.
 * Replaces: autograd of update.py:67,74. */
int ecorr_conv1x1_relu_backward_workspace_size(int B, int C, int Q, int O, int64_t* bytes);
int ecorr_conv1x1_relu_backward(const float* grad_out, const float* out, const float* in, const void* packed_t,
                                int B, int C, int Q, int O,
                                float* grad_in, float* grad_weight, float* grad_bias,
                                void* workspace, void* stream);

/* Presplit convc1 (ABI 16): the lookup writes corr already split for the split conv, so the conv
 * loads each 8-channel B fragment as two 16-byte pieces and runs no split arithmetic and no maxima.
 * The query's scale must be known before any level's samples are written, so it is a bound, not
 * the samples' maximum: every sample of query p (level-0 values, their 2x2 averages and bilinear
 * blends) is at most sqrt(D) * max_d |fmap1[b][d][p]| * max |fmap2[b]| in magnitude.
 * ecorr_split_column_scale: fmap1, fmap2 float[B][D][H][W] -> scale int[B*H*W + B] (the last B
 *   entries are scratch): scale[b*H*W + p] = s_p, with every sample of p times 2^s_p below 2^15.
 * ecorr_presplit_size: bytes of the presplit corr of B items of Q queries (88 * levels positions
 *   for the 81 * levels channels).
 * ecorr_lookup_presplit: radius 4 (else ECORR_ERADIUS), levels <= 4 (else ECORR_ELEVELS):
 *   ecorr_lookup's samples x 2^s_p, split into f16 hi + lo (exactly: x 2^s = hi + lo + O(2^-22)),
 *   in the presplit layout (groups of 8 positions, 16 B per group / hi|lo / query; the channel
 *   order of e-raft_amd/csrc/ecorr_internal.h presplit_pos, zeros at the 7 * levels padding
 *   positions).  scale as written above.
 * ecorr_conv1x1_presplit_size / ecorr_conv1x1_split_pack_presplit: ecorr_conv1x1_split_pack with the
 *   weight columns at those positions (C = 81 * levels).
 * ecorr_conv1x1_relu_presplit: ecorr_conv1x1_relu_split's result from the presplit corr and the
 *   same scale: normwise within 1e-5 of the fp32 conv, not bitwise the split conv (other column
 *   scales, other channel order); the non-finite contract of ecorr_conv1x1_relu_split.
 * Replaces: CorrBlock.__call__ (corr.py:29-50) + F.relu(self.convc1(corr)) (update.py:67,74). */
int ecorr_split_column_scale(const float* fmap1, const float* fmap2, int B, int D, int H, int W, int* scale,
                             void* stream);
int ecorr_presplit_size(int B, int levels, int q_count, int64_t* bytes);
int ecorr_lookup_presplit(const float* pyramid, const float* coords, int B, int H, int W, int q_count, int levels,
                          int radius, const int* scale, void* out, void* stream);
int ecorr_conv1x1_presplit_size(int O, int levels, int64_t* bytes);
int ecorr_conv1x1_split_pack_presplit(const float* weight, int O, int levels, void* packed, void* stream);
int ecorr_conv1x1_relu_presplit(const void* in, int B, int levels, int Q, const int* scale, const void* packed,
                                const float* bias, int O, float* out, void* stream);

/* Generic bilinear_sampler: img float[N][C][h][w], coords float[N][Hg][Wg][2] in pixels ->
 * out float[N][C][Hg][Wg]; mask (nullable) float[N][Hg][Wg] = 1 where the normalized sample
 * lies strictly inside (-1, 1)^2.  Replaces: model/utils.py:7-21. */
int ecorr_bilinear_sampler(const float* img, int N, int C, int h, int w, const float* coords,
                           int Hg, int Wg, float* out, float* mask, void* stream);

/* coords_grid: out float[B][2][H][W], channel 0 = x (column), 1 = y (row).
 * Replaces: model/utils.py:24-27. */
int ecorr_coords_grid(int B, int H, int W, float* out, void* stream);

/* ---- SURVEY §8e, configs[4]: the query-row sharded CorrBlock's exchange (rowshard.py) ----
 * Reassembly after an all-gather of `world` fixed-size chunks: chunk r (floats [r*chunk,
 * (r+1)*chunk) of `chunks`) starts with rank r's rows as float[B][C][rows_r][W], where rows_r is
 * the contiguous near-equal partition of H (the first H % world ranks own H/world + 1 rows, rank r
 * starts at row r*(H/world) + min(r, H % world)); the rest of the chunk is padding.  Writes
 * out float[B][C][H][W].  chunk >= B*C*ceil(H/world)*W and H >= world (else ECORR_EINVAL).
 * Replaces: the torch.cat reassembly of the per-iteration lookup all-gather (the reference
 * keeps the GRU replicated, eraft.py:128-132, so every rank needs the full map). */
int ecorr_rows_assemble(const float* chunks, int64_t chunk, int world, int B, int C, int H, int W,
                        float* out, void* stream);

/* ---- the warm-start splat (utils/image_utils.py) ----
 * Deterministic and bit-exact with the reference's serial CPU put_(accumulate=True): the scatter
 * runs as a counting sort + ordered gather in a caller-provided workspace. */

/* Workspace bytes for B items of n points splatted onto an h x w grid (B = 1 for
 * ecorr_grid_sample_values, n = h*w for ecorr_forward_interpolate). */
int ecorr_splat_workspace_size(int B, int64_t n, int h, int w, int64_t* bytes);

/* forward_interpolate_pytorch: flow float[B][2][h][w] -> out float[B][2][h][w]; every pixel moves
 * to (col + dx, row + dy) and is splatted bilinearly; pixels nothing lands on read 0.
 * Replaces: utils/image_utils.py:50-83 (and its per-sample Python loop, :78-80). */
int ecorr_forward_interpolate(const float* flow, int B, int h, int w, float* out, void* workspace,
                              void* stream);

/* grid_sample_values: pts float[3][n] rows x, y, z -> values float[h][w] (interpolated z) and
 * valid uint8[h][w] (nullable; 1 where some weight landed).  0 <= n < 2^24.
 * Replaces: utils/image_utils.py:10-47. */
int ecorr_grid_sample_values(const float* pts, int64_t n, int h, int w, float* values, uint8_t* valid,
                             void* workspace, void* stream);

/* ---- convex upsampling and the DSEC 16-bit PNG flow codec ---- */

/* ERAFT.upsample_flow: flow float[N][2][H][W], mask float[N][576][H][W] (the update block's
 * 0.25 * mask head) -> out float[N][2][8H][8W]; softmax over the 9 taps, convex combination of
 * the zero-padded 3x3 window of 8 * flow.  Within a few ulp of the reference (device expf).
 * out must be 16-byte aligned (it is stored as 16-byte vectors; every row of it then is, 8W floats
 * long); flow and mask need a float's alignment only.  A misaligned out is ECORR_EINVAL, as null
 * pointers and N, H, W outside N <= 65535, H * W <= 2^26 are, before any launch.
 * Non-finite values keep the reference's footprint.  A NaN in flow[n][c][y][x] makes channel c NaN on
 * the 8x8 blocks of the pixels of its 3x3 neighbourhood inside the map (a weight times NaN), and +-inf
 * there gives +-inf on those blocks, NaN where +inf and -inf meet or a weight is 0; the other channel,
 * the other items and every other pixel keep the bits of the finite run.  A sub-pixel whose nine logits
 * hold a NaN, a +inf, or nothing but -inf has both its outputs (c = 0, 1) NaN and touches nothing else
 * (the maximum is taken with fmaxf, which drops a NaN, and the NaN returns through the sum); a -inf
 * logit beside finite ones is a weight of exactly 0.
 * Replaces: model/eraft.py:74-85. */
int ecorr_upsample_flow(const float* flow, const float* mask, int N, int H, int W, float* out, void* stream);

/* The backward of ecorr_upsample_flow (two entries added within ABI 17: purely additive, the version
 * is unchanged).  grad_out float[N][2][8H][8W] contiguous, flow and mask the forward's inputs ->
 * grad_flow float[N][2][H][W] and grad_mask float[N][576][H][W].  Either of the two may be NULL and is
 * then not computed; both NULL is ECORR_EINVAL.  Every element of a non-null output is overwritten
 * (never accumulated into), and nothing else is written but the workspace.  The softmax is recomputed
 * from mask by the forward's definition (nothing mask-sized is saved).  Deterministic: no float
 * atomics, one writer per output cell and a fixed summation order (j, then i, then k ascending), so
 * equal inputs give bitwise equal gradients.  workspace: ecorr_upsample_backward_workspace_size bytes
 * of device memory (float[N][18][H*W], contents undefined before and after), required whichever
 * gradients are asked for; NULL is ECORR_EINVAL.  N, H, W as ecorr_upsample_flow (N <= 65535,
 * H * W <= 2^26, any H, W >= 1).  grad_out must be 16-byte aligned (it is read as 16-byte vectors);
 * a misaligned grad_out is ECORR_EINVAL.  Validation happens before any launch.
 * Replaces: autograd of eraft.py:74-85. */
int ecorr_upsample_backward_workspace_size(int N, int H, int W, int64_t* bytes);
int ecorr_upsample_flow_backward(const float* grad_out, const float* flow, const float* mask, int N, int H, int W,
                                 float* grad_flow, float* grad_mask, void* workspace, void* stream);

/* DSEC submission encoding: flow float[B][2][h][w] -> out uint16[B][h][w][3] =
 * (u16)rint(flow * 128 + 2^15) with numpy's x86 float32 -> uint16 cast, channel 2 = 0.
 * Bit-exact.  Replaces: utils/visualization.py:81-84 (before imageio.imwrite). */
int ecorr_flow_to_png16(const float* flow, int B, int h, int w, uint16_t* out, void* stream);

/* DSEC ground-truth decoding: in uint16[B][h][w][3] -> flow float[B][h][w][2] = (v - 2^15) / 128
 * where channel 2 == 1 (else 0), valid uint8[B][h][w] = channel 2 == 1.  *bad (device int, zeroed
 * by the caller) counts pixels whose channel 2 is neither 0 nor 1 (the reference asserts).
 * Bit-exact.  Replaces: utils/dsec_utils.py:66-83 (after imageio.imread). */
int ecorr_png16_to_flow(const uint16_t* in, int B, int h, int w, float* flow, uint8_t* valid, int* bad,
                        void* stream);

/* ---- event stream -> voxel grid ----
 * The accumulated grid is bit-exact with the reference's single-threaded serial fold (stable sort
 * of the events by base cell + ordered per-cell gather); normalization (nonzero mean / unbiased
 * std) agrees within an ulp or two.  n >= 1 events; voxel float[C][H][W]. */

/* Workspace bytes for n events on a C x H x W grid (dsec != 0: ecorr_voxel_grid_dsec, else
 * ecorr_voxel_grid_mvsec). */
int ecorr_voxel_workspace_size(int dsec, int64_t n, int C, int H, int W, int64_t* bytes);

/* VoxelGrid.convert: p, t, x, y float[n] (t ascending), trilinear in (x, y, t).
 * Replaces: utils/dsec_utils.py:26-64 (as called by loader/loader_dsec.py:245-257). */
int ecorr_voxel_grid_dsec(const float* p, const float* t, const float* x, const float* y, int64_t n, int C,
                          int H, int W, int normalize, float* voxel, void* workspace, void* stream);

/* EventSequenceToVoxelGrid_Pytorch: events double[n][4] = (t, x, y, p), bilinear in t.
 * *bad_index (device int, zeroed by the caller) becomes nonzero where the reference's index_add_
 * would raise (an index outside the grid); the grid is then undefined.
 * Replaces: utils/transformers.py:36-126. */
int ecorr_voxel_grid_mvsec(const double* events, int64_t n, int C, int H, int W, int normalize, float* voxel,
                           int* bad_index, void* workspace, void* stream);

/* ---- Volume-free correlation (three entries added within ABI 17: purely additive, the version stays 17) ----
 * The lookup of ecorr_build + ecorr_lookup without the all-pairs volume (csrc/alt.hip): the block keeps
 * the feature maps, channel-last, and every lookup computes the correlation values its samples need.
 * avg_pool2d over the target axes is linear, so level i of the volume is fmap1^T pool^i(fmap2) / sqrt(D)
 * with the pyramid's own floor-halving 2 x 2 mean; the arithmetic is reordered, so a result equals the
 * volume lookup's up to rounding, not bit for bit, while sample positions, NaN samples, exact zeros and
 * contributing corners are the volume lookup's by construction (the same device functions).  A corner
 * value is an fp32 dot product of the query's features with one pooled fmap2 pixel, then the build's
 * scale step (/ sqrtf(D), a multiply where that is a power of two).  No atomics: bitwise reproducible.
 *
 * Feature buffer (ecorr_alt_size floats, 16-byte aligned), Dp = D rounded up to a multiple of 4, pad
 * channels zero:  fmap1 as float[B][H*W][Dp], then for each level i the pooled fmap2 as
 * float[B][h_i*w_i][Dp], h_i = H >> i, w_i = W >> i, pooled level from level as (((a+b)+c)+d) * 0.25f.
 * ecorr_alt_pack_as reads fmaps of fmap_format (ECORR_ELEM_*: the conversion is exact) in the build's
 * [B][D][H][W] order.  ecorr_alt_lookup_as: coords float[B][2][H*W]; out: B * levels*(2r+1)^2 * H*W
 * elements of out_format (ECORR_OUT_*) in ecorr_lookup's order, each the fp32 sample rounded once.
 * Radii <= 4 run one wave per (query, level): at most (2r+3)^2 window dot products, then the blends;
 * larger radii, and queries whose window does not fit (NaN / inf / huge coordinates), compute the
 * up to four in-image corner dots of each sample.
 * Errors (before any GPU call), all ECORR_EINVAL: a null pointer, B, D, H or W < 1, levels outside
 * [1, ECORR_MAX_LEVELS], a level of 0 pixels, radius outside [0, 32], an unknown format, a feature buffer
 * that is not 16-byte aligned, and a level of one batch item beyond 2^31 bytes (h_i*w_i*Dp*4). */
int ecorr_alt_size(int B, int D, int H, int W, int levels, int64_t* floats);
int ecorr_alt_pack_as(const void* fmap1, const void* fmap2, int fmap_format, int B, int D, int H, int W,
                      int levels, float* feat, void* stream);
int ecorr_alt_lookup_as(const float* feat, const float* coords, int B, int D, int H, int W, int levels,
                        int radius, void* out, int out_format, void* stream);

/* The backward of the volume-free lookup (three more entries added within ABI 17, csrc/alt_grad.hip):
 * the gradients of the two fmaps without a gradient pyramid.  With s = 1/sqrt(D), F2_i the pooled fmap2
 * level i and Wg_i[p] the (2r+3)^2 window gradient of query p on level i (ecorr_lookup_backward's window:
 * the same device function), grad_f1[p,:] = s sum_i sum_t Wg_i[p][t] F2_i[t,:], grad_F2_i[t,:] = s sum_p
 * Wg_i[p][t] f1[p,:], and grad_fmap2 is the fold of the grad_F2_i onto level 0 (the chain of floor-mode
 * avg_pool2d backwards).  No atomics: the destination owns every sum and each runs in a fixed order,
 * so equal inputs give bitwise equal gradients.  Queries with NaN / inf / huge coordinates contribute
 * nothing.  First order only; there is no gradient with respect to coords.
 * grad_feat: ecorr_alt_size floats in the feature buffer's layout, 16-byte aligned.  Workspace:
 * ecorr_alt_backward_workspace_size bytes, 16-byte aligned -- per (batch item, level, query) two ints of
 * window origin and (2r+3)^2 floats of window, B*levels*H*W*(8 + 4 (2r+3)^2) bytes; it needs no
 * initialisation.  Radius 0 .. 32 (the forward window kernel's 128-tap limit does not apply).
 * Errors (before any GPU call), all ECORR_EINVAL: those of ecorr_alt_lookup_as, and a null or misaligned
 * grad_feat or workspace. */
int ecorr_alt_backward_workspace_size(int B, int H, int W, int levels, int radius, int64_t* bytes);
/* grad_feat += one lookup's contribution (grad_feat: ecorr_alt_size floats in the feature buffer's layout,
 * zeroed by the caller before the block's first call; calls on one grad_feat stream-ordered).
 * grad_out float[B][levels*(2r+1)^2][H*W].  workspace: contents undefined before and after. */
int ecorr_alt_lookup_backward(const float* feat, const float* coords, const float* grad_out, int B, int D,
                              int H, int W, int levels, int radius, float* grad_feat, void* workspace, void* stream);
/* Consumes grad_feat (the pooled fmap2 levels are folded onto level 0 in place).
 * grad_fmap1 / grad_fmap2 float[B][D][H][W]; either may be NULL. */
int ecorr_alt_pack_backward(float* grad_feat, int B, int D, int H, int W, int levels,
                            float* grad_fmap1, float* grad_fmap2, void* stream);

/* ---- SepConvGRU (four entries added within ABI 17: purely additive, the version stays 17) ----
 * The update block's separable ConvGRU (model/update.py:33-60, csrc/gru.hip): a half-step along x with
 * the (1,5) convolutions z1 r1 q1, then one along y with the (5,1) convolutions z2 r2 q2, zero padding 2:
 *   z = sigmoid(conv_z([h, x])), r = sigmoid(conv_r([h, x])), q = tanh(conv_q([r*h, x])), h' = (1-z)*h + z*q.
 * h float[B][hidden][H][W], x float[B][input][H][W], h_out float[B][hidden][H][W], contiguous fp32; h and x
 * are read in place (no concatenation).  Supported sizes: hidden = 128 and input = 256 only (the update
 * block's); every other (hidden, input) returns ECORR_EINVAL from all four entries.  H = 1 and W = 1 are
 * valid (every off-centre tap is then padding).  Forward only (the gradients: ecorr_sepconv_gru_backward).
 * Arithmetic: the products run on the fp32 matrix instruction (exact fp32 operands, fp32 accumulation in
 * chains of 192 products that are then summed), sigmoid as 1 / (1 + expf(-v)), tanhf, the blend as two
 * products and a sum: within 1e-5 of an fp64 GRU, normwise (max |error| / rms).  No atomics: bitwise
 * reproducible.  Non-finite values: a NaN in h or x makes the outputs of its own batch item NaN on
 * exactly the reference's footprint (the 9 x 9 block around the pixel, clipped to the image, all channels:
 * two taps per half-step, and two more because r*h carries it into q's taps) and nowhere else -- there is
 * no shared exponent to spread it; +-inf behaves as in an fp32
 * convolution (inf * 0 weight = NaN; no split, so no inf - inf of the split kernels).
 * Packed weights: ecorr_sepconv_gru_packed_size bytes = 4 * (6 * hidden * (hidden + input) * 5 + 6 * hidden),
 * 16-byte aligned; written once per weight set by ecorr_sepconv_gru_pack (one launch) from weight[i]
 * float[hidden][hidden + input][5] and bias[i] float[hidden], i in the order z1 r1 q1 z2 r2 q2 (a (1,5)
 * and a (5,1) kernel both flatten to that).  The arrays of six pointers are host arrays of device pointers.
 * Workspace: ecorr_sepconv_gru_workspace_size bytes = 3 * B * hidden * H * W * 4 (the first half-step's h,
 * z and r*h), 16-byte aligned; it needs no initialisation and its contents are undefined afterwards.
 * ecorr_sepconv_gru: four launches on `stream`, no host synchronisation, no allocation.
 * Errors (before any GPU call), all ECORR_EINVAL: a null pointer (an array entry included), an unsupported
 * (hidden, input), B, H or W < 1, B > 65535, B * (hidden + input) * H * W * 4 beyond 2^31 - 1 (the buffer
 * range of the kernels' 32-bit offsets), a packed buffer or workspace that is not 16-byte aligned, h_out
 * overlapping h or x, and the workspace overlapping h, x or h_out, or the packed buffer overlapping the
 * workspace or h_out: the five buffers must be disjoint, except that h and x are only read and may share
 * memory with each other or with the pack. */
int ecorr_sepconv_gru_packed_size(int hidden, int input, int64_t* bytes);
int ecorr_sepconv_gru_pack(const float* const weight[6], const float* const bias[6],
                           int hidden, int input, void* packed, void* stream);
int ecorr_sepconv_gru_workspace_size(int B, int hidden, int input, int H, int W, int64_t* bytes);
int ecorr_sepconv_gru(const float* h, const float* x, int B, int hidden, int input, int H, int W,
                      const void* packed, float* h_out, void* workspace, void* stream);

/* ---- SepConvGRU backward (four entries added within ABI 17: purely additive, the version stays 17) ----
 * The gradients of ecorr_sepconv_gru (csrc/gru_grad.hip), first order, fp32, the same sizes (hidden = 128 and
 * input = 256 only) and geometry limits.  Given h, x (the forward's inputs) and grad_out = dL/dh_out
 * float[B][hidden][H][W], per half-step (the y half-step first, its grad_h is the x half-step's grad_out):
 *   gq = g z (1 - q^2), gz = g (q - h) z (1 - z), [g_rh; gx_q] = conv_q^T(gq), gr = g_rh h r (1 - r),
 *   [gh_zr; gx_zr] = conv_zr^T([gz; gr]), grad_h = g (1 - z) + g_rh r + gh_zr, grad_x = gx_q + gx_zr (summed
 *   over both half-steps), grad_weight[o][c][t] = sum over batch items and pixels p of gpre[o][p] in[c][p + (t-2) e]
 *   (valid shifted pixels only), grad_bias[o] = the sum of gpre[o][p].
 * Nothing but h and x is kept from the forward: the call recomputes h1 and the six gates with the forward's
 * kernels (the recomputed h_out is bitwise the forward's), so `packed` (ecorr_sepconv_gru_pack) is needed too.
 * Outputs: grad_h float[B][hidden][H][W], grad_x float[B][input][H][W], each may be NULL (not wanted);
 * grad_weight[i] float[hidden][hidden + input][5] and grad_bias[i] float[hidden], i in the order z1 r1 q1 z2
 * r2 q2 (host arrays of six device pointers), both arrays NULL (a frozen GRU: the weight GEMMs are skipped) or
 * both complete.  Every element of a wanted output is overwritten.
 * Arithmetic: the fp32 matrix instruction; data gradients in chains of 160 products that are then summed,
 * weight gradients in chains of at most 1024 pixels, summed per slab and then over the slabs in ascending
 * order; a slab is a run of pixels of one batch item whose length depends on B, H and W alone.  No atomics:
 * bitwise reproducible.
 * Transposed pack: ecorr_sepconv_gru_backward_packed_size bytes = 4 * 6 * hidden * (hidden + input) * 5, 16-byte
 * aligned, written once per weight set by ecorr_sepconv_gru_backward_pack (one launch).
 * Workspace: ecorr_sepconv_gru_backward_workspace_size bytes, 16-byte aligned, no initialisation needed, contents
 * undefined afterwards except as stated here.  With n = B * hidden * H * W * 4 bytes and P = H * W:
 *   13 * n                                       h1 z1 r1 q1 z2 r2 q2 h_out' | r*h | gq | gz gr | grad_h1
 *   + align256(B * ceil(P / 64) * 384 * 4)       bias partials
 *   + B * nsl * 5 * 256 * 384 * 4                weight slab partials
 * where cap = 1024, doubled while cap < P and B * ceil(P / cap) > 64; slab = ceil(ceil(P / ceil(P / cap)) / 32) * 32;
 * nsl = ceil(P / slab); align256 rounds up to a multiple of 256.  After the call the first 8 * n bytes hold the
 * recomputed h1, z1, r1, q1, z2, r2, q2 and h_out, each float[B][hidden][H][W].
 * ecorr_sepconv_gru_backward: stream-ordered launches on `stream`, no host synchronisation, no allocation.
 * Errors (before any GPU call), all ECORR_EINVAL: those of ecorr_sepconv_gru (sizes, geometry, null h, x,
 * packed, workspace; misaligned packed or workspace), a null grad_out or packed_t, a misaligned packed_t, all
 * of grad_h, grad_x and grad_weight NULL, exactly one of grad_weight and grad_bias NULL, a NULL entry in
 * either array, an output overlapping h, x, grad_out, a pack, the workspace or another output, and the
 * workspace overlapping h, x, grad_out or a pack. */
int ecorr_sepconv_gru_backward_packed_size(int hidden, int input, int64_t* bytes);
int ecorr_sepconv_gru_backward_pack(const float* const weight[6], int hidden, int input, void* packed_t, void* stream);
int ecorr_sepconv_gru_backward_workspace_size(int B, int hidden, int input, int H, int W, int64_t* bytes);
int ecorr_sepconv_gru_backward(const float* h, const float* x, const float* grad_out,
                               int B, int hidden, int input, int H, int W,
                               const void* packed, const void* packed_t,
                               float* grad_h, float* grad_x,
                               float* const grad_weight[6], float* const grad_bias[6],
                               void* workspace, void* stream);

/* ---- Motion encoder (four entries added within ABI 17: purely additive, the version stays 17) ----
 * BasicMotionEncoder behind convc1 (model/update.py:68-81, csrc/motion_enc.hip), zero padding throughout:
 *   cor = relu(convc2(c1))  3x3, 256 -> 192      f1  = relu(convf1(flow))  7x7, 2 -> 128
 *   flo = relu(convf2(f1))  3x3, 128 -> 64       out = [relu(conv([cor, flo])), flow]  3x3, 256 -> 126, then flow's 2
 * c1 float[B][256][H][W] = relu(convc1(corr)) (ecorr_lookup_conv1x1_relu*, or any producer), flow float[B][2][H][W],
 * both contiguous fp32 and only read.  out: batch item b is float[128][H][W] at out + b * out_batch_stride (in
 * floats, >= 128 * H * W), so out may be the upper half of the GRU's x float[B][256][H][W] (out = x + 128 * H * W,
 * out_batch_stride = 256 * H * W) and neither concatenation runs.  H = 1 and W = 1 are valid (every off-centre
 * tap is then padding).  Forward only (the gradients: ecorr_motion_encoder_backward).
 * Arithmetic: the three 3x3 convolutions run on the fp32 matrix instruction (exact fp32 operands, fp32
 * accumulation in chains of 192 products -- 12 chains for convc2 and conv, 6 for convf2 -- that are then summed),
 * convf1 as one k-ordered fmaf chain of 98 products; the bias is added last; relu is v < 0 ? 0 : v: within 1e-5 of
 * an fp64 encoder on channels 0-125, normwise (max |error| / rms).  Channels 126 and 127 of out are flow, copied
 * bit for bit.  No atomics: bitwise reproducible, and a batch item's result does not depend on B.
 * Non-finite values: relu keeps a NaN (as torch.relu does), and there is no shared exponent to spread one: a NaN
 * in c1 makes channels 0-125 NaN on the 5 x 5 block around its pixel (two 3x3 convolutions), a NaN in flow on the
 * 11 x 11 block (7x7, then two 3x3) and in its own flow channel at its own pixel, each clipped to the image and
 * within its own batch item -- the reference's footprint, nothing more.  +-inf behaves as in an fp32
 * convolution (inf * 0 weight = NaN).
 * Packed weights: ecorr_motion_encoder_packed_size bytes = 4 * (9 * 256 * 192 + 9 * 128 * 64 + 9 * 256 * 128 +
 * 128 * 100 + 512) = 3297280 (convc2, convf2 and conv with its 126 rows padded to 128 by zero rows, convf1's rows of
 * 98 padded to 100, the biases 192 + 128 + 64 + 128), 16-byte aligned; written once per weight set by
 * ecorr_motion_encoder_pack (one launch).  weight and bias are host arrays of four device pointers.
 * Workspace: ecorr_motion_encoder_workspace_size bytes = 384 * B * H * W * 4 (cor, f1 and flo), 16-byte aligned;
 * it needs no initialisation and its contents are undefined afterwards.
 * ecorr_motion_encoder: four launches on `stream`, no host synchronisation, no allocation.
 * Errors (before any GPU call), all ECORR_EINVAL: a null pointer (an array entry included), a packed buffer or
 * workspace that is not 16-byte aligned, B, H or W < 1, B > 65535, 256 * H * W * 4 beyond 2^31 - 1 (H * W >
 * 2097151: the buffer range of the kernels' 32-bit offsets within one batch item; the batch offsets are 64-bit),
 * out_batch_stride < 128 * H * W (or beyond 2^40), out's whole strided extent ((B - 1) * out_batch_stride +
 * 128 * H * W floats) overlapping c1, flow, the pack or the workspace, and the workspace overlapping c1, flow or
 * the pack.  c1 and flow may share memory with each other or with the pack. */
int ecorr_motion_encoder_packed_size(int64_t* bytes);
int ecorr_motion_encoder_pack(const float* const weight[4], const float* const bias[4], void* packed, void* stream);
        /* order: convc2 convf1 convf2 conv; weight shapes [192][256][3][3] [128][2][7][7] [64][128][3][3] [126][256][3][3] */
int ecorr_motion_encoder_workspace_size(int B, int H, int W, int64_t* bytes);
int ecorr_motion_encoder(const float* c1, const float* flow, int B, int H, int W, const void* packed,
                         float* out, int64_t out_batch_stride, void* workspace, void* stream);

/* ---- Motion encoder backward (four entries added within ABI 17: purely additive, the version stays 17) ----
 * The gradients of ecorr_motion_encoder (csrc/motion_enc_grad.hip), first order, fp32, the same geometry limits.
 * Given c1, flow (the forward's inputs) and grad_out = dL/dout, batch item b float[128][H][W] at grad_out + b *
 * grad_out_batch_stride (in floats, >= 128 * H * W: it may be the upper half of the GRU's grad_x), with
 * relu'(y) v = (y <= 0 ? 0 : v) on the ReLU's output y (a NaN y passes v, an exact 0 gives 0):
 *   go = relu'(o) grad_out[:126], [gcor; gflo] = conv^T(go), gc2 = relu'(cor) gcor, gf2 = relu'(flo) gflo,
 *   grad_c1 = convc2^T(gc2), gf1 = relu'(f1) convf2^T(gf2), grad_flow = convf1^T(gf1) + grad_out[126:128],
 *   grad_weight[o][c][ky][kx] = sum over batch items and pixels p of gpre[o][p] in[c][p + (ky, kx) - reach] (valid
 *   shifted pixels only), grad_bias[o] = the sum of gpre[o][p]; (gpre, in) = (go, [cor, flo]) for conv, (gc2, c1) for
 *   convc2, (gf2, f1) for convf2, (gf1, flow) for convf1.
 * Nothing but c1 and flow is kept from the forward: the call recomputes f1, cor and flo with the forward's kernels,
 * so `packed` (ecorr_motion_encoder_pack) is needed too; conv's recompute writes go directly.
 * Outputs: grad_c1 float[B][256][H][W], grad_flow float[B][2][H][W], each may be NULL (not wanted; a NULL grad_flow
 * skips convf1's data gradient); grad_weight[i] and grad_bias[i] in the shapes and the order of
 * ecorr_motion_encoder_pack (convc2 convf1 convf2 conv; host arrays of four device pointers), both arrays NULL (a
 * frozen encoder: every weight GEMM and bias pass is skipped) or both complete.  Every element of a wanted output is
 * overwritten.
 * Arithmetic: the fp32 matrix instruction; the three 3x3 data gradients in chains of 192 products that are then
 * summed (6 chains for conv^T, 9 for convc2^T, 3 for convf2^T); convf1^T on the VALU, per output one chain of 49
 * products per f1 channel, the channels added in ascending order in four groups of 32, the groups in ascending
 * order, grad_out's flow channels last; weight gradients in chains of at most 1024 pixels, summed per slab and then
 * over the slabs in ascending order, a slab being a run of pixels of one batch item whose length depends on B, H and
 * W alone; bias gradients as sums of 64 pixels added in ascending order.  No atomics: bitwise reproducible, and a
 * batch item's grad_c1 and grad_flow do not depend on B.
 * Transposed pack: ecorr_motion_encoder_backward_packed_size bytes = 4 * 9 * (256 * 128 + 256 * 192 + 128 * 64) =
 * 3244032 (conv^T with its 126 reduction rows padded to 128, convc2^T, convf2^T; convf1 has none), 16-byte aligned,
 * written once per weight set by ecorr_motion_encoder_backward_pack (one launch).
 * Workspace: ecorr_motion_encoder_backward_workspace_size bytes, 16-byte aligned, no initialisation needed, contents
 * undefined afterwards.  With n = B * H * W * 4 bytes and P = H * W:
 *   896 * n                                      cor 192, f1 128, flo 64 | go 128 | gc2 192, gf2 64 | gf1 128
 *   + align256(B * ceil(P / 64) * 512 * 4)       bias partials
 *   + B * nsl * 9 * 192 * 256 * 4                weight slab partials (the largest gradient's; the four take turns)
 * where cap = 1024, doubled while cap < P and B * ceil(P / cap) > 64; slab = ceil(ceil(P / ceil(P / cap)) / 32) * 32;
 * nsl = ceil(P / slab); align256 rounds up to a multiple of 256 (the slab rule of ecorr_sepconv_gru_backward).
 * ecorr_motion_encoder_backward: stream-ordered launches on `stream`, no host synchronisation, no allocation.
 * Errors (before any GPU call), all ECORR_EINVAL: those of ecorr_motion_encoder (geometry: B, H or W < 1, B > 65535,
 * H * W > 2097151; null c1, flow, packed, workspace; misaligned packed or workspace), a null grad_out or packed_t, a
 * misaligned packed_t, grad_out_batch_stride < 128 * H * W (or beyond 2^40), all of grad_c1, grad_flow and
 * grad_weight NULL, exactly one of grad_weight and grad_bias NULL, a NULL entry in either array, an output
 * overlapping c1, flow, grad_out's whole strided extent ((B - 1) * grad_out_batch_stride + 128 * H * W floats), a
 * pack, the workspace or another output, and the workspace overlapping c1, flow, that extent or a pack. */
int ecorr_motion_encoder_backward_packed_size(int64_t* bytes);
int ecorr_motion_encoder_backward_pack(const float* const weight[4], void* packed_t, void* stream);
int ecorr_motion_encoder_backward_workspace_size(int B, int H, int W, int64_t* bytes);
int ecorr_motion_encoder_backward(const float* c1, const float* flow, const float* grad_out,
                                  int64_t grad_out_batch_stride, int B, int H, int W,
                                  const void* packed, const void* packed_t,
                                  float* grad_c1, float* grad_flow,
                                  float* const grad_weight[4], float* const grad_bias[4],
                                  void* workspace, void* stream);

/* Tile shape of the pyramid storage (ECORR_TILE_H, ECORR_TILE_W). */
int ecorr_pyramid_tile(int* tile_h, int* tile_w);

/* Storage format of each level of an H x W pyramid: ntx[i] = tiles per tile row (tiled), 0
 * (compact row-major) or -nbx (interleaved, nbx blocks per block row).  Same errors as
 * ecorr_pyramid_layout. */
int ecorr_pyramid_formats(int H, int W, int levels, int* ntx);

/* Human-readable name of a status code (static storage). */
const char* ecorr_strerror(int status);

/* ECORR_ABI_VERSION of the loaded library. */
int ecorr_abi_version(void);

#ifdef __cplusplus
}
#endif
#endif /* ECORR_H */
