// ecorr_device.h -- device helpers shared by the build and lookup kernels (gfx950 only).
//
// Exactness contract: every helper below performs the reference's fp32 operations in the
// reference's order with explicit round-to-nearest intrinsics, so no -ffp-contract setting or
// compiler reassociation can change a bit.  The library is additionally compiled with
// -ffp-contract=off.
#pragma once
#include <hip/hip_runtime.h>
#include <stdint.h>

#include "../../include/ecorr.h"

namespace ecorr {

constexpr int kWave = 64;

// Pyramid level storage (include/ecorr.h): each query's level image [h][w] is stored as
// row-major 4 x 8-float tiles (128 B = one L2 line); ntx = padded width / 8 tiles per tile row.
constexpr int kTileH = 4, kTileW = 8, kTile = kTileH * kTileW;
// float offset of tile (tr, tc)'s line in a query image
__host__ __device__ __forceinline__ int tile_base(int tr, int tc, int ntx) { return (tr * ntx + tc) * kTile; }
// pixel (y, x) = tile_base(y >> 2, x >> 3, ntx) + in-tile offset, spelled out (the call reorders kernels)
__host__ __device__ __forceinline__ int tiled_off(int y, int x, int ntx) {
    return (((y >> 2) * ntx + (x >> 3)) << 5) + ((y & 3) << 3) + (x & 7);
}
// its inverse: pixel (y, x) of stored cell c (a padding cell's pixel lies outside the image)
__host__ __device__ __forceinline__ void tiled_cell_yx(int c, int ntx, int& y, int& x) {
    const int tile = c >> 5;
    y = (tile / ntx) * kTileH + ((c >> 3) & 3);
    x = (tile % ntx) * kTileW + (c & 7);
}
__host__ __device__ __forceinline__ int pad_h(int h) { return (h + kTileH - 1) & ~(kTileH - 1); }
__host__ __device__ __forceinline__ int pad_w(int w) { return (w + kTileW - 1) & ~(kTileW - 1); }

// Levels 1-3 are interleaved (below), so only level 0 and levels >= 4 are tiled, and only levels
// >= 4 can be compact: those whose tile padding would exceed half the image are stored row-major
// instead (the window covers most of such an image, so the padding would only add lines to every
// lookup's read footprint).
__host__ __device__ __forceinline__ bool level_ilv(int level) { return level >= 1 && level <= 3; }
__host__ __device__ __forceinline__ bool level_compact(int level, int h, int w) {
    return level >= 4 && 2 * pad_h(h) * pad_w(w) > 3 * h * w;
}

// Offset of pixel (y, x) in one query image: tiled (ntx = tiles per tile row > 0) or row-major
// (ntx <= 0, width w).
__host__ __device__ __forceinline__ int level_off(int y, int x, int ntx, int w) {
    return ntx > 0 ? tiled_off(y, x, ntx) : y * w + x;
}

// Levels 1-3 are stored interleaved (ntx = -nbx < 0): query rows in groups of kGroup = 64, and a
// group holds, for each bh x bw block of the level image (2 x 4 at levels 1 and 2, 1 x 2 at level
// 3: what one 8 x 16 target block of level 0 pools to at levels 2 and 3), that block of its 64 rows
// back to back: [group][block][row][bh][bw], blocks row-major (nbx per block row).  One build tile
// then writes each block of its 256 query rows as whole lines (the per-row pieces are 32 / 8
// bytes), and the lookup reads a window's blocks with lines shared by adjacent queries.
constexpr int kGroup = ECORR_ROW_GROUP;
__host__ __device__ __forceinline__ int ilv_sy(int lv) { return lv == 3 ? 0 : 1; }   // log2 block height
__host__ __device__ __forceinline__ int ilv_sx(int lv) { return lv == 3 ? 1 : 2; }   // log2 block width
__host__ __device__ __forceinline__ int ilv_bsz(int lv) { return 1 << (ilv_sy(lv) + ilv_sx(lv)); }   // block floats
// The format's one definition: the float offset of pixel (y, x) of query row R in a level of nbx
// blocks per block row and sz floats per query image, from the first float of 64-row group g0.  It
// is the sum of a row term (this function at pixel (0, 0)) and a cell term (at row 0, sz 0), which
// the build epilogues take apart: the cell term hoisted out of their query loops.
__host__ __device__ __forceinline__ int64_t ilv_pix_off(int64_t R, int64_t g0, int y, int x, int lv, int nbx,
                                                        int64_t sz) {
    const int sy = ilv_sy(lv), sx = ilv_sx(lv);
    return ((R >> 6) - g0) * (kGroup * sz) +
           ((int64_t)((y >> sy) * nbx + (x >> sx)) * kGroup + (R & (kGroup - 1))) * (1 << (sy + sx)) +
           ((y & ((1 << sy) - 1)) << sx) + (x & ((1 << sx) - 1));
}
__host__ __device__ __forceinline__ int64_t ilv_row_off(int64_t R, int64_t g0, int lv, int64_t sz) {
    return ilv_pix_off(R, g0, 0, 0, lv, 0, sz);
}
__host__ __device__ __forceinline__ int64_t ilv_cell_off(int y, int x, int lv, int nbx) {
    return ilv_pix_off(0, 0, y, x, lv, nbx, 0);
}
// whether pixel (y, x)'s block exists in a level of nby x nbx blocks
__host__ __device__ __forceinline__ bool ilv_cell_in(int y, int x, int lv, int nby, int nbx) {
    return (y >> ilv_sy(lv)) < nby && (x >> ilv_sx(lv)) < nbx;
}

// Float offset of pixel (y, x) of query row R (0 .. B*q_count - 1) from the level's base, any
// format; sz = floats per query image (an interleaved group spans kGroup * sz floats).
__host__ __device__ __forceinline__ int64_t pix_off(int64_t R, int y, int x, int lv, int ntx, int w, int64_t sz) {
    if (ntx >= 0) return R * sz + level_off(y, x, ntx, w);
    return ilv_pix_off(R, 0, y, x, lv, -ntx, sz);
}

// The slab of a level that holds query rows [R0, R0 + nq), any format (ilv: interleaved), which a
// buffer descriptor over those rows spans: its first float from the level's base and its bytes --
// the 64-row groups the rows touch, from group g0 (which ilv_pix_off counts from), else the nq images.
__host__ __device__ __forceinline__ int64_t slab_g0(int64_t R0) { return R0 >> 6; }
__host__ __device__ __forceinline__ int64_t slab_first(bool ilv, int64_t R0, int64_t sz) {
    return ilv ? slab_g0(R0) * kGroup * sz : R0 * sz;
}
__host__ __device__ __forceinline__ int64_t slab_bytes(bool ilv, int64_t R0, int nq, int64_t sz) {
    return (ilv ? (((R0 + nq - 1) >> 6) - slab_g0(R0) + 1) * kGroup * sz : nq * sz) * 4;
}

// model/utils.py:11-12 then ATen grid_sampler unnormalize (align_corners=True):
//   g  = RN(RN(2x / (size-1)) - 1)
//   ix = RN(RN(g + 1) * ((size-1)/2))
// 2x and (size-1)/2 are exact; the division is IEEE (v_div_scale/fmas/fixup sequence).
__device__ __forceinline__ float unnormalize(float x, float size_m1, float half_size_m1) {
    const float g = __fsub_rn(__fdiv_rn(__fmul_rn(2.0f, x), size_m1), 1.0f);
    return __fmul_rn(__fadd_rn(g, 1.0f), half_size_m1);
}

// The build's scale step on a finished sum (abi.hip scale_step_of): / sqrtf(D), as a multiply where
// sqrtf(D) is a power of two (scale is then 1 / sqrtf(D)).  The volume-free lookup and its backward.
__device__ __forceinline__ float scale_step(int is_mul, float scale, float s) {
    return is_mul ? __fmul_rn(s, scale) : __fdiv_rn(s, scale);
}

// One coordinate chain of the lookup (corr.py:41-43, utils.py:11-12, grid_sampler unnormalize): the
// tap at offset d = o - r (o = 0 .. 2r) of the axis whose scaled coordinate is cs = coords / 2^lv, on
// a level side of m1 + 1 pixels -> floor and fraction.  The forward (lookup_stage.h coord_chain<R>)
// and the backward (grad.hip) both call this, so their supports cannot differ.
__device__ __forceinline__ void coord_chain(float cs, int d, float m1, float& f, float& wgt) {
    const float c = __fadd_rn(cs, (float)d);
    const float v = unnormalize(c, m1, m1 * 0.5f);
    f = floorf(v);
    wgt = __fsub_rn(v, f);
}

// Whether the floors of a query's first / last taps (x0, xl), (y0, yl) bound a window of at most
// span + 1 floors per axis (md 0, else 1), and then its origin and the corner columns / rows it
// spans, [x0, xl + 1]: nx, ny <= span + 2 (all zeros when it does not fit).  Every step of the chain
// (exact-or-rounded add of the offset, the normalize / unnormalize roundings by positive factors,
// floor) is monotone, so the floors are non-decreasing in the offset and the end taps bound the
// whole window; NaN / inf / huge coordinates do not fit (the forward gathers them directly, the
// backward walks them serially, and they fail every in-range test there).
struct WindowFit { int md, x0, y0, nx, ny; };
__device__ __forceinline__ WindowFit window_fit(float x0, float xl, float y0, float yl, int span) {
    bool ok = fabsf(x0) < 1.0e7f && fabsf(y0) < 1.0e7f;  // false for NaN / inf / huge
    const float dx = xl - x0, dy = yl - y0;   // exact: integers < 2^24
    ok &= (dx >= 0.0f) & (dx <= (float)span) & (dy >= 0.0f) & (dy <= (float)span);
    WindowFit f;
    f.md = ok ? 0 : 1;
    f.x0 = ok ? (int)x0 : 0;
    f.y0 = ok ? (int)y0 : 0;
    f.nx = ok ? (int)dx + 2 : 0;
    f.ny = ok ? (int)dy + 2 : 0;
    return f;
}

// grid_sample's zeros padding, tested in float: NaN, +-inf and huge floors are outside, exactly as
// ATen's int32-converted masks have them.  axis_in: one axis alone (the backward's separable passes);
// it is the two-axis test with a constant second axis, not the other way round, because the corner
// fetches' instruction streams depend on the association of the four compares.
__device__ __forceinline__ bool in_image(int h, int w, float fx, float fy) {
    return (fx >= 0.0f) & (fx < (float)w) & (fy >= 0.0f) & (fy < (float)h);
}
__device__ __forceinline__ bool axis_in(float f, int n) { return in_image(1, n, f, 0.0f); }

// Bilinear blend exactly as ATen's AVX512 grid_sampler (nw product, then FMA chain).
// w = x-frac, n = y-frac; out-of-image corners must already be 0.
__device__ __forceinline__ float blend(float vnw, float vne, float vsw, float vse, float w, float n) {
    const float e = __fsub_rn(1.0f, w);
    const float s = __fsub_rn(1.0f, n);
    float acc = __fmul_rn(vnw, __fmul_rn(s, e));
    acc = __builtin_fmaf(vne, __fmul_rn(s, w), acc);
    acc = __builtin_fmaf(vsw, __fmul_rn(n, e), acc);
    acc = __builtin_fmaf(vse, __fmul_rn(n, w), acc);
    return acc;
}

// Zeros-padding corner fetch by float coordinates (in_image).  Used by the generic / fallback paths only.
// ntx <= 0: row-major image (bilinear_sampler, compact levels); otherwise a tiled pyramid level.
__device__ __forceinline__ float corner(const float* __restrict__ img, int h, int w, float fx, float fy,
                                        int ntx = 0) {
    if (!in_image(h, w, fx, fy)) return 0.0f;
    const int y = (int)fy, x = (int)fx;
    return img[ntx <= 0 ? (int64_t)y * w + x : (int64_t)tiled_off(y, x, ntx)];
}

// The same corner fetch from pyramid level lv (base lvbase, any format) for query row R.
__device__ __forceinline__ float level_corner(const float* __restrict__ lvbase, int64_t R, int lv, int ntx, int h,
                                              int w, int64_t sz, float fx, float fy) {
    if (!in_image(h, w, fx, fy)) return 0.0f;
    return lvbase[pix_off(R, (int)fy, (int)fx, lv, ntx, w, sz)];
}

// One bilinear sample of img[h][w] at pixel coordinates (x, y) (model/utils.py:7-21).
__device__ __forceinline__ float sample_px(const float* __restrict__ img, int h, int w, float x, float y,
                                           int ntx = 0) {
    const float ix = unnormalize(x, (float)(w - 1), (float)(w - 1) * 0.5f);
    const float iy = unnormalize(y, (float)(h - 1), (float)(h - 1) * 0.5f);
    const float x0 = floorf(ix), y0 = floorf(iy);
    const float wx = __fsub_rn(ix, x0), wy = __fsub_rn(iy, y0);
    const float x1 = __fadd_rn(x0, 1.0f), y1 = __fadd_rn(y0, 1.0f);
    return blend(corner(img, h, w, x0, y0, ntx), corner(img, h, w, x1, y0, ntx),
                 corner(img, h, w, x0, y1, ntx), corner(img, h, w, x1, y1, ntx), wx, wy);
}

// sample_px on query row R of pyramid level lv (any format).
__device__ __forceinline__ float sample_level_px(const float* __restrict__ lvbase, int64_t R, int lv, int ntx, int h,
                                                 int w, int64_t sz, float x, float y) {
    const float ix = unnormalize(x, (float)(w - 1), (float)(w - 1) * 0.5f);
    const float iy = unnormalize(y, (float)(h - 1), (float)(h - 1) * 0.5f);
    const float x0 = floorf(ix), y0 = floorf(iy);
    const float wx = __fsub_rn(ix, x0), wy = __fsub_rn(iy, y0);
    const float x1 = __fadd_rn(x0, 1.0f), y1 = __fadd_rn(y0, 1.0f);
    return blend(level_corner(lvbase, R, lv, ntx, h, w, sz, x0, y0), level_corner(lvbase, R, lv, ntx, h, w, sz, x1, y0),
                 level_corner(lvbase, R, lv, ntx, h, w, sz, x0, y1), level_corner(lvbase, R, lv, ntx, h, w, sz, x1, y1),
                 wx, wy);
}

}  // namespace ecorr
