// build_tile.h -- what the CorrBlock build's GEMM kernels (build.hip and, for the hi-only split16
// kernels, build_hi.hip: the translation units that include this header) share because it is a property of the tile, not of one kernel: the n-tile
// geometry and tile order, the operand-panel order of the targets, the pooled-level addressing and
// descriptors, and the frame of the three 256 x 128 kernels (build_split_kernel,
// build_split16_kernel, build_f32_kernel): their one LDS array, the per-pixel exponents, the
// operand-panel descriptors, the accumulator pin, the epilogues' scale step and their stores.
#pragma once
#include "ecorr_device.h"
#include "ecorr_internal.h"
#include "split_f16.h"

namespace ecorr {

namespace {

constexpr int TBH = 8, TBW = 16;  // regular target block (rows x cols) of one n-tile
constexpr int PANEL = 8192;       // bytes of one (128-pixel tile, 16-deep K chunk) operand panel

__device__ __forceinline__ float pool4(float a, float b, float c, float d) {
    return __fmul_rn(__fadd_rn(__fadd_rn(__fadd_rn(a, b), c), d), 0.25f);
}

// pool4 as four VALU ops in the same order: left to itself hipcc pairs the split epilogue's pools
// into v_pk_add_f32 whose operands sit in different register pairs (two v_mov per packed add)
__device__ __forceinline__ float pool4_v(float a, float b, float c, float d) {
    float s;
    asm("v_add_f32 %0, %1, %2" : "=v"(s) : "v"(a), "v"(b));
    asm("v_add_f32 %0, %1, %2" : "=v"(s) : "v"(s), "v"(c));
    asm("v_add_f32 %0, %1, %2" : "=v"(s) : "v"(s), "v"(d));
    asm("v_mul_f32 %0, 0.25, %1" : "=v"(s) : "v"(s));
    return s;
}

// Bijective XCD-aware remap (cdna_hip_programming.md §5 T1): consecutive logical tiles land on
// one XCD so tiles sharing operand panels share that XCD's L2.  Speed only, never correctness.
__device__ __forceinline__ int xcd_remap(int bid, int nwg) {
    const int q = nwg / 8, r = nwg % 8, xcd = bid % 8, k = bid / 8;
    return (xcd < r ? xcd * (q + 1) : r * (q + 1) + (xcd - r) * q) + k;
}

// n-tiles: 8 x 16 target blocks (regular), or, in the last 4 rows when H % 8 is 1..4, 4 x 32
// blocks ("band"): those rows feed pyramid levels 0-2 only (level 3 of an H = 8k + r map, r <= 4,
// has k rows), so the band pools 4 x 8 sub-blocks and no 8-row tile row is padded half empty
// (DSEC H = 60: 6.7% of the matrix work saved).
struct NTile { int ty0, tx0, band; };
__device__ __forceinline__ NTile ntile_of(const BuildParams& P, int nt) {
    NTile n;
    if (nt < P.n_reg) {
        const int nty = nt / P.n_ntx;
        n.ty0 = nty * TBH;
        n.tx0 = (nt - nty * P.n_ntx) * TBW;
        n.band = 0;
    } else {
        n.ty0 = P.band_y0;
        n.tx0 = (nt - P.n_reg) * 32;
        n.band = 1;
    }
    return n;
}

// Grouped tile order: GM m-tiles x all n-tiles per group, so consecutive tiles share panels.  BAL:
// the item's m-tiles split into ceil(n_m / GM) groups of (nearly) equal size instead of full groups
// and a remainder -- at DSEC (19 split16 query tiles) GM 10 makes two groups (10, 9), so every
// target panel leaves the L2 twice per item instead of three times (8, 8, 3): FETCH -20%, the build
// 1.3% shorter (profiles/r05_lab/gm_clock_l2_b.txt); 10 query panels (2.5 MB) + the resident
// blocks' target panels still fit an XCD's 4-MB L2 (GM 16 does not: 4.5 MB, slower).
template <int GM, bool BAL>
__device__ __forceinline__ void decode_tile(const BuildParams& P, int t, int n_m, int& b, int& mt, int& nt) {
    const int per_b = n_m * P.n_nt;
    b = t / per_b;
    const int i = t - b * per_b;
    const int ng = (n_m + GM - 1) / GM;
    const int gm = BAL ? (n_m + ng - 1) / ng : GM;
    const int gsz = gm * P.n_nt;
    const int grp = i / gsz, gi = i - grp * gsz;
    const int first_m = grp * gm;
    const int gsm = min(n_m - first_m, gm);
    mt = first_m + gi % gsm;
    nt = gi / gsm;
}

// The tile of this block in that order (XCD-remapped): batch item b, m-tile mt of the item's n_m,
// n-tile nt; returns nt's target block.
template <int GM, bool BAL>
__device__ __forceinline__ NTile block_tile(const BuildParams& P, int n_m, int& b, int& mt, int& nt) {
    decode_tile<GM, BAL>(P, xcd_remap(blockIdx.x, gridDim.x), n_m, b, mt, nt);
    return ntile_of(P, nt);
}

// One pooled-level pixel (row, col) of a query image: tiled (ntx > 0; the tile must exist, cells
// in a tile's padding are written and never read), interleaved (ntx < 0; likewise the block) or
// compact row-major (range-checked).
__device__ __forceinline__ float* level_px(const BuildParams& P, int L, int64_t row_img, int r, int c) {
    if (P.lntx[L] < 0) {   // interleaved: the block must exist
        if (!ilv_cell_in(r, c, L, P.lnty[L], -P.lntx[L])) return nullptr;
        return P.lvl[L] + pix_off(row_img, r, c, L, P.lntx[L], P.lw[L], P.lsz[L]);
    }
    float* img = P.lvl[L] + row_img * P.lsz[L];
    if (P.lntx[L] > 0) {
        if ((r >> 2) >= P.lnty[L] || (c >> 3) >= P.lntx[L]) return nullptr;
        return img + tiled_off(r, c, P.lntx[L]);
    }
    if (r >= P.lh[L] || c >= P.lw[L]) return nullptr;
    return img + (int64_t)r * P.lw[L] + c;
}

// Buffer descriptor over the slab of fused level lv that holds the query images [rows0, rows0 + nq)
// (ecorr_device.h slab_first / slab_bytes): its range check is the query bound.  lv >= 1: the fused
// levels that are interleaved.
__device__ __forceinline__ __amdgpu_buffer_rsrc_t level_rsrc(const BuildParams& P, int lv, int64_t rows0, int nq) {
    if (lv >= 1)
        return __builtin_amdgcn_make_buffer_rsrc(P.lvl[lv] + slab_first(true, rows0, P.lsz[lv]), 0,
                                                 (int)slab_bytes(true, rows0, nq, P.lsz[lv]), 0x00020000);
    return __builtin_amdgcn_make_buffer_rsrc(P.lvl[lv] + slab_first(false, rows0, P.lsz[lv]), 0,
                                             (int)slab_bytes(false, rows0, nq, P.lsz[lv]), 0x00020000);
}

// ============================================================================================
// The 256 x 128 kernels: 256 queries x one 128-target n-tile per block, 4 waves of 64 queries x
// all 128 targets, two blocks per CU, a per-wave register epilogue.
// ============================================================================================
constexpr int SQ = 256;                     // queries per split tile
constexpr int SLDS = 4 * 4 * 32 * 144;      // LDS bytes: the epilogue's transpose regions (> the K loop's)
constexpr int SOOB = 0x7ffffff0;            // buffer offset beyond any panel or operand: loads (and lands in
                                            // LDS as) 0, touches nothing
constexpr int ST_L01 = 2;                   // level-0/1 store cache policy: nt (A/B: 725 vs 731 us for nt sc1;
                                            // plain and sc1 alone ~1000 us: the lines stay in L2 and evict the panels;
                                            // split16, round 3: nt 605 vs nt sc1 627 us)

// ALL the LDS of such a kernel is ONE array, char smem[TILE_LDS]: a second __shared__ object can
// make hipcc wait vmcnt(0) before every ds_read while a buffer_load ... lds is in flight
// (cdna_hip_programming.md trap 4(a)).  SLDS bytes of K-loop buffers, which the epilogue reuses as
// its transpose scratch, then the exponents the epilogue scales by:
constexpr int TILE_LDS = SLDS + (SQ + 256) * 4;
__device__ __forceinline__ int* tile_exq(char* smem) { return reinterpret_cast<int*>(smem + SLDS); }     // exponents of the 256 queries
__device__ __forceinline__ int* tile_ext(char* smem) { return tile_exq(smem) + SQ; }                     // ... negated, of the 128 panel targets
__device__ __forceinline__ float* tile_fst(char* smem) { return reinterpret_cast<float*>(tile_ext(smem) + 128); }   // 2^ext when |ext| <= 63

// target (y, x) of position p of a split fmap2 panel, relative to the n-tile origin
__host__ __device__ __forceinline__ void split_target(int p, bool band, int& y, int& x) {
    if (!band) {
        y = 4 * ((p >> 5) & 1) + ((p >> 3) & 3);
        x = 8 * (p >> 6) + (p & 7);
    } else {
        y = (p >> 3) & 3;
        x = 8 * (p >> 5) + (p & 7);
    }
}

// target (y, x) of position p of a split16 fmap2 panel, relative to the n-tile origin: p = 16 tg +
// 4 kb + i lies in quadrant kb (regular: rows 4 (kb & 1) .., cols 8 (kb >> 1) ..; band: cols 8 kb ..)
// at quadrant row tg >> 1, column 4 (tg & 1) + i
__host__ __device__ __forceinline__ void split16_target(int p, bool band, int& y, int& x) {
    const int tg = p >> 4, kb = (p >> 2) & 3, i = p & 3;
    if (!band) {
        y = 4 * (kb & 1) + (tg >> 1);
        x = 8 * (kb >> 1) + 4 * (tg & 1) + i;
    } else {
        y = tg >> 1;
        x = 8 * kb + 4 * (tg & 1) + i;
    }
}

// Per-pixel exponents of thread tid's query (eq) and, tid < 128, of position tid of the target
// panel in TARGET order (et; negated when published): only the epilogue reads them, so they load
// behind the K loop's last static wait and reach LDS after it (in the prologue, their two dependent
// global loads with vmcnt(0) waits delayed every block's first DMA)
template <void (*TARGET)(int, bool, int&, int&)>
__device__ __forceinline__ void load_exponents(const BuildParams& P, const NTile& tc, int b, int q0, int tid, int& eq,
                                               int& et) {
    eq = q0 + tid < P.q_count ? P.ex1[(int64_t)b * P.q_count + q0 + tid] : 0;
    if (tid < 128) {
        int y, x;
        TARGET(tid, tc.band, y, x);
        y += tc.ty0;
        x += tc.tx0;
        et = (y < P.H && x < P.W) ? P.ex2[b * ((int64_t)P.H * P.W) + (int64_t)y * P.W + x] : 0;
    }
}

// ... and into the block's LDS for the epilogue (the caller's barrier publishes them); zero
// exponents (the fp32 kernel: no operand scaling) make the scale 1 / sqrt(D) alone
__device__ __forceinline__ void publish_exponents(char* smem, int tid, int eq, int et) {
    tile_exq(smem)[tid] = eq;
    if (tid < 128) {
        tile_ext(smem)[tid] = -et;
        tile_fst(smem)[tid] = exp2i(max(-63, min(-et, 63)));
    }
}

// Operand-panel descriptors of split tile (b, qt, nt), pstride = bytes of one 128-pixel tile's
// panels: rq over the two query panels (adjacent tiles of pk1), rt over the one target panel
__device__ __forceinline__ void panel_rsrc(const BuildParams& P, int64_t pstride, int b, int qt, int nt,
                                           __amdgpu_buffer_rsrc_t& rq, __amdgpu_buffer_rsrc_t& rt) {
    const int qp = 2 * qt;
    const int nqp = min(2, P.n_mt - qp);
    rq = __builtin_amdgcn_make_buffer_rsrc(const_cast<char*>(P.pk1 + ((int64_t)b * P.n_mt + qp) * pstride), 0,
                                           (int)(nqp * pstride), 0x00020000);
    rt = __builtin_amdgcn_make_buffer_rsrc(const_cast<char*>(P.pk2 + ((int64_t)b * P.n_nt + nt) * pstride), 0,
                                           (int)pstride, 0x00020000);
}

// Pin the accumulators to one register class, AGPR: "a" or VGPR: "v" (before the K loop, and
// again before the epilogue).  Left to its heuristics hipcc keeps floatx16 accumulators in VGPRs
// with MFMA destinations apart from their sources and spills ~100 registers at 2 waves per SIMD.
template <bool AGPR, typename T, int NI, int NJ>
__device__ __forceinline__ void pin_acc(T (&acc)[NI][NJ]) {
#pragma unroll
    for (int i = 0; i < NI; ++i)
#pragma unroll
        for (int j = 0; j < NJ; ++j) {
            if constexpr (AGPR) asm volatile("" : "+a"(acc[i][j]));
            else asm volatile("" : "+v"(acc[i][j]));
        }
}
template <bool AGPR, typename T, int NI, int NJ>
__device__ __forceinline__ void zero_acc(T (&acc)[NI][NJ]) {
#pragma unroll
    for (int i = 0; i < NI; ++i)
#pragma unroll
        for (int j = 0; j < NJ; ++j) acc[i][j] = T{};
    pin_acc<AGPR>(acc);
}

// ---- the epilogues' scale step: x = acc 2^(nqe + ext) (/ sqrt(D) when that is no power of two),
// nqe = query_exp of the lane's query, ext the target's negated exponent.  Where every exponent of
// the wave's queries and of the panel's targets lies in [-63, 63] (fast_scale), the 2^nqe 2^ext
// product is a normal power of two and one multiply by it rounds exactly as ldexpf does: two
// packed multiplies per element pair instead of an add, a negate and an ldexp per element.
template <bool MUL>
__device__ __forceinline__ int query_exp(const BuildParams& P, const int* exq, int q) {
    return -(exq[q] + (MUL ? P.scale_shift : 0));
}
// wave-uniform; qw = the first of the wave's 64 block-local queries
template <bool MUL>
__device__ __forceinline__ bool fast_scale(const BuildParams& P, const int* exq, const int* ext, int qw, int lane) {
    const int n = query_exp<MUL>(P, exq, qw + lane);
    return __all(ext[lane] >= -63 && ext[lane] <= 63 && ext[lane + 64] >= -63 && ext[lane + 64] <= 63 && n >= -63 &&
                 n <= 63);
}
// four accumulators of one query on four consecutive panel targets (fst4 / ext4 = their entries of
// tile_fst / tile_ext), fast: sq = 2^nqe; exact power-of-two products, as v_pk_mul_f32 pairs (the
// library is built without SLP vectorization, which packed the pooling adds at two v_mov each;
// packing is spelled out where it pays)
template <bool MUL>
__device__ __forceinline__ void scale4_fast(const BuildParams& P, floatx4 a, float sq, const float* fst4, float (&v)[4]) {
    const floatx4 s4 = *reinterpret_cast<const floatx4*>(fst4);
    const floatx2 sq2 = {sq, sq};
#pragma unroll
    for (int h = 0; h < 2; ++h) {
        const floatx2 x = floatx2{a[2 * h], a[2 * h + 1]} * (sq2 * floatx2{s4[2 * h], s4[2 * h + 1]});
        v[2 * h] = MUL ? x[0] : __fdiv_rn(x[0], P.scale);
        v[2 * h + 1] = MUL ? x[1] : __fdiv_rn(x[1], P.scale);
    }
}
// ... and outside the window
template <bool MUL>
__device__ __forceinline__ void scale4_ldexp(const BuildParams& P, floatx4 a, int nqe, const int* ext4, float (&v)[4]) {
    const int4 e4 = *reinterpret_cast<const int4*>(ext4);
    const int e[4] = {e4.x, e4.y, e4.z, e4.w};
#pragma unroll
    for (int t = 0; t < 4; ++t) {
        const float x = ldexpf(a[t], nqe + e[t]);
        v[t] = MUL ? x : __fdiv_rn(x, P.scale);
    }
}

// The descriptors of a block's query images [rows0, rows0 + nq) over the four fused levels
// (level_rsrc; a level the build does not fuse aliases level 0 and is not stored to)
__device__ __forceinline__ void block_levels(const BuildParams& P, int64_t rows0, int nq, __amdgpu_buffer_rsrc_t (&r)[4]) {
    const int L = P.fused_levels;
    r[0] = level_rsrc(P, 0, rows0, nq);
    r[1] = level_rsrc(P, L > 1 ? 1 : 0, rows0, nq);
    r[2] = level_rsrc(P, L > 2 ? 2 : 0, rows0, nq);
    r[3] = level_rsrc(P, L > 3 ? 3 : 0, rows0, nq);
}

// One 16- / 8-byte piece of a pyramid level at byte voff + uoff of descriptor rs, non-temporal
// (ST_L01); a voff of SOOB (or beyond the slab) drops the piece.  uoff is for a wave-uniform term:
// it is added into the voffset and the soffset stays 0 -- with the term in an SGPR soffset hipcc
// omits the wait state a 16-byte store needs before a VALU overwrites its data VGPRs (LLVM assumes
// that hazard only without an soffset register), and such a store wrote the next VALU's value
// (round 3's "lost" rows; round 5, tools/soff_repro.py; guarded by tests/test_isa_store_hazard.py).
__device__ __forceinline__ void store_piece(__amdgpu_buffer_rsrc_t rs, int voff, int uoff, floatx4 v) {
    __builtin_amdgcn_raw_buffer_store_b128(__builtin_bit_cast(uint4v, v), rs, voff + uoff, 0, ST_L01);
}
__device__ __forceinline__ void store_piece(__amdgpu_buffer_rsrc_t rs, int voff, int uoff, floatx2 v) {
    __builtin_amdgcn_raw_buffer_store_b64(__builtin_bit_cast(uint2v, v), rs, voff + uoff, 0, ST_L01);
}
// ... at byte off, dropped unless ok (off is computed either way: a select, not a branch)
template <typename V>
__device__ __forceinline__ void store_piece_if(__amdgpu_buffer_rsrc_t rs, bool ok, int off, V v) {
    store_piece(rs, ok ? off : SOOB, 0, v);
}

}  // namespace

}  // namespace ecorr
