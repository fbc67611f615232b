// build.hip -- CorrBlock build on gfx950: the all-pairs correlation GEMM with the 1/sqrt(D) scale
// and the 3 pooled pyramid levels fused into its epilogue.
//
// Replaces corr.py:13-27 (CorrBlock.__init__) and corr.py:52-60 (CorrBlock.corr):
//   level0[b*q_count + p][y][x] = (sum_d f1[b][d][p] * f2[b][d][y*W+x]) / sqrt(D)
//   level{i+1} = (((x00 + x01) + x10) + x11) / 4 over 2x2 floor-mode windows of level i,
// stored in the tiled pyramid layout of include/ecorr.h (4 x 8-float tiles per query image).
//
// Two build modes, one result contract (include/ecorr.h), four GEMM kernels (launch_build):
//   split (ecorr_build_split, default): pack_both_kernel splits every fp32 operand into
//     per-pixel-scaled f16 hi + lo halves, written as operand panels in MFMA-fragment order; the
//     GEMM sums lo*hi + hi*lo + hi*hi per product:
//       build_split16_kernel  16 K chunks (D = 241 .. 256: the E-RAFT feature width), on
//                             v_mfma_f32_16x16x32_f16 with its own panel layout;
//       build_split_kernel    every other D, on v_mfma_f32_32x32x16_f16, a rolled K loop.
//     (ecorr_build_split_*_hi, build_hi.hip: build_split16_kernel on hi*hi alone while every lo
//     half is +-0, as for finite 16-bit fmaps -- the same pyramid bit for bit.)
//   fp32 (ecorr_build): v_mfma_f32_32x32x2_f32, an exact k-ordered fmaf chain:
//       build_f32_kernel      D = 256 with W a multiple of 4, fmap2 16-byte aligned and 31-bit
//                             operand offsets: 256 x 128 block tile;
//       build_kernel          everything else: 128 x 128 block tile (16-byte loads and LDS-DMA
//                             staging where alignment and the offsets allow).
// Pooling is bit-exact given the same level 0 in both; per-element accumulation order does not
// depend on the tiling, so query-slab (row-sharded) builds are bitwise the whole build's rows.
//
// What is a property of the tile and not of one kernel -- tile geometry and order, level addressing,
// the 256 x 128 kernels' LDS array, exponents, panel descriptors, scale step and stores -- is in
// build_tile.h; what the split16 kernels of this file and of build_hi.hip (the hi-only GEMM,
// ecorr_build_split_gemm_hi) share beyond that is in build_split16.h and build_split16_loop.h.
//
// There are no runtime knobs: every variant that lost an A/B is gone from the source (DESIGN.md
// §3.1 keeps the record); lab builds for new A/Bs are separate .so files (tools/).
#include "build_split16.h"
#include "build_tile.h"
#include "out_elem.h"
#include "split_f16.h"

#include <type_traits>

namespace ecorr {

namespace {

// ============================================================================================
// Split GEMM (default).  Block tile: 256 queries (two 128-query fmap1 panels) x one 128-target
// n-tile (one fmap2 panel); 4 waves, wave w = queries 64 w .. 64 w + 63 x all 128 targets = 2 x 4
// v_mfma_f32_32x32x16_f16 tiles (128 accumulators, pinned to AGPRs).  Two blocks per CU.
//
// The MFMAs take the fmap2 fragment as their A operand: the accumulators hold C^T, lane (acol,
// arow) of tile (i, j) owns query 32 i + acol and targets 32 j + 8 g4 + 4 arow + t (reg 4 g4 + t).
// The fmap2 panel stores the n-tile's targets (split_target) so that target group j of a regular
// 8 x 16 tile is one pyramid tile line: rows 4 (j & 1) + g4, cols 8 (j >> 1) + 4 arow + t -- each
// lane holds 4 x 4 pixels of every line of its query, the 2 x 2 and 4 x 4 pools are in-lane and
// the 8 x 8 pool needs one value from lane acol + 32.  Band tiles (4 x 32): rows g4, cols 8 j +
// 4 arow + t.
//
// K loop: the target panel (shared by the 4 waves) goes global -> LDS verbatim by LDS-DMA
// (buffer_load_dwordx4 ... lds, 2 per wave and chunk) through 3 buffers, two chunks ahead; the
// query fragments (wave-private) go global -> VGPR, two chunks ahead.  One barrier per chunk;
// target fragments are lane-linear ds_read_b128 (conflict-free).  Chunk kc + 1's barrier and
// first fragments are read between chunk kc's lo*hi MFMAs and its hi*lo / hi*hi MFMAs.  Chunks
// past the end are issued as out-of-range loads (they land as zeros), which keeps every wait
// count static.
//
// Epilogue, per wave from its accumulators: scale by 2^-(e_q + e_t) / sqrt(D), pool 8x8 -> 4x4 ->
// 2x2 -> 1 in registers in the reference's order, then store.  Store shape matters more than
// anything else here (tools/store_lab.hip, DSEC level-0 shape): whole 128-byte lines run at
// 5.2-5.5 TB/s with any cache policy; 32-byte pieces only as plain stores, which keep every line
// in L2 and evict the operand panels (PMC: 1 GB of panel re-reads per build).  So level-0 and
// level-1 lines pass through a wave-private LDS transpose and leave whole as non-temporal stores
// (out of L2); levels 2-3 (6% of the bytes) leave as 16- / 8-byte row pieces.
// ============================================================================================
constexpr int SCHUNK = PANEL;               // LDS bytes per K chunk (the target panel)
constexpr int SNBUF = 4;                    // LDS buffers of the target panel's chunk ring
constexpr int SCOPIES = SCHUNK / 1024 / 4;  // LDS-DMA copies per wave per chunk (2)
constexpr int QLOADS = 4;                   // query fragment loads per wave per chunk (hi, lo x 2 rows)
constexpr int XS = 144;                     // LDS bytes per query of the epilogue's line transpose
static_assert(4 * 4 * 32 * XS <= SLDS && SNBUF * SCHUNK <= SLDS, "LDS regions");

// lanes 32-63 of a <-> lanes 0-31 of b (v_permlane32_swap)
__device__ __forceinline__ void swap32(float& a, float& b) {
    const auto r = __builtin_amdgcn_permlane32_swap(__float_as_uint(a), __float_as_uint(b), false, false);
    a = __uint_as_float(r[0]);
    b = __uint_as_float(r[1]);
}

// Epilogue of the split build for one wave: its 64 queries (block-local qw .. qw + 63) x the
// n-tile tc, from its accumulators (C^T fragments, build_split_kernel); xw = the wave's four
// LDS transpose regions (4 x 32 x XS bytes); smem = the block's LDS array with the published
// exponents (build_tile.h).
template <bool MUL>
__device__ __forceinline__ void split_epilogue(const BuildParams& P, floatx16 (&acc)[2][4], char* smem, char* const xw,
                                               int qw, const NTile& tc, int b, int q0, int lane) {
    const int *exq = tile_exq(smem), *ext = tile_ext(smem);
    const float* fst = tile_fst(smem);
    const int acol = lane & 31, arow = lane >> 5;
    // Line segments through a wave-private LDS transpose (no barrier: a wave's LDS accesses are
    // processed in order): the lane writes its 16-byte pieces into the line image of its query
    // (32 queries x 144 B: conflict-free ds_write_b128 and ds_read_b128), then reads back piece m
    // of segment arow of query 4k + s, so the 4 lanes of a quad store 64 contiguous bytes and
    // lanes acol, acol + 32 the two halves of one line.
    // four regions per wave (one per level-0 line of a tile row; the level-1 line reuses region
    // 0): no line waits for the previous line's read-back before writing
    const int m4 = lane & 3, k4 = acol >> 2;
    const int wo = acol * XS, ro = (4 * k4) * XS + 64 * arow + 16 * m4;
    const int L = P.fused_levels;
    // per-level descriptors over the block's query images (level_rsrc); interleaved levels: over
    // the 64-row groups the block's rows touch, from group g0
    const int64_t rows0 = (int64_t)b * P.q_count + q0;   // the block's first query image
    const int nq = min(SQ, P.q_count - q0);
    __amdgpu_buffer_rsrc_t rl[4];
    block_levels(P, rows0, nq, rl);
    const int64_t g0 = slab_g0(rows0);
    // read the transposed segments back and store them: line byte offset lo (+ the query image)
    auto store_lines = [&](const char* xp, __amdgpu_buffer_rsrc_t rs, int64_t lsz, int ql, int lo, bool ok) {
        floatx4 pc[4];
#pragma unroll
        for (int s = 0; s < 4; ++s) pc[s] = *reinterpret_cast<const floatx4*>(xp + ro + s * XS);
        const int base = (int)((ql + 4 * k4) * lsz * 4) + lo + 16 * m4;
#pragma unroll
        for (int s = 0; s < 4; ++s) store_piece_if(rs, ok, base + (int)(s * lsz * 4), pc[s]);
    };
    // One block row (r, c .. c + N - 1), N = the block width, of level 2 or 3 (interleaved) for
    // block-local query qloc: lanes on consecutive queries write consecutive 4N-byte pieces, so a
    // store instruction covers whole lines, which leave non-temporally like levels 0-1 (A/B: 656
    // vs 685 us with plain stores, which park the lines in L2).  Queries past the block and
    // blocks outside the level are dropped (padding cells of a block are written, never read).
    auto store_px = [&](__amdgpu_buffer_rsrc_t rs, int lv, int qloc, int r, int c, auto val) {
        const bool in = qloc < nq && ilv_cell_in(r, c, lv, P.lnty[lv], -P.lntx[lv]);
        // row term + cell term, each in 32 bits (summed in 64 bits the epilogue grows by ~200 instructions)
        const int off = ((int)ilv_row_off(rows0 + qloc, g0, lv, P.lsz[lv]) + (int)ilv_cell_off(r, c, lv, -P.lntx[lv])) * 4;
        store_piece_if(rs, in, off, val);
    };
    const bool fast = fast_scale<MUL>(P, exq, ext, qw, lane);   // the scale step: build_tile.h
    // the lane's four targets of a group: one base register, the group in the ds_read's immediate
    const int* const extl = ext + 4 * arow;
    const float* const fstl = fst + 4 * arow;
#pragma unroll
    for (int i = 0; i < 2; ++i) {
        const int ql = qw + 32 * i;          // first block-local query of this tile row
        const int nqe = query_exp<MUL>(P, exq, ql + acol);
        // level-1 values of the lane's query: [block bb][row][col pair] (band: [half][2 y1 + jl]);
        // level 2: [bb][row r] (band: [bb][jl]); level 3: [bb]
        float l1[2][4][2], l2[2][2], l3[2];
#pragma unroll
        for (int bb = 0; bb < 2; ++bb) {
            // scaled values of lines j = 2 bb + jl, [jl][g4][t]; target exponents
            // ext[32 j + 8 g4 + 4 arow + t]
            float v[2][4][4];
            // one uniform branch around the eight groups of four, as in split16_epilogue
            auto acc4 = [&](int j, int g4) {
                return floatx4{acc[i][j][4 * g4], acc[i][j][4 * g4 + 1], acc[i][j][4 * g4 + 2], acc[i][j][4 * g4 + 3]};
            };
            if (fast) {
                const float sq = exp2i(nqe);
#pragma unroll
                for (int k = 0; k < 8; ++k) {   // k = 4 jl + g4
                    const int j = 2 * bb + (k >> 2), g4 = k & 3;
                    scale4_fast<MUL>(P, acc4(j, g4), sq, fstl + 32 * j + 8 * g4, v[k >> 2][g4]);
                }
            } else {
#pragma unroll
                for (int k = 0; k < 8; ++k) {
                    const int j = 2 * bb + (k >> 2), g4 = k & 3;
                    scale4_ldexp<MUL>(P, acc4(j, g4), nqe, extl + 32 * j + 8 * g4, v[k >> 2][g4]);
                }
            }
            // level 0: line j = rows g4 x this lane's 4 columns
#pragma unroll
            for (int jl = 0; jl < 2; ++jl) {
                const int j = 2 * bb + jl;
                char* const xp = xw + j * (32 * XS);
#pragma unroll
                for (int g4 = 0; g4 < 4; ++g4)
                    *reinterpret_cast<floatx4*>(xp + wo + 32 * g4 + 16 * arow) =
                        floatx4{v[jl][g4][0], v[jl][g4][1], v[jl][g4][2], v[jl][g4][3]};
                const int tr = (tc.ty0 >> 2) + (tc.band ? 0 : (j & 1));
                const int tcl = (tc.tx0 >> 3) + (tc.band ? j : (j >> 1));
                store_lines(xp, rl[0], P.lsz[0], ql, tile_base(tr, tcl, P.lntx[0]) * 4 + 64 * arow,
                            tr < P.lnty[0] && tcl < P.lntx[0]);
            }
            if (L < 2) continue;
            if (!tc.band) {
                // regular: line j = rows 4 jl + g4 of 8 x 8 block bb; level 1 rows y1 = 0..3, cols
                // 4 bb + 2 arow + c; level 2 rows r, col 2 bb + arow; level 3 needs lane acol + 32
#pragma unroll
                for (int y1 = 0; y1 < 4; ++y1)
#pragma unroll
                    for (int c = 0; c < 2; ++c) {
                        const int jl = y1 >> 1, g = 2 * (y1 & 1);
                        l1[bb][y1][c] = pool4_v(v[jl][g][2 * c], v[jl][g][2 * c + 1], v[jl][g + 1][2 * c],
                                              v[jl][g + 1][2 * c + 1]);
                    }
                if (L >= 3) {   // level 2: rows r, col 2 bb + arow (stored per i below)
#pragma unroll
                    for (int r = 0; r < 2; ++r)
                        l2[bb][r] = pool4_v(l1[bb][2 * r][0], l1[bb][2 * r][1], l1[bb][2 * r + 1][0], l1[bb][2 * r + 1][1]);
                    // level 3, the 8 x 8 pool: lane acol + 32 holds the right column
                    const float o0 = __shfl_xor(l2[bb][0], 32), o1 = __shfl_xor(l2[bb][1], 32);
                    l3[bb] = pool4_v(l2[bb][0], o0, l2[bb][1], o1);
                }
            } else {
                // band: line j = row g4 x cols 8 j + 4 arow + t; level 1 rows y1 = 0..1, cols
                // 4 j + 2 arow + c (l1[bb][2 y1 + jl][c]); level 2 col 2 j + arow
#pragma unroll
                for (int jl = 0; jl < 2; ++jl)
#pragma unroll
                    for (int y1 = 0; y1 < 2; ++y1)
#pragma unroll
                        for (int c = 0; c < 2; ++c)
                            l1[bb][2 * y1 + jl][c] = pool4_v(v[jl][2 * y1][2 * c], v[jl][2 * y1][2 * c + 1],
                                                           v[jl][2 * y1 + 1][2 * c], v[jl][2 * y1 + 1][2 * c + 1]);
                if (L >= 3) {   // level 2: col 2 (2 bb + jl) + arow (stored per i below)
#pragma unroll
                    for (int jl = 0; jl < 2; ++jl)
                        l2[bb][jl] = pool4_v(l1[bb][jl][0], l1[bb][jl][1], l1[bb][2 + jl][0], l1[bb][2 + jl][1]);
                }
            }
        }
        if (L < 2) continue;
        if (L >= 3) {
            // level 2: one 16-byte row piece per lane.  Regular: the n-tile's 2 x 4 pixels, lane
            // acol row 0, lane acol + 32 row 1, cols {2 bb, 2 bb + 1} = (l2[bb][0] | l2[bb][1]) after
            // swapping row 1 of the arow-0 lanes with row 0 of the arow-1 lanes.  Band: the 1 x 8
            // pixels, lane acol cols 0-3, lane acol + 32 cols 4-7 (swap bb = 1 of the arow-0 lanes
            // with bb = 0 of the arow-1 lanes)
#pragma unroll
            for (int k = 0; k < 2; ++k) {
                if (!tc.band) swap32(l2[k][0], l2[k][1]);
                else swap32(l2[0][k], l2[1][k]);
            }
            const floatx4 row2 = tc.band ? floatx4{l2[0][0], l2[1][0], l2[0][1], l2[1][1]}
                                         : floatx4{l2[0][0], l2[0][1], l2[1][0], l2[1][1]};
            store_px(rl[2], 2, ql + acol, (tc.ty0 >> 2) + (tc.band ? 0 : arow), (tc.tx0 >> 2) + (tc.band ? 4 * arow : 0), row2);
            if (L >= 4 && !tc.band)   // level 3: the n-tile's 1 x 2 pixels, from the arow-0 lanes
                store_px(rl[3], 3, arow ? nq : ql + acol, tc.ty0 >> 3, tc.tx0 >> 3, floatx2{l3[0], l3[1]});
        }
        // level 1 (interleaved 2 x 4 blocks): the lane holds cols 2 arow, 2 arow + 1 of each block
        // row; one swap of rows between the arow halves leaves lane acol with row 0 and lane
        // acol + 32 with row 1 of the block, each a 16-byte piece (as level 2).  Regular: blocks
        // (r, bb) = level-1 rows ty0/2 + 2r .. +1, cols tx0/2 + 4 bb .. +3 (l1[bb][y1][c], y1 = 2r,
        // 2r + 1); band: blocks j = 2 bb + jl = rows ty0/2 .. +1, cols tx0/2 + 4j .. +3
        // (l1[bb][2 y1 + jl][c])
#pragma unroll
        for (int bb = 0; bb < 2; ++bb)
#pragma unroll
            for (int r = 0; r < 2; ++r) {
                float x0, x1, y0, y1;
                if (!tc.band) {
                    x0 = l1[bb][2 * r][0], x1 = l1[bb][2 * r][1], y0 = l1[bb][2 * r + 1][0], y1 = l1[bb][2 * r + 1][1];
                } else {
                    x0 = l1[bb][r][0], x1 = l1[bb][r][1], y0 = l1[bb][2 + r][0], y1 = l1[bb][2 + r][1];
                }
                swap32(x0, y0);
                swap32(x1, y1);
                const int yb = (tc.ty0 >> 1) + (tc.band ? 0 : 2 * r) + arow;
                const int xb = (tc.tx0 >> 1) + (tc.band ? 4 * (2 * bb + r) : 4 * bb);
                store_px(rl[1], 1, ql + acol, yb, xb, floatx4{x0, x1, y0, y1});
            }
    }
}

template <bool MUL>
__global__ __launch_bounds__(256, 2) void build_split_kernel(BuildParams P) {
    __shared__ __attribute__((aligned(16))) char smem[TILE_LDS];   // ALL its LDS (build_tile.h)

    const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
    int b, qt, nt;
    const NTile tc = block_tile<8, false>(P, P.n_qt, b, qt, nt);
    const int q0 = qt * SQ;

    // ---- operand panels of this tile: two query panels (adjacent tiles of pk1), one target panel
    const int nk = (P.D + 15) / 16;   // K chunks
    const int64_t pstride = (int64_t)nk * PANEL;   // bytes of one 128-pixel tile's panels
    __amdgpu_buffer_rsrc_t rq, rt;
    panel_rsrc(P, pstride, b, qt, nt, rq, rt);
    // target panel: copy s of this wave = 1-KB piece wave + 4 s of the chunk (lane-linear, as
    // LDS-DMA requires)
    auto issue = [&](int kc) {
        char* dst = smem + (kc % SNBUF) * SCHUNK;
        const bool in = kc < nk;
#pragma unroll
        for (int s = 0; s < SCOPIES; ++s) {
            const int c = wave + 4 * s;
            __builtin_amdgcn_raw_ptr_buffer_load_lds(rt, (__attribute__((address_space(3))) void*)(dst + c * 1024), 16,
                                                     in ? kc * PANEL + c * 1024 + lane * 16 : SOOB, 0, 0, 0);
        }
    };

    floatx16 acc[2][4];
    zero_acc<true>(acc);   // pinned to AGPRs

    // query fragments: wave-private (rows 64 wave .. + 63), so they go global -> VGPR directly,
    // one chunk ahead: query panel wave/2, 32-row group 2 (wave&1) + i, [hi | lo] 1 KB each
    struct QFrags { halfx8 qh[2], ql[2]; };
    const int qgo = (wave >> 1) * (int)pstride + (wave & 1) * 4096 + lane * 16;
    auto load_q = [&](int kc, QFrags& q) {
        const bool in = kc < nk;
#pragma unroll
        for (int i = 0; i < 2; ++i) {
            q.qh[i] = __builtin_bit_cast(halfx8, __builtin_amdgcn_raw_buffer_load_b128(
                                                     rq, in ? qgo + kc * PANEL + i * 2048 : SOOB, 0, 0));
            q.ql[i] = __builtin_bit_cast(halfx8, __builtin_amdgcn_raw_buffer_load_b128(
                                                     rq, in ? qgo + kc * PANEL + i * 2048 + 1024 : SOOB, 0, 0));
        }
    };
    // target fragments of one chunk from LDS: group j, [hi k0-15 | lo k0-15] x 32 rows, 16 B per lane
    const int tfo = lane * 16;
    struct TFrags { halfx8 th[4], tl[4]; };
    auto read_lo = [&](int kc, TFrags& f) {   // what the lo*hi MFMAs need besides ql: th
        const char* cb = smem + (kc % SNBUF) * SCHUNK;
#pragma unroll
        for (int j = 0; j < 4; ++j) f.th[j] = *reinterpret_cast<const halfx8*>(cb + tfo + j * 2048);
    };
    auto read_hi = [&](int kc, TFrags& f) {   // tl
        const char* cb = smem + (kc % SNBUF) * SCHUNK;
#pragma unroll
        for (int j = 0; j < 4; ++j) f.tl[j] = *reinterpret_cast<const halfx8*>(cb + tfo + j * 2048 + 1024);
    };
    // per element: lo*hi, then hi*lo, then hi*hi (the accumulation order of the round-1 build)
    auto mfma_lohi = [&](const TFrags& f, const QFrags& q) {
#pragma unroll
        for (int i = 0; i < 2; ++i)
#pragma unroll
            for (int j = 0; j < 4; ++j)
                acc[i][j] = __builtin_amdgcn_mfma_f32_32x32x16_f16(f.th[j], q.ql[i], acc[i][j], 0, 0, 0);
    };
    auto mfma_rest = [&](const TFrags& f, const QFrags& q) {
#pragma unroll
        for (int i = 0; i < 2; ++i)
#pragma unroll
            for (int j = 0; j < 4; ++j)
                acc[i][j] = __builtin_amdgcn_mfma_f32_32x32x16_f16(f.tl[j], q.qh[i], acc[i][j], 0, 0, 0);
#pragma unroll
        for (int i = 0; i < 2; ++i)
#pragma unroll
            for (int j = 0; j < 4; ++j)
                acc[i][j] = __builtin_amdgcn_mfma_f32_32x32x16_f16(f.th[j], q.qh[i], acc[i][j], 0, 0, 0);
    };
    // VMEM issue order per wave: t(j + 1) [in advance(j - 1)], q(j) [end of chunk j - 2], t(j + 2)
    // [advance(j)], q(j + 1) [end of chunk j - 1], ...  advance(j) (after chunk j - 1's lo*hi
    // MFMAs) waits until t(j) has landed, with the 6 younger t(j + 1), q(j) in flight; the
    // compiler's own vmcnt waits cover the q registers before their MFMAs.  The barrier publishes
    // chunk j and retires every wave's reads of chunk j - 1, whose buffer chunk j + 2 then takes
    // Every wait count above assumes the VMEM issue order of the source, so the loads are fenced
    // from each other and from the waits by sched_barrier (hipcc otherwise hoists the query loads
    // over the LDS-DMA, e.g. q(0) in front of t(0) -- a race on t(0)), and the phases below stay
    // in program order (left free, hipcc gathers each chunk's LDS reads in front of their first
    // MFMA and exposes their latency every chunk).
#define PHASE __builtin_amdgcn_sched_barrier(0)
    auto advance = [&](int j) {
        PHASE;
        wait_vm<SCOPIES + QLOADS, true>();
        __builtin_amdgcn_s_barrier();
        PHASE;
        issue(j + 2);
        PHASE;
    };

    TFrags fa, fb;
    QFrags qa, qb;
    issue(0);
    PHASE;
    issue(1);
    PHASE;
    load_q(0, qa);
    PHASE;
    wait_vm<SCOPIES + QLOADS, true>();   // t(0) landed (t(1), q(0) may fly)
    __builtin_amdgcn_s_barrier();
    PHASE;
    issue(2);
    PHASE;
    read_lo(0, fa);
    read_hi(0, fa);
    PHASE;
    load_q(1, qb);
    PHASE;
#pragma unroll 1
    for (int kc = 0; kc < nk; kc += 2) {
        mfma_lohi(fa, qa);
        PHASE;
        advance(kc + 1);
        read_lo(kc + 1, fb);
        PHASE;
        mfma_rest(fa, qa);
        PHASE;
        read_hi(kc + 1, fb);
        load_q(kc + 2, qa);
        PHASE;
        if (kc + 1 >= nk) break;   // odd chunk count: fb is a zero chunk
        mfma_lohi(fb, qb);
        PHASE;
        advance(kc + 2);
        read_lo(kc + 2, fa);
        PHASE;
        mfma_rest(fb, qb);
        PHASE;
        read_hi(kc + 2, fa);
        load_q(kc + 3, qb);
        PHASE;
    }
#undef PHASE
    int eq = 0, et = 0;
    load_exponents<split_target>(P, tc, b, q0, tid, eq, et);
    wait_vm<0, true>();             // the exponents and the trailing zero chunks have landed, this wave's reads are done ...
    publish_exponents(smem, tid, eq, et);
    __syncthreads();                // ... in every wave: the chunk buffers are the epilogue's scratch
    pin_acc<true>(acc);

    // ---------------- epilogue (per wave, from registers) ----------------
    split_epilogue<MUL>(P, acc, smem, smem + wave * (4 * 32 * XS), wave * 64, tc, b, q0, lane);
}

// ============================================================================================
// Split GEMM on v_mfma_f32_16x16x32_f16 (D = 256, the E-RAFT feature width: the default build):
// build_split16.h (constants, wait counts, epilogue) and build_split16_loop.h (the body).
// ============================================================================================
template <bool MUL>
__global__ __launch_bounds__(256, 2) void build_split16_kernel(BuildParams P) {
    constexpr int TERMS = 3;   // hi*hi + lo*hi + hi*lo per product
#include "build_split16_loop.h"
}

// ============================================================================================
// fp32 GEMM for D = 256 (ecorr_build): build_split_kernel's structure -- 256 x 128 block tile, 4
// waves of 64 queries x 128 targets, two blocks per CU, the register epilogue split_epilogue() --
// on v_mfma_f32_32x32x2_f32 with the fp32 operands read straight from the fmaps (no operand pass):
//   targets: chunk kc (16 k rows) goes global -> LDS by LDS-DMA as [k][128 targets in split_target
//     order] (8 KB; a lane copies 4 adjacent pixels of one row, 16 bytes, so W % 4 == 0); the A
//     fragment of group j, k-step s is one ds_read_b32 (lane (t, kh): target 32 j + t, k 2 s + kh);
//   queries: the B fragment (lane (q, kh): query 32 i + q of the wave, k 2 s + kh) is one dword
//     load per (i, s) from fmap1 [D][q_count] (a lane pair's 32 queries: two whole 128-byte rows).
// Per element the k order is that of the fp32 build_kernel (chunks, k-steps, the MFMA's own k pair:
// an exact k-ordered fmaf chain), so the pyramid is bitwise the same; the MFMA work per chunk (64
// instructions per wave) is 5.3x the split kernel's, so operand traffic no longer binds.
// ============================================================================================
constexpr int FDT = 3;    // target chunks ahead (LDS buffers)
constexpr int FDQ = 2;    // query chunks ahead (register sets)
constexpr int FQL = 16;   // query dword loads per wave and chunk (2 groups x 8 k-steps)

// VMEM instructions a wave has issued after t(j) when advance(j) waits for it (chunk j - 1, before its
// own t issue): the kernel's issue order replayed at compile time (t = SCOPIES LDS-DMA pieces, q = FQL
// query loads; q(k) exists for k < nk)
constexpr int f32_vm_after(int j, int nk) {
    int n = 0;
    bool seen = false;
    for (int k = 0; k < FDT; ++k) {   // prologue: t(k) q(k)
        if (seen) n += SCOPIES;
        if (k == j) seen = true;
        if (k < FDQ && k < nk && seen) n += FQL;
    }
    for (int c = 0; c <= j - 2; ++c) {   // chunk c: t(c + FDT), q(c + FDQ)
        if (seen) n += SCOPIES;
        if (c + FDT == j) seen = true;
        if (c + FDQ < nk && seen) n += FQL;
    }
    return n;
}
// the waits as literals (hipcc does not fold the replay inside the unrolled loop):
// advance(j) waits with 18 younger ops for j = 1, 2, 16 and 34 for j = 3 .. 15; the prologue with 36
static_assert(f32_vm_after(0, 16) == 36 && f32_vm_after(1, 16) == 18 && f32_vm_after(2, 16) == 18 &&
                  f32_vm_after(3, 16) == 34 && f32_vm_after(15, 16) == 34 && f32_vm_after(16, 16) == 18,
              "fp32 loop wait counts");

template <bool MUL>
__global__ __launch_bounds__(256, 2) void build_f32_kernel(BuildParams P) {
    constexpr int NK = 16;
    __shared__ __attribute__((aligned(16))) char smem[TILE_LDS];   // ALL its LDS (build_tile.h)

    const int tid = threadIdx.x, lane = tid & 63;
    const int wave = __builtin_amdgcn_readfirstlane(tid >> 6);
    int b, qt, nt;
    decode_tile<8, false>(P, xcd_remap(blockIdx.x, gridDim.x), P.n_qt, b, qt, nt);
    b = __builtin_amdgcn_readfirstlane(b);
    qt = __builtin_amdgcn_readfirstlane(qt);
    nt = __builtin_amdgcn_readfirstlane(nt);
    const NTile tc = ntile_of(P, nt);
    const int q0 = qt * SQ;
    const int H = P.H, W = P.W;
    const int64_t Q = (int64_t)H * W;
    // no operand scaling: zero exponents make split_epilogue's scale 1 / sqrt(D) alone
    publish_exponents(smem, tid, 0, 0);

    const __amdgpu_buffer_rsrc_t rq = __builtin_amdgcn_make_buffer_rsrc(
        const_cast<float*>(P.f1 + (int64_t)b * P.D * P.q_count), 0, (int)((int64_t)P.D * P.q_count * 4), 0x00020000);
    const __amdgpu_buffer_rsrc_t rt = __builtin_amdgcn_make_buffer_rsrc(
        const_cast<float*>(P.f2 + (int64_t)b * P.D * Q), 0, (int)((int64_t)P.D * Q * 4), 0x00020000);
    // DMA piece c = wave + 4 s of a chunk: k rows 2c, 2c + 1; lane l copies targets 4 (l & 31) .. +3
    // of row 2c + (l >> 5) (4 adjacent pixels of one image row in split_target order)
    // per-lane byte offsets fixed for the whole loop (the row-dependent part rides in the scalar
    // soffset; a per-load select on the lane offset makes hipcc branch around every load)
    int tvo;   // the lane's 4 pixels in k row (lane >> 5), or out of range outside the image
    {
        int y, x;
        split_target(4 * (lane & 31), tc.band, y, x);
        y += tc.ty0;
        x += tc.tx0;
        tvo = (y < H && x < W) ? (int)(((lane >> 5) * Q + (int64_t)y * W + x) * 4) : SOOB;
    }
    auto issue = [&](int kc) {
        char* dst = smem + (kc % FDT) * SCHUNK;
#pragma unroll
        for (int s = 0; s < SCOPIES; ++s) {
            const int c = wave + 4 * s;
            __builtin_amdgcn_raw_ptr_buffer_load_lds(rt, (__attribute__((address_space(3))) void*)(dst + c * 1024), 16,
                                                     tvo, kc < NK ? (int)((16 * kc + 2 * c) * Q * 4) : SOOB, 0, 0);
        }
    };

    floatx16 acc[2][4];
    zero_acc<true>(acc);   // pinned to AGPRs

    // query fragments: lane (q, kh) of group i, k-step s = fmap1[16 kc + 2 s + kh][q0 + 64 wave + 32 i + q]
    struct QF { float v[2][8]; };
    const int kh = lane >> 5;
    int qvo[2];   // the lane's query in k row kh, or out of range past the slab
#pragma unroll
    for (int i = 0; i < 2; ++i) {
        const int qq = q0 + 64 * wave + 32 * i + (lane & 31);
        qvo[i] = qq < P.q_count ? (int)(((int64_t)kh * P.q_count + qq) * 4) : SOOB;
    }
    auto load_q = [&](int kc, QF& q) {
#pragma unroll
        for (int i = 0; i < 2; ++i)
#pragma unroll
            for (int s = 0; s < 8; ++s)
                q.v[i][s] = __uint_as_float(__builtin_amdgcn_raw_buffer_load_b32(
                    rq, qvo[i], (int)((int64_t)(16 * kc + 2 * s) * P.q_count * 4), 0));
    };
    // target fragments from LDS: group j, k-step s at (2 s + kh) * 512 + (32 j + t) * 4
    struct TF { float v[4][8]; };
    const int tfo = kh * 512 + (lane & 31) * 4;
    auto read_t = [&](int kc, TF& f, int s0) {
        const char* cb = smem + (kc % FDT) * SCHUNK + tfo;
#pragma unroll
        for (int s = s0; s < s0 + 4; ++s)
#pragma unroll
            for (int j = 0; j < 4; ++j) f.v[j][s] = *reinterpret_cast<const float*>(cb + s * 1024 + j * 128);
    };
    auto mfma_half = [&](const TF& f, const QF& q, int s0) {
#pragma unroll
        for (int s = s0; s < s0 + 4; ++s)
#pragma unroll
            for (int i = 0; i < 2; ++i)
#pragma unroll
                for (int j = 0; j < 4; ++j)
                    acc[i][j] = __builtin_amdgcn_mfma_f32_32x32x2f32(f.v[j][s], q.v[i][s], acc[i][j], 0, 0, 0);
    };
#define PHASE __builtin_amdgcn_sched_barrier(0)
    auto advance = [&](int j) {
        PHASE;
        if (j == 1 || j == 2 || j == NK) wait_vm<18, true>();
        else wait_vm<34, true>();
        __builtin_amdgcn_s_barrier();
        PHASE;
        issue(j + FDT - 1);
        PHASE;
    };
    TF f[2];
    QF qs[FDQ];
#pragma unroll
    for (int k = 0; k < FDT; ++k) {
        issue(k);
        PHASE;
        if (k < FDQ) load_q(k, qs[k]);
        PHASE;
    }
    wait_vm<36, true>();   // t(0) landed
    __builtin_amdgcn_s_barrier();
    PHASE;
    read_t(0, f[0], 0);
    read_t(0, f[0], 4);
    PHASE;
#pragma unroll
    for (int kc = 0; kc < NK; ++kc) {
        mfma_half(f[kc & 1], qs[kc % FDQ], 0);
        PHASE;
        advance(kc + 1);
        read_t(kc + 1, f[(kc + 1) & 1], 0);
        PHASE;
        mfma_half(f[kc & 1], qs[kc % FDQ], 4);
        PHASE;
        read_t(kc + 1, f[(kc + 1) & 1], 4);
        if (kc + FDQ < NK) load_q(kc + FDQ, qs[kc % FDQ]);
        PHASE;
    }
#undef PHASE
    wait_vm<0, true>();
    __builtin_amdgcn_s_barrier();   // every wave is done with the chunk buffers (epilogue scratch)
    pin_acc<true>(acc);
    split_epilogue<MUL>(P, acc, smem, smem + wave * (4 * 32 * XS), wave * 64, tc, b, q0, lane);
}

// Split-mode operand pass: per pixel, ex = 15 - E with max_d |x| = f 2^E, f in [0.5, 1) (so the
// pixel's largest scaled value lies in [2^14, 2^15); 0 for all-zero or non-finite maxima, so NaN
// inputs propagate through the GEMM as in the reference), and the f16 split of all D values:
// x 2^ex = hi + lo + O(2^-22 |x|), hi = f16(x 2^ex), lo = f16(x 2^ex - hi) (the subtraction is
// exact; lo is exact for values down to 2^-10 of the pixel maximum and keeps 11 bits down to
// 2^-17 of it -- f16 subnormals below; tests/test_build_modes_gpu.py pins the error over those
// ranges).  Written as the build's 8-KB panels: panel (tile, chunk) = [32-row group g][hi k0-7 |
// hi k8-15 | lo k0-7 | lo k8-15][row r][8 halves], i.e. the v_mfma_f32_32x32x16_f16 operand of lane
// (r, h) is the 16 bytes at g*2048 + part*1024 + lane*16.  Positions without a pixel (ragged
// edges) and k >= D are zeros.  ISB = 0: fmap1 slab, tile = 128 consecutive queries; ISB = 1:
// fmap2, tile = the n-tile's targets in split_target order.  Block = 64 positions x 4 chunk
// quarters; the D <= 256 values of a thread stay in registers between the max and the split.
// (split_exponent and split_f16: split_f16.h.)
//
// L16: the panel layout of build_split16_kernel (16 KB per 128-pixel tile and 32-deep chunk pair:
// [16-pixel group g][hi | lo][k block kb][pixel r][8 halves], k = 8 kb + j within the pair; fmap2
// positions in split16_target order) instead of build_split_kernel's 8-KB chunk panels.
//
// T: the element the operands are stored as (float, _Float16 or __bf16: ecorr_build_split_pack_as),
// converted to fp32 on load -- exactly; everything after the load is the fp32 pass.  Lanes stay
// consecutive pixels (2-byte loads: a 16-bit slab view may be 2-byte aligned only).  A 16-bit element
// is loaded as its bit pattern (0 where the lane has no pixel or k >= D); on the register path all
// of a thread's patterns are loaded before the first is converted: with the convert beside the load
// hipcc keeps it inside the load's branch with a vmcnt(0) wait behind it -- 64 serialized round
// trips per thread where the fp32 pass has its loads in flight together (the pack alone 98 vs 63 us
// at DSEC B = 16 in that form, profiles/half_io/).
template <bool ISB, bool L16, typename T>
__device__ __forceinline__ void pack_body(const T* __restrict__ x, const BuildParams& P, int* __restrict__ ex,
                                          char* __restrict__ pack) {
    __shared__ float red[4][64];
    const int b = blockIdx.y;
    int tile = blockIdx.x >> 1;
    int pos = (blockIdx.x & 1) * 64 + (threadIdx.x & 63);   // panel position of this lane's pixel
    const int qtr = threadIdx.x >> 6, D = P.D, dc = (D + 15) / 16;
    const int64_t N = ISB ? (int64_t)P.H * P.W : (int64_t)P.q_count;
    int64_t pix = -1;
    bool live = true;   // the lane owns a panel position (it writes its zeros too)
    if (!ISB) {
        const int64_t p = (int64_t)tile * 128 + pos;
        if (p < P.q_count) pix = p;
    } else {
        // lanes on 2 rows x 32 consecutive pixels (whole 128-byte lines of fmap2: an L2 miss
        // fetches the whole line, so 16-pixel row pieces read every line twice): regular blocks
        // cover rows 2 r4, 2 r4 + 1 of a pair of horizontally adjacent 8 x 16 n-tiles, band blocks
        // rows 2 h, 2 h + 1 of one 4 x 32 band tile; each lane goes to its n-tile's panel
        // position (split_target inverted)
        const int l = threadIdx.x & 63, npair = (P.n_ntx + 1) / 2, nreg_blk = 4 * (P.n_reg / P.n_ntx) * npair;
        int y, x;
        bool ok;
        if ((int)blockIdx.x < nreg_blk) {
            const int r4 = blockIdx.x & 3, pr = blockIdx.x >> 2, trow = pr / npair, col = 2 * (pr - trow * npair) + (l >> 4 & 1);
            ok = col < P.n_ntx;
            tile = trow * P.n_ntx + (ok ? col : 0);
            // L16: rows r4, r4 + 4, whose 16 pixels per n-tile row half complete two 16-position
            // groups of the panel (256-byte runs per store); otherwise rows 2 r4, 2 r4 + 1
            y = L16 ? r4 + 4 * (l >> 5) : 2 * r4 + (l >> 5);
            x = l & 15;
            pos = L16 ? 16 * (2 * (y & 3) + ((x >> 2) & 1)) + 4 * ((y >> 2) | ((x >> 3) << 1)) + (x & 3)
                      : 64 * (x >> 3) + 32 * (y >> 2) + 8 * (y & 3) + (x & 7);
        } else {
            const int bb = blockIdx.x - nreg_blk;
            tile = P.n_reg + (bb >> 1);
            ok = tile < P.n_nt;
            y = 2 * (bb & 1) + (l >> 5);
            x = l & 31;
            pos = L16 ? 16 * (2 * y + ((x >> 2) & 1)) + 4 * (x >> 3) + (x & 3) : 32 * (x >> 3) + 8 * y + (x & 7);
        }
        const NTile n = ntile_of(P, ok ? tile : 0);
        live = ok;
        if (ok && n.ty0 + y < P.H && n.tx0 + x < P.W) pix = (int64_t)(n.ty0 + y) * P.W + n.tx0 + x;
    }
    using Raw = std::conditional_t<std::is_same_v<T, float>, float, unsigned short>;   // the element as loaded
    const Raw* px = reinterpret_cast<const Raw*>(x) + (int64_t)b * D * N + (pix < 0 ? 0 : pix);
    auto cv = [](Raw r) -> float {
        if constexpr (std::is_same_v<T, float>) return r;
        else return (float)__builtin_bit_cast(T, r);
    };
    constexpr int CPT = 4;
    const bool regs = dc <= 4 * CPT;
    float v[CPT][16];
    float m = 0.f;
    if (regs) {
        if constexpr (std::is_same_v<T, float>) {
#pragma unroll
            for (int i = 0; i < CPT; ++i)
#pragma unroll
                for (int kk = 0; kk < 16; ++kk) {
                    const int k = (qtr + 4 * i) * 16 + kk;
                    v[i][kk] = (pix >= 0 && k < D) ? px[(int64_t)k * N] : 0.f;
                    m = fmaxf(m, fabsf(v[i][kk]));
                }
        } else {
            // all the bit patterns first, each pinned in its register behind the last load, then the
            // converts: left to itself hipcc converts inside each load's branch, with a vmcnt(0)
            // wait per load (see above)
            unsigned r[CPT][16];
#pragma unroll
            for (int i = 0; i < CPT; ++i)
#pragma unroll
                for (int kk = 0; kk < 16; ++kk) {
                    const int k = (qtr + 4 * i) * 16 + kk;
                    r[i][kk] = (pix >= 0 && k < D) ? px[(int64_t)k * N] : 0u;
                }
#pragma unroll
            for (int i = 0; i < CPT; ++i)
#pragma unroll
                for (int kk = 0; kk < 16; ++kk) {
                    asm volatile("" : "+v"(r[i][kk]));
                    v[i][kk] = cv((Raw)r[i][kk]);
                    m = fmaxf(m, fabsf(v[i][kk]));
                }
        }
    } else if (pix >= 0) {
        for (int k = qtr * 16; k < D; k += 64)
#pragma unroll 4
            for (int kk = 0; kk < 16 && k + kk < D; ++kk) m = fmaxf(m, fabsf(cv(px[(int64_t)(k + kk) * N])));
    }
    red[qtr][threadIdx.x & 63] = m;
    __syncthreads();
    const int l = threadIdx.x & 63;
    m = fmaxf(fmaxf(red[0][l], red[1][l]), fmaxf(red[2][l], red[3][l]));
    const int e = split_exponent(m);
    if (qtr == 0 && pix >= 0) ex[(int64_t)b * N + pix] = e;
    const float s = exp2i(e);
    const int ntiles = ISB ? P.n_nt : P.n_mt;
    char* pan = pack + ((int64_t)b * ntiles + tile) * dc * PANEL +
                (L16 ? (pos >> 4) * 2048 + (pos & 15) * 16 : (pos >> 5) * 2048 + (pos & 31) * 16);
    auto put = [&](int c, const float (&w)[16]) {
        halfx8 h0, l0, h1, l1;
        split_f16(*reinterpret_cast<const float(*)[8]>(w), s, h0, l0);
        split_f16(*reinterpret_cast<const float(*)[8]>(w + 8), s, h1, l1);
        // L16: chunk c is k blocks 2 (c & 1), 2 (c & 1) + 1 of chunk pair c / 2
        char* p = L16 ? pan + (int64_t)(c >> 1) * 2 * PANEL + (c & 1) * 512 : pan + (int64_t)c * PANEL;
        const int k8 = L16 ? 256 : 512;   // the next 8 k
        *reinterpret_cast<halfx8*>(p) = h0;
        *reinterpret_cast<halfx8*>(p + k8) = h1;
        *reinterpret_cast<halfx8*>(p + 1024) = l0;
        *reinterpret_cast<halfx8*>(p + 1024 + k8) = l1;
    };
    if (!live) return;   // (after the block's only barrier)
    if (regs) {
#pragma unroll
        for (int i = 0; i < CPT; ++i)
            if (qtr + 4 * i < dc) put(qtr + 4 * i, v[i]);
        return;
    }
    for (int c = qtr; c < dc; c += 4) {
        float w[16];
#pragma unroll
        for (int kk = 0; kk < 16; ++kk) {
            const int k = c * 16 + kk;
            w[kk] = cv((pix >= 0 && k < D) ? px[(int64_t)k * N] : Raw(0));
        }        put(c, w);
    }
}

// Both operand passes in ONE launch: grid (2 * max(n_mt, n_nt), B, 2), z = 0 packs fmap1 (128-query
// tiles), z = 1 fmap2 (n-tiles).  Neither pass alone fills the chip; one grid overlaps the two and
// drops a launch boundary (round-1 A/B, profiles/r01_final8/ab_pack.txt).  Surplus x blocks of the
// shorter pass return at once (block-uniform, before pack_body's barrier).
// T: the fmaps' element (P.f1 / P.f2 point at elements of T; float: the fp32 entries).
// x blocks of the fmap2 pass (pack_body<true>): 4 per pair of regular n-tiles, 2 per band tile
__host__ __device__ __forceinline__ int pack_grid_x(const BuildParams& P) {
    return 4 * (P.n_reg / P.n_ntx) * ((P.n_ntx + 1) / 2) + 2 * (P.n_nt - P.n_reg);
}

template <bool L16, typename T = float>
__global__ __launch_bounds__(256) void pack_both_kernel(BuildParams P) {
    if (blockIdx.z == 0) {
        if ((int)blockIdx.x < 2 * P.n_mt)
            pack_body<false, L16, T>(reinterpret_cast<const T*>(P.f1), P, P.ex1, const_cast<char*>(P.pk1));
    } else if ((int)blockIdx.x < pack_grid_x(P)) {
        pack_body<true, L16, T>(reinterpret_cast<const T*>(P.f2), P, P.ex2, const_cast<char*>(P.pk2));
    }
}

// ============================================================================================
// fp32 GEMM (ecorr_build).  Block tile 128 queries x one 8 x 16 (or 4 x 32 band) target block,
// K staged 16 deep; 4 waves of 64 x 64 = 2 x 2 v_mfma_f32_32x32x2_f32 tiles, 3 blocks per CU.
// GLDS: the K chunks go global -> LDS directly (buffer_load_dwordx4 ... lds, whose range check
// zero-fills the padding) through 3 buffers with two chunks in flight; otherwise (ragged shapes,
// operands beyond the 31-bit buffer range) float4 / scalar register staging, double-buffered.
// The C tile passes through LDS in two 64-query halves; the epilogue pools each (query, 8 x 8
// block) in registers and leaves as whole tiles (levels 0-1) and row pieces (levels 2-3).
// ============================================================================================
constexpr int BM = 128;             // queries per block tile
constexpr int BN = TBH * TBW;       // 128 targets
constexpr int NT = 256;             // threads
constexpr int KB = 16;              // K chunk
constexpr int MR = BM / 2;          // C-tile rows per half
constexpr int CS = BN + 4;          // C-tile LDS row stride (floats): conflict-free ds_read_b128
constexpr int P1S = 36, P2S = 12;   // LDS per-query strides of the pooled staging (conflict-free)
constexpr int FNBUF = 3;
constexpr int FSM = (FNBUF * KB * (BM + BN) > MR * CS) ? FNBUF * KB * (BM + BN) : MR * CS;

template <typename V>
__device__ __forceinline__ void st_nt(V* p, V v) { __builtin_nontemporal_store(v, p); }

// What the two epilogues below share: 8 consecutive floats of a C-tile row from LDS, and 4
// consecutive level-2 pixels (r, c .. c + 3) of query image row from the pooled staging
__device__ __forceinline__ void read_row8(const float* p, float (&v)[8]) {
    const floatx4 lo = *reinterpret_cast<const floatx4*>(p);
    const floatx4 hi = *reinterpret_cast<const floatx4*>(p + 4);
#pragma unroll
    for (int j = 0; j < 4; ++j) { v[j] = lo[j]; v[4 + j] = hi[j]; }
}
__device__ __forceinline__ void store_level2_row(const BuildParams& P, int64_t row, int r, int c, const float* src) {
#pragma unroll
    for (int j = 0; j < 4; ++j) {
        float* p = level_px(P, 2, row, r, c + j);
        if (p) *p = src[j];
    }
}

// Epilogue of a regular tile (all threads; contains barriers).  Cs = scaled C-tile rows ([m][n],
// stride CS, n = ty*16 + tx) of MR of the block's queries: query images row0 .. of the pyramid, the
// first mvalid of them in range.  Level 0: 4 whole tiles per query; pooling: thread (query m,
// 8 x 8 block blk) reduces in registers 8x8 -> 4x4 -> 2x2 -> 1, each level from the rounded previous one, parks levels 1-3 in LDS, then level 1 leaves as
// one whole tile per query, level 2 as two 16-byte rows, level 3 as single pixels.
__device__ __forceinline__ void epilogue(const BuildParams& P, const NTile& tc, float* Cs, int tid, int64_t row0,
                                         int mvalid) {
    {   // level 0
        const int ntx = P.lntx[0], nty = P.lnty[0];
        const int tr0 = tc.ty0 / kTileH, tc0 = tc.tx0 / kTileW;
#pragma unroll 4
        for (int s = 0; s < (MR * 32) / NT; ++s) {
            const int idx = tid + NT * s;
            const int m = idx >> 5, rem = idx & 31;
            const int trl = rem >> 4, tcl = (rem >> 3) & 1, j = rem & 7;
            const int tr = tr0 + trl, tcc = tc0 + tcl;
            if (m < mvalid && tr < nty && tcc < ntx) {
                const floatx4 v = *reinterpret_cast<const floatx4*>(
                    Cs + m * CS + (trl * 4 + (j >> 1)) * TBW + tcl * 8 + (j & 1) * 4);
                st_nt(reinterpret_cast<floatx4*>(P.lvl[0] + (row0 + m) * P.lsz[0] + tile_base(tr, tcc, ntx) + 4 * j), v);
            }
        }
    }
    if (P.fused_levels < 2) return;   // uniform over the block
    const bool pooler = tid < 2 * MR;
    const int m = tid % MR, blk = tid / MR;
    float l1[4][4], l2[2][2], l3 = 0.0f;
    if (pooler) {
        float v[8][8];
#pragma unroll
        for (int ty = 0; ty < 8; ++ty) read_row8(Cs + m * CS + ty * TBW + blk * 8, v[ty]);
#pragma unroll
        for (int y = 0; y < 4; ++y)
#pragma unroll
            for (int x = 0; x < 4; ++x)
                l1[y][x] = pool4(v[2 * y][2 * x], v[2 * y][2 * x + 1], v[2 * y + 1][2 * x], v[2 * y + 1][2 * x + 1]);
#pragma unroll
        for (int y = 0; y < 2; ++y)
#pragma unroll
            for (int x = 0; x < 2; ++x)
                l2[y][x] = pool4(l1[2 * y][2 * x], l1[2 * y][2 * x + 1], l1[2 * y + 1][2 * x], l1[2 * y + 1][2 * x + 1]);
        l3 = pool4(l2[0][0], l2[0][1], l2[1][0], l2[1][1]);
    }
    __syncthreads();   // all reads of Cs done: reuse it for the pooled staging
    float* S1 = Cs;                       // [MR][4 rows][8 cols] = the level-1 tile, stride P1S
    float* S2 = Cs + MR * P1S;            // [MR][2 rows][4 cols], stride P2S
    float* S3 = S2 + MR * P2S;            // [MR][2 cols]
    if (pooler) {
#pragma unroll
        for (int y = 0; y < 4; ++y)
            *reinterpret_cast<floatx4*>(S1 + m * P1S + y * 8 + blk * 4) = floatx4{l1[y][0], l1[y][1], l1[y][2], l1[y][3]};
#pragma unroll
        for (int y = 0; y < 2; ++y)
            *reinterpret_cast<floatx2*>(S2 + m * P2S + y * 4 + blk * 2) = floatx2{l2[y][0], l2[y][1]};
        S3[m * 2 + blk] = l3;
    }
    __syncthreads();
    {   // level 1 (interleaved): rows ty0/2 .. +3, cols tx0/2 .. +7, 8 float4 block-row pieces per query
#pragma unroll
        for (int s = 0; s < (MR * 8) / NT; ++s) {
            const int idx = tid + NT * s;
            const int mm = idx >> 3, j = idx & 7;
            float* p = mm < mvalid ? level_px(P, 1, row0 + mm, tc.ty0 / 2 + (j >> 1), tc.tx0 / 2 + 4 * (j & 1)) : nullptr;
            if (p) st_nt(reinterpret_cast<floatx4*>(p), *reinterpret_cast<const floatx4*>(S1 + mm * P1S + 4 * j));
        }
    }
    if (P.fused_levels >= 3 && tid < 2 * MR) {   // level 2: rows ty0/4 + {0,1}, cols tx0/4 .. +3
        const int mm = tid >> 1, y = tid & 1;
        if (mm < mvalid) store_level2_row(P, row0 + mm, tc.ty0 / 4 + y, tc.tx0 / 4, S2 + mm * P2S + y * 4);
    }
    if (P.fused_levels >= 4 && tid < MR && tid < mvalid) {   // level 3: row ty0/8, cols tx0/8 .. +1
#pragma unroll
        for (int j = 0; j < 2; ++j) {
            float* p = level_px(P, 3, row0 + tid, tc.ty0 / 8, tc.tx0 / 8 + j);
            if (p) *p = S3[tid * 2 + j];
        }
    }
}

// Epilogue of a band tile (4 target rows x 32 cols; n = ty*32 + tx).  Level 0: one tile row of
// 4 tiles per query.  Pooling: thread (query m, 4x8 block blk = 0..3) reduces 4x8 -> 2x4 -> 1x2 in
// registers (the reference's order, from the rounded previous level); level 1 leaves as two 8-float
// rows of two tiles, level 2 as single pixels.  No level-3 pixel draws on these rows.
__device__ __forceinline__ void epilogue_band(const BuildParams& P, const NTile& tc, float* Cs, int tid, int64_t row0,
                                              int mvalid) {
    {   // level 0: tile row ty0/4, tile cols tx0/8 .. +3
        const int ntx = P.lntx[0];
        const int tr = tc.ty0 / kTileH, tc0 = tc.tx0 / kTileW;
#pragma unroll 4
        for (int s = 0; s < (MR * 32) / NT; ++s) {
            const int idx = tid + NT * s;
            const int m = idx >> 5, rem = idx & 31;
            const int tcl = rem >> 3, j = rem & 7;
            if (m < mvalid && tc0 + tcl < ntx) {
                const floatx4 v = *reinterpret_cast<const floatx4*>(Cs + m * CS + (j >> 1) * 32 + tcl * 8 + (j & 1) * 4);
                st_nt(reinterpret_cast<floatx4*>(P.lvl[0] + (row0 + m) * P.lsz[0] + tile_base(tr, tc0 + tcl, ntx) + 4 * j), v);
            }
        }
    }
    if (P.fused_levels < 2) return;
    constexpr int NU = (4 * MR + NT - 1) / NT;   // (query, block) items per thread
    float l1[NU][2][4], l2[NU][2];
#pragma unroll
    for (int u = 0; u < NU; ++u) {
        const int it = tid + NT * u, m = it % MR, blk = it / MR;
        if (it < 4 * MR) {
            float v[4][8];
#pragma unroll
            for (int ty = 0; ty < 4; ++ty) read_row8(Cs + m * CS + ty * 32 + blk * 8, v[ty]);
#pragma unroll
            for (int y = 0; y < 2; ++y)
#pragma unroll
                for (int x = 0; x < 4; ++x)
                    l1[u][y][x] = pool4(v[2 * y][2 * x], v[2 * y][2 * x + 1], v[2 * y + 1][2 * x], v[2 * y + 1][2 * x + 1]);
#pragma unroll
            for (int x = 0; x < 2; ++x)
                l2[u][x] = pool4(l1[u][0][2 * x], l1[u][0][2 * x + 1], l1[u][1][2 * x], l1[u][1][2 * x + 1]);
        }
    }
    __syncthreads();   // all reads of Cs done: reuse it for the pooled staging
    float* S1 = Cs;                 // [MR][2 rows][16 cols], stride P1S
    float* S2 = Cs + MR * P1S;      // [MR][8 cols], stride P2S
#pragma unroll
    for (int u = 0; u < NU; ++u) {
        const int it = tid + NT * u, m = it % MR, blk = it / MR;
        if (it < 4 * MR) {
#pragma unroll
            for (int y = 0; y < 2; ++y)
                *reinterpret_cast<floatx4*>(S1 + m * P1S + y * 16 + blk * 4) =
                    floatx4{l1[u][y][0], l1[u][y][1], l1[u][y][2], l1[u][y][3]};
            *reinterpret_cast<floatx2*>(S2 + m * P2S + blk * 2) = floatx2{l2[u][0], l2[u][1]};
        }
    }
    __syncthreads();
    {   // level 1 (interleaved): rows ty0/2 .. +1, cols tx0/2 .. +15, 8 float4 block-row pieces per query
#pragma unroll
        for (int s = 0; s < (MR * 8 + NT - 1) / NT; ++s) {
            const int idx = tid + NT * s;
            const int mm = idx >> 3, t = idx & 7;
            const int y = t >> 2, tcl = (t >> 1) & 1, hf = t & 1;
            float* p = mm < mvalid ? level_px(P, 1, row0 + mm, tc.ty0 / 2 + y, tc.tx0 / 2 + tcl * 8 + hf * 4) : nullptr;
            if (p)
                st_nt(reinterpret_cast<floatx4*>(p), *reinterpret_cast<const floatx4*>(S1 + mm * P1S + y * 16 + tcl * 8 + hf * 4));
        }
    }
    if (P.fused_levels >= 3 && tid < 2 * MR) {   // level 2: row ty0/4, cols tx0/4 .. +7
        const int mm = tid >> 1, hf = tid & 1;
        if (mm < mvalid) store_level2_row(P, row0 + mm, tc.ty0 / 4, tc.tx0 / 4 + hf * 4, S2 + mm * P2S + hf * 4);
    }
}

// VEC: float4 operand loads (W and q_count multiples of 4, 16-byte aligned fmaps); GLDS: LDS-DMA
// staging (needs VEC and byte offsets below 2^31).  A/B record: LDS-DMA 2.4-4% faster than
// register staging; 16x16x4 tiles 1% slower than 32x32x2; KB = 32 / 4 blocks per CU / setprio /
// k-permuted layouts / fragment prefetch all slower.
template <bool VEC, bool GLDS>
__global__ __launch_bounds__(NT, 3) void build_kernel(BuildParams P) {
    constexpr int AS = BM, BSS = BN;           // LDS row strides
    constexpr int NLD = (KB * BM / 4) / NT;    // float4 of A (and of B) per thread per chunk (2)
    constexpr int NBUF = GLDS ? FNBUF : 2;
    static_assert(!GLDS || VEC, "GLDS: vector path");
    __shared__ __attribute__((aligned(16))) float smem[FSM];
    float* As = smem;                       // [NBUF][KB][AS]
    float* Bs = smem + NBUF * KB * AS;      // [NBUF][KB][BSS]

    const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
    int b, mt, nt;
    const NTile tc = block_tile<8, false>(P, P.n_mt, b, mt, nt);
    const int m0 = mt * BM;
    const int q_end = P.q_count;
    const int H = P.H, W = P.W, D = P.D;
    const int64_t Q = (int64_t)H * W;
    const int64_t QA = P.q_count;
    const float* __restrict__ A = P.f1 + (int64_t)b * D * QA;
    const float* __restrict__ Bm = P.f2 + (int64_t)b * D * Q;

    floatx4 ra[NLD], rb[NLD];
    auto load_chunk = [&](int k0) {
#pragma unroll
        for (int i = 0; i < NLD; ++i) {
            const int s = tid + NT * i;
            const int k = k0 + (s >> 5);
            {   // A: row k, queries m0 + 4c .. +3
                const int m = m0 + 4 * (s & 31);
                floatx4 v = {0.f, 0.f, 0.f, 0.f};
                if (VEC) {
                    if (k < D && m < q_end) v = *reinterpret_cast<const floatx4*>(A + (int64_t)k * QA + m);
                } else {
#pragma unroll
                    for (int j = 0; j < 4; ++j)
                        if (k < D && m + j < q_end) v[j] = A[(int64_t)k * QA + m + j];
                }
                ra[i] = v;
            }
            {   // B: row k, target row ty0 + ty, cols tx0 + 4c .. +3 (LDS column 4r = ty*TBW + tx)
                const int r = s & 31;
                const int y = tc.ty0 + (tc.band ? r >> 3 : r >> 2), x = tc.tx0 + 4 * (tc.band ? r & 7 : r & 3);
                floatx4 v = {0.f, 0.f, 0.f, 0.f};
                if (VEC) {
                    if (k < D && y < H && x < W)
                        v = *reinterpret_cast<const floatx4*>(Bm + (int64_t)k * Q + (int64_t)y * W + x);
                } else {
#pragma unroll
                    for (int j = 0; j < 4; ++j)
                        if (k < D && y < H && x + j < W) v[j] = Bm[(int64_t)k * Q + (int64_t)y * W + x + j];
                }
                rb[i] = v;
            }
        }
    };
    auto store_chunk = [&](int buf) {
#pragma unroll
        for (int i = 0; i < NLD; ++i) {
            const int s = tid + NT * i;
            const int kk = s >> 5, c = s & 31;
            *reinterpret_cast<floatx4*>(As + (buf * KB + kk) * AS + 4 * c) = ra[i];
            *reinterpret_cast<floatx4*>(Bs + (buf * KB + kk) * BSS + 4 * c) = rb[i];
        }
    };

    floatx16 acc[2][2];
#pragma unroll
    for (int i = 0; i < 2; ++i)
#pragma unroll
        for (int j = 0; j < 2; ++j)
#pragma unroll
            for (int r = 0; r < 16; ++r) acc[i][j][r] = 0.0f;

    // MFMA 32x32x2 f32 operand maps: lane l holds A[i = l&31][k = l>>5] and B[k = l>>5][j = l&31]
    const int wm = wave & 1, wn = wave >> 1;
    const int arow = lane >> 5, acol = lane & 31;
    const int nk = (D + KB - 1) / KB;

    auto mfma_chunk = [&](int buf) {
        const float* as = As + buf * KB * AS + wm * 64 + acol;
        const float* bs = Bs + buf * KB * BSS + wn * 64 + acol;
#pragma unroll
        for (int kk = 0; kk < KB; kk += 2) {
            const int ro = kk + arow;
            const float a0 = as[ro * AS], a1 = as[ro * AS + 32];
            const float b0 = bs[ro * BSS], b1 = bs[ro * BSS + 32];
            acc[0][0] = __builtin_amdgcn_mfma_f32_32x32x2f32(a0, b0, acc[0][0], 0, 0, 0);
            acc[0][1] = __builtin_amdgcn_mfma_f32_32x32x2f32(a0, b1, acc[0][1], 0, 0, 0);
            acc[1][0] = __builtin_amdgcn_mfma_f32_32x32x2f32(a1, b0, acc[1][0], 0, 0, 0);
            acc[1][1] = __builtin_amdgcn_mfma_f32_32x32x2f32(a1, b1, acc[1][1], 0, 0, 0);
        }
    };

    if constexpr (GLDS) {
        // copy i of this wave covers chunk rows kk = 2 wave + 8 i + (lane >> 5), 4 floats at
        // column 4 (lane & 31): lane-linear 1 KB per wave-instruction, as LDS-DMA requires
        const __amdgpu_buffer_rsrc_t rsa =
            __builtin_amdgcn_make_buffer_rsrc(const_cast<float*>(A), 0, (int)((int64_t)D * QA * 4), 0x00020000);
        const __amdgpu_buffer_rsrc_t rsb =
            __builtin_amdgcn_make_buffer_rsrc(const_cast<float*>(Bm), 0, (int)((int64_t)D * Q * 4), 0x00020000);
        const int c = lane & 31, kl = lane >> 5;
        const int m = m0 + 4 * c;
        const int y = tc.ty0 + (tc.band ? c >> 3 : c >> 2), x = tc.tx0 + 4 * (tc.band ? c & 7 : c & 3);
        const bool aok = m < q_end, bok = y < H && x < W;
        const int abase = m * 4, bbase = (y * W + x) * 4;
        auto issue = [&](int kc) {
            const int buf = kc % NBUF;
#pragma unroll
            for (int i = 0; i < NLD; ++i) {
                const int kk = 2 * wave + 8 * i;   // wave-uniform first row of this copy
                const int k = kc * KB + kk + kl;
                const bool kin = k < D;
                __builtin_amdgcn_raw_ptr_buffer_load_lds(
                    rsa, (__attribute__((address_space(3))) void*)(As + (buf * KB + kk) * AS), 16,
                    aok && kin ? abase + k * (int)QA * 4 : SOOB, 0, 0, 0);
                __builtin_amdgcn_raw_ptr_buffer_load_lds(
                    rsb, (__attribute__((address_space(3))) void*)(Bs + (buf * KB + kk) * BSS), 16,
                    bok && kin ? bbase + k * (int)Q * 4 : SOOB, 0, 0, 0);
            }
        };
        for (int kc = 0; kc < NBUF - 1 && kc < nk; ++kc) issue(kc);
        for (int kc = 0; kc < nk; ++kc) {
            // this wave's copies of chunk kc have landed (those of chunk kc + 1 may still fly) ...
            if (kc + 1 < nk) wait_vm<2 * NLD, false>();
            else wait_vm<0, false>();
            // ... and every wave's have once all passed this barrier, which also retires the
            // reads of chunk kc - 1, whose buffer chunk kc + 2 now overwrites
            __builtin_amdgcn_s_barrier();
            if (kc + NBUF - 1 < nk) issue(kc + NBUF - 1);
            mfma_chunk(kc % NBUF);
        }
        __syncthreads();   // the C tile aliases the chunk buffers
    } else {
        load_chunk(0);
        store_chunk(0);
        __syncthreads();
        for (int kc = 0; kc < nk; ++kc) {
            const int buf = kc & 1;
            if (kc + 1 < nk) load_chunk((kc + 1) * KB);
            mfma_chunk(buf);
            if (kc + 1 < nk) store_chunk(buf ^ 1);
            __syncthreads();
        }
    }

    // ---- scaled accumulators -> LDS C tile [m][n] in two 64-query halves; C/D map:
    //      col = lane&31, row = mfma_c_row(reg, lane>>5) ----
    float* Cs = smem;
#pragma unroll
    for (int half = 0; half < 2; ++half) {
        if (wm == half) {
            // one uniform branch on the scale mode around the whole tile (a per-element select
            // had the compiler emit an IEEE division next to every element's multiply)
            auto write_c = [&](auto scaled) {
#pragma unroll
                for (int i = 0; i < 2; ++i)
#pragma unroll
                    for (int j = 0; j < 2; ++j)
#pragma unroll
                        for (int r = 0; r < 16; ++r) {
                            const int m = i * 32 + mfma_c_row(r, arow);
                            const int n = wn * 64 + j * 32 + acol;
                            Cs[m * CS + n] = scaled(acc[i][j][r]);
                        }
            };
            if (P.scale_is_mul) write_c([&](float v) { return __fmul_rn(v, P.scale); });
            else write_c([&](float v) { return __fdiv_rn(v, P.scale); });
        }
        __syncthreads();
        // this half's query images and how many of them are in range
        const int64_t row0 = (int64_t)b * P.q_count + m0 + half * MR;
        const int mvalid = min(MR, P.q_count - m0 - half * MR);
        if (tc.band) epilogue_band(P, tc, Cs, tid, row0, mvalid);
        else epilogue(P, tc, Cs, tid, row0, mvalid);
        if (half == 0) __syncthreads();   // half 0 fully consumed before half 1 overwrites Cs
    }
}

// Levels beyond the 4 fused ones (num_levels > 4): plain 2x2 floor-mode pooling, tiled in and
// out, one thread per output pixel.  Not on the E-RAFT path (num_levels = 4, eraft.py:50).
__global__ __launch_bounds__(256) void pool2_kernel(const float* __restrict__ in, float* __restrict__ out,
                                                    int64_t rows, int h, int w, int lv_in, int ntx_in, int64_t sz_in,
                                                    int ntx_out, int64_t sz_out) {
    const int ho = h / 2, wo = w / 2;
    const int64_t n = rows * ho * wo;
    for (int64_t i = blockIdx.x * (int64_t)blockDim.x + threadIdx.x; i < n; i += (int64_t)gridDim.x * blockDim.x) {
        const int64_t rw = i / ((int64_t)ho * wo);
        const int yx = (int)(i - rw * ho * wo);
        const int y = yx / wo, x = yx - y * wo;
        auto at = [&](int yy, int xx) { return in[pix_off(rw, yy, xx, lv_in, ntx_in, w, sz_in)]; };
        out[rw * sz_out + level_off(y, x, ntx_out, wo)] =
            pool4(at(2 * y, 2 * x), at(2 * y, 2 * x + 1), at(2 * y + 1, 2 * x), at(2 * y + 1, 2 * x + 1));
    }
}

}  // namespace

namespace {
void tile_counts(BuildParams& P) {
    P.n_ntx = (P.W + TBW - 1) / TBW;
    // 8-row tile rows; a remainder of 1..4 rows (the last 8k + r rows, r <= 4) becomes a band of
    // 4 x 32 tiles (see ntile_of), a remainder of 5..7 a padded regular tile row
    const int rem = P.H % TBH;
    const bool band = rem > 0 && rem <= 4;
    P.n_reg = P.n_ntx * (band ? P.H / TBH : (P.H + TBH - 1) / TBH);
    P.band_y0 = (P.H / TBH) * TBH;
    P.n_nt = P.n_reg + (band ? (P.W + 31) / 32 : 0);
    P.n_mt = (P.q_count + BM - 1) / BM;      // 128-query tiles (fp32 blocks, fmap1 panels)
    P.n_qt = (P.q_count + SQ - 1) / SQ;      // 256-query tiles (split blocks)
}

// split workspace: exponents (fmap1 slab, fmap2), then fmap1 and fmap2 panels (256-B aligned)
struct SplitWs { int64_t ex2, pk1, pk2, total; };
SplitWs split_ws(const BuildParams& P, int B) {
    const int64_t dc = (P.D + 15) / 16;
    SplitWs w;
    w.ex2 = (int64_t)B * P.q_count * 4;
    w.pk1 = (w.ex2 + (int64_t)B * P.H * P.W * 4 + 255) & ~(int64_t)255;
    w.pk2 = w.pk1 + (int64_t)B * P.n_mt * dc * PANEL;
    w.total = w.pk2 + (int64_t)B * P.n_nt * dc * PANEL;
    return w;
}
}  // namespace

int64_t build_split_workspace_bytes(int B, int D, int H, int W, int q_count) {
    BuildParams P{};
    P.D = D;
    P.H = H;
    P.W = W;
    P.q_count = q_count;
    tile_counts(P);
    return split_ws(P, B).total;
}

namespace {
// the operand pass on fmaps of element T (ECORR_ELEM_*: InElem)
template <typename T>
void launch_pack(const BuildParams& P, int nx, int B, bool s16, hipStream_t stream) {
    if (s16) hipLaunchKernelGGL((pack_both_kernel<true, T>), dim3((unsigned)nx, B, 2), dim3(256), 0, stream, P);
    else hipLaunchKernelGGL((pack_both_kernel<false, T>), dim3((unsigned)nx, B, 2), dim3(256), 0, stream, P);
}

// a 256 x 128 kernel's instantiation for the scale mode: mul<true> / div<false>
void launch_mul(const BuildParams& P, int64_t ntiles, hipStream_t stream, void (*mul)(BuildParams),
                void (*div)(BuildParams)) {
    hipLaunchKernelGGL(P.scale_is_mul ? mul : div, dim3((unsigned)ntiles), dim3(256), 0, stream, P);
}

// both fp32 operands' byte offsets fit the 31-bit buffer range
bool fits_buffer_range(const BuildParams& P) {
    return (int64_t)P.D * P.H * P.W * 4 < 0x7fff0000LL && (int64_t)P.D * P.q_count * 4 < 0x7fff0000LL;
}
}  // namespace

int launch_build(const BuildParams& P0, int B, const PyrGeom& g, float* pyramid, hipStream_t stream, int stages,
                 int fmap_format, bool hi) {
    BuildParams P = P0;
    const int levels = g.levels;
    P.fused_levels = levels < 4 ? levels : 4;
    tile_counts(P);
    level_table<float>(g, pyramid, &P);   // zeros past the last level: the kernels index levels < 4 unguarded
    if ((uintptr_t)pyramid % 16 != 0) return ECORR_EINVAL;   // tile stores are 16-byte vectors
    if (P.ws) {
        // split build: one 128-query tile's panels (dc * 8 KB, the buffer range of the kernel's
        // per-tile descriptors) always fit 31 bits for D < 2^22
        const int64_t ntiles = (int64_t)B * P.n_qt * P.n_nt;
        if (ntiles <= 0 || ntiles > 0x7fffffff || (int64_t)2 * ((P.D + 15) / 16) * PANEL >= 0x7fff0000LL)
            return ECORR_EINVAL;
        if ((stages & 1) && fmap_format != ECORR_ELEM_F32 && fmap_format != ECORR_ELEM_F16 &&
            fmap_format != ECORR_ELEM_BF16)
            return ECORR_EINVAL;
        const SplitWs w = split_ws(P, B);
        P.ex1 = reinterpret_cast<int*>(P.ws);
        P.ex2 = reinterpret_cast<int*>(P.ws + w.ex2);
        P.pk1 = P.ws + w.pk1;
        P.pk2 = P.ws + w.pk2;
        const int nx = 2 * P.n_mt > pack_grid_x(P) ? 2 * P.n_mt : pack_grid_x(P);
        // D = 256: build_split16_kernel and its panel layout; other D: build_split_kernel
        const bool s16 = (P.D + 15) / 16 == 2 * NCP;
        if (stages & 1) {
            if (hi && hipMemsetAsync(P.ws - kHiFlagBytes, 0, 4, stream) != hipSuccess) return hip_status();
            if (fmap_format == ECORR_ELEM_F16) launch_pack<InElem<ECORR_ELEM_F16>::type>(P, nx, B, s16, stream);
            else if (fmap_format == ECORR_ELEM_BF16) launch_pack<InElem<ECORR_ELEM_BF16>::type>(P, nx, B, s16, stream);
            else launch_pack<float>(P, nx, B, s16, stream);
            // hi: the pass is the plain one (its panels byte for byte); the flag comes from its lo halves
            if (hi) launch_lo_flag(P.pk1, w.total - w.pk1, reinterpret_cast<int*>(P.ws - kHiFlagBytes), stream);
        }
        if (!(stages & 2)) return hip_status();
        // hi: the kernel that reads the flag; other D have no one-term form and ignore the flag
        if (s16 && hi) launch_split16_hi(P, ntiles, stream);   // build_hi.hip
        else if (s16) launch_mul(P, ntiles, stream, build_split16_kernel<true>, build_split16_kernel<false>);
        else launch_mul(P, ntiles, stream, build_split_kernel<true>, build_split_kernel<false>);
    } else {
        // D = 256 with 4-aligned rows and 31-bit operand offsets: the 256 x 128 fp32 kernel
        if (P.D == 256 && P.W % 4 == 0 && (uintptr_t)P.f2 % 16 == 0 && fits_buffer_range(P)) {
            const int64_t nt2 = (int64_t)B * P.n_qt * P.n_nt;
            if (nt2 <= 0 || nt2 > 0x7fffffff) return ECORR_EINVAL;
            launch_mul(P, nt2, stream, build_f32_kernel<true>, build_f32_kernel<false>);
        } else {   // any D: the 128 x 128 fp32 kernel
            const int64_t ntiles = (int64_t)B * P.n_mt * P.n_nt;
            if (ntiles <= 0 || ntiles > 0x7fffffff) return ECORR_EINVAL;
            const bool vec = (P.W % 4 == 0) && (P.q_count % 4 == 0) && ((uintptr_t)P.f1 % 16 == 0) &&
                             ((uintptr_t)P.f2 % 16 == 0);
            // LDS-DMA staging whenever both operands' byte offsets fit the 31-bit buffer range
            const bool glds = vec && fits_buffer_range(P);
            const dim3 grid((unsigned)ntiles), block(NT);
            if (glds) hipLaunchKernelGGL((build_kernel<true, true>), grid, block, 0, stream, P);
            else if (vec) hipLaunchKernelGGL((build_kernel<true, false>), grid, block, 0, stream, P);
            else hipLaunchKernelGGL((build_kernel<false, false>), grid, block, 0, stream, P);
        }
    }
    int st = hip_status();
    const int64_t rows = (int64_t)B * P.q_count;
    for (int i = 4; i < levels && st == ECORR_OK; ++i) {
        const int64_t n = rows * g.h[i] * g.w[i];
        const int grid = (int)((n + 255) / 256 < 4096 ? (n + 255) / 256 : 4096);
        hipLaunchKernelGGL(pool2_kernel, dim3(grid), dim3(256), 0, stream, pyramid + g.off[i - 1], pyramid + g.off[i],
                           rows, g.h[i - 1], g.w[i - 1], i - 1, g.ntx[i - 1], g.sz[i - 1], g.ntx[i], g.sz[i]);
        st = hip_status();
    }
    return st;
}

}  // namespace ecorr
