// build_split16.h -- what the split16 kernels share across their two translation units (build.hip:
// build_split16_kernel; build_hi.hip: build_split16_hi_kernel): the K loop's constants and static
// wait counts, the epilogue, and the hi workspace's flag word.  The kernels' body is the fragment
// build_split16_loop.h.
#pragma once
#include "build_tile.h"

namespace ecorr {

namespace {

constexpr int kGM16 = 10;   // build_split16_kernel's group bound (balanced); the other builds: 8

// The flag word of a hi workspace (ecorr_build_split_hi_workspace_size; written by lo_flag_kernel,
// build_hi.hip): kHiFlagBytes in front of the split workspace proper, whose first bytes are fmap1's
// exponents -- so BuildParams and the arguments of every kernel stay what they are.
__device__ __forceinline__ int* hi_flag(const BuildParams& P) {
    return reinterpret_cast<int*>(reinterpret_cast<char*>(P.ex1) - kHiFlagBytes);
}

// wait_vm<n> for an n that is a constant once the loop around the call is unrolled
template <bool LGKM0, int N = 40>
__device__ __forceinline__ void wait_vm_n(int n) {
    if constexpr (N >= 0) {
        if (n == N) wait_vm<N, LGKM0>();
        else wait_vm_n<LGKM0, N - 1>(n);
    }
}


// ============================================================================================
// Split GEMM on v_mfma_f32_16x16x32_f16 (D = 256, the E-RAFT feature width: the default build).
// The same block tile, waves and operand split as build_split_kernel (256 queries x one 128-target
// n-tile, wave w = queries 64 w .. + 63 x all 128 targets, two blocks per CU, lo*hi + hi*lo + hi*hi
// per product), on the 16x16x32 MFMA shape: at the same cycles per FLOP the chip holds a higher
// clock under this load on 16x16x32 than on 32x32x16 (MI355X_MICROARCH.md, DVFS give-back item 7;
// round-2 lab: 1.81 vs 1.49 GHz in the K loop alone, profiles/r02_lab/NOTES.md).
//
// K is consumed in 32-deep chunk pairs (the panel layout of pack_body<., true>): per pair and 16x16
// tile three MFMAs, hi*hi, lo*hi, hi*lo, each over the pair's 32 k -- every fragment is loaded once
// and used twice.  The MFMAs take the fmap2 fragment as A (16 targets x 32 k) and the query
// fragment as B (32 k x 16 queries), so lane l of tile (query group qg, target group tg) holds
// query 16 qg + (l & 15) and targets 16 tg + 4 kb + i, kb = l >> 4, i = 0..3.  The fmap2 panel
// stores the n-tile's targets in split16_target order, which makes a lane's 32 targets of a
// query one 4 x 8 quadrant of the 8 x 16 tile (band: one 4 x 8 block of the 4 x 32 tile) -- one
// level-0 tile line, in line order (value 4 tg + i) -- so levels 1 and 2 pool in-lane and the 8 x 8
// pool of level 3 needs one value from lane l ^ 16.
//
// K loop (8 chunk pairs): the target panel of a pair (16 KB, shared by the 4 waves) goes global ->
// LDS by LDS-DMA (4 pieces per wave) through 4 buffers, two pairs ahead; the wave-private query
// fragments (8 x 16 B per lane and pair) global -> VGPR one pair ahead.  One barrier per pair, in
// the middle of the pair's 8 target groups (after group 5): it publishes the next pair (whose first
// A fragments are then read under the last two groups' MFMAs) and retires every wave's reads of the
// pair before, whose buffer the DMA two pairs ahead then takes.  Every wait is a static vmcnt that
// assumes the source's VMEM issue order (s16_vm_after), fenced by sched_barrier; the CPU test
// tests/test_isa_waits.py replays the emitted order.
// ============================================================================================
constexpr int PANEL16 = 2 * PANEL;              // bytes of one (128-pixel tile, 32-deep chunk pair) panel
constexpr int NCP = 8;                          // chunk pairs at D = 256
constexpr int S16NB = 4;                        // LDS buffers (chunk pairs) of the target panel
constexpr int S16COPIES = PANEL16 / 1024 / 4;   // LDS-DMA pieces per wave and pair (4)
constexpr int S16QL = 8;                        // query fragment loads per wave and pair
constexpr int S16LS = 144;                      // LDS bytes per level-0 line in the epilogue transpose
static_assert(S16NB * PANEL16 <= SLDS && 4 * 2 * 64 * S16LS <= SLDS, "split16 LDS regions");

// VMEM instructions a wave issues after the last piece of t(j) until the wait for t(j) (j >= 1: in
// mid(j - 1)).  Issue order: prologue t(0) .. t(S16NB - 2), q(0); pair c: q(c + 1) (c + 1 < NCP),
// then at its mid barrier (c + 1 < NCP) the wait for t(c + 1) and t(c + S16NB - 1) (< NCP).
// copies = LDS-DMA pieces per wave and pair, ql = query fragment loads per wave and pair: (4, 8) in
// the three-term loop, (2, 4) in the one-term loop (split16_kloop).
constexpr int s16_vm_after(int j, int copies = S16COPIES, int ql = S16QL) {
    int n = 0;
    bool seen = false;
    for (int k = 0; k < S16NB - 1; ++k) {
        if (seen) n += copies;
        if (k == j) seen = true;
    }
    if (j == 0) return n + ql;   // the prologue's wait: t(1) .. t(NB - 2), q(0)
    n += seen ? ql : 0;          // q(0)
    for (int c = 0; c + 1 < NCP; ++c) {
        if (seen) n += ql;       // q(c + 1)
        if (c + 1 == j) return n;   // mid(c)
        const int k = c + S16NB - 1;
        if (k < NCP) {
            if (seen) n += copies;
            if (k == j) seen = true;
        }
    }
    return n;
}
static_assert(S16NB != 4 || S16COPIES != 4 || S16QL != 8 ||
                  (s16_vm_after(0) == 16 && s16_vm_after(1) == 20 && s16_vm_after(2) == 28 &&
                   s16_vm_after(3) == 20 && s16_vm_after(6) == 20 && s16_vm_after(7) == 16),
              "split16 wait counts (hand-checked for 4 buffers, 4 pieces, 8 query loads)");
// one-term loop: t(0): t(1) t(2) q(0); t(1): t(2) q(0) q(1); t(2): q(0) q(1) t(3) q(2); t(3 .. 6):
// q(j - 1) t(j + 1) q(j); t(7): q(6) q(7)
static_assert(S16NB != 4 || (s16_vm_after(0, 2, 4) == 8 && s16_vm_after(1, 2, 4) == 10 && s16_vm_after(2, 2, 4) == 14 &&
                             s16_vm_after(3, 2, 4) == 10 && s16_vm_after(6, 2, 4) == 10 && s16_vm_after(7, 2, 4) == 8),
              "split16 one-term wait counts (hand-checked for 4 buffers, 2 pieces, 4 query loads)");

// Epilogue of build_split16_kernel for one wave: its 64 queries (block-local qw .. qw + 63) x the
// n-tile tc from its accumulators acc[qg][tg]; xw = the wave's two LDS transpose regions (2 x 64
// lines x S16LS bytes), smem = the block's LDS array with the published exponents.  It runs
// beside the partner block's K loop, whose MFMAs hold the SIMD's vector issue half the time, so its VALU count is the cost: every address is 32-bit and hoisted
// out of the query-group loop (the quadrant geometry is the lane's; only the query row changes),
// and the cross-lane steps are v_permlane16/32_swap.
// FULL (a whole 256-query tile whose first query row starts a 64-row group, as every tile of the
// BASELINE configs does): every store's query-row term is wave-uniform, so it rides in the scalar
// soffset and a lane's voffset is one constant per store kind (SOOB where its piece lies outside
// the level) -- no per-store address VALU, compare or select.
template <bool MUL, bool FULL>
__device__ __forceinline__ void split16_epilogue(const BuildParams& P, floatx4 (&acc)[4][8], char* smem, char* const xw,
                                                 int qw, const NTile& tc, int b, int q0, int lane) {
    const int *exq = tile_exq(smem), *ext = tile_ext(smem);
    const float* fst = tile_fst(smem);
    const int qn = lane & 15, kb = lane >> 4;
    const int L = P.fused_levels;
    const int64_t rows0 = (int64_t)b * P.q_count + q0;   // the block's first query image
    const int nq = min(SQ, P.q_count - q0);
    __amdgpu_buffer_rsrc_t rl[4];
    block_levels(P, rows0, nq, rl);
    // level-0 line (tile row, tile col) of quadrant k of the n-tile
    auto line_tr = [&](int k) { return (tc.ty0 >> 2) + (tc.band ? 0 : (k & 1)); };
    auto line_tc = [&](int k) { return (tc.tx0 >> 3) + (tc.band ? k : (k >> 1)); };
    // Level-0 transpose: lane l writes its line (query qn, quadrant kb) as line l of the region;
    // store instruction s then takes lines s + 8 j, j = 0..7 (queries s, s + 8 of every quadrant),
    // lane l piece pc of line s + 8 jl, with (jl, pc) chosen so that each 16-lane group of the
    // ds_read_b128 ({0-3, 12-15, 20-27}, {4-11, 16-19, 28-31}, +32) reads two lines 8 apart: all 64
    // banks (line stride 144 B = 36 dwords, 8 lines = 32 banks).
    int jl, pc;
    {
        const int l = lane & 31;
        const bool g1 = (l >= 4 && l < 12) || (l >= 16 && l < 20) || l >= 28;
        const bool second = g1 ? l >= 12 : l >= 16;
        pc = g1 ? (second ? (l < 20 ? l - 16 : l - 24) : l - 4) : (second ? l - 20 : (l < 4 ? l : l - 8));
        jl = 4 * (lane >> 5) + 2 * (g1 ? 1 : 0) + (second ? 1 : 0);
    }
    const int l0stride = (int)P.lsz[0] * 4;            // bytes per query image
    int l0off;                                          // this lane's piece of line s + 8 jl, query row qw + s (+ lq)
    bool l0ok;
    {
        const int lk = jl >> 1, ltr = line_tr(lk), ltc = line_tc(lk);
        l0ok = ltr < P.lnty[0] && ltc < P.lntx[0];
        l0off = (qw + (jl & 1 ? 8 : 0)) * l0stride + tile_base(ltr, ltc, P.lntx[0]) * 4 + 16 * pc;
    }
    const int l0q = qw + (jl & 1 ? 8 : 0);              // query row of store s = 0 (block-local)
    // Interleaved levels 1-3 (ecorr_device.h): a piece of query row R at byte (rowoff + blkoff) 4 of
    // the block's slab; rowoff = ilv_row_off of rr = R - 64 g0 (a slab is below 2^31 bytes: 32-bit),
    // blkoff = ilv_cell_off of the piece's first pixel (the lane's; -1 = outside the level)
    const int rl0 = (int)(rows0 & (kGroup - 1));          // row-in-group of the block's first query
    auto ilv_blkoff = [&](int lv, int r, int c) {          // level pixel (r, c) -> blkoff, or -1
        if (!ilv_cell_in(r, c, lv, P.lnty[lv], -P.lntx[lv])) return -1;
        return (int)ilv_cell_off(r, c, lv, -P.lntx[lv]);
    };
    // level 1: after the row swap, lane kb holds block row kb & 1 of quadrants kb & ~1 (x) and kb | 1 (y)
    const int b1x = L > 1 ? ilv_blkoff(1, 2 * line_tr(kb & ~1) + (kb & 1), 4 * line_tc(kb & ~1)) : -1;
    const int b1y = L > 1 ? ilv_blkoff(1, 2 * line_tr(kb | 1) + (kb & 1), 4 * line_tc(kb | 1)) : -1;
    // level 2: the quadrant's 1 x 2 pixels at (line_tr, 2 line_tc)
    const int b2 = L > 2 ? ilv_blkoff(2, line_tr(kb), 2 * line_tc(kb)) : -1;
    // level 3 (regular tiles, stored by the kb = 0 lanes): the tile's 1 x 2 at (ty0 / 8, tx0 / 8)
    const int b3 = (L > 3 && !tc.band && kb == 0) ? ilv_blkoff(3, tc.ty0 >> 3, tc.tx0 >> 3) : -1;
    auto rowoff = [&](int lv, int rr) { return (int)ilv_row_off(rr, 0, lv, P.lsz[L > lv ? lv : 0]); };   // rr: row from the slab's first group
    // FULL: lane-constant offsets (query-row term qn of the 16-query group, the lane's piece; FOOB
    // where the piece lies outside the level) plus a wave-uniform term (qg, the store, the wave's
    // 64-row group = its index: rl0 == 0) -- one v_add per store.  The uniform term stays in the
    // voffset, soffset 0 (store_piece, build_tile.h, has the hazard that forbids the soffset).
    constexpr int FOOB = 0x70000000;   // + any uniform term stays beyond every slab, below 2^31
    const int qwu = __builtin_amdgcn_readfirstlane(qw);   // wave-uniform (qw = 64 wave)
    const int v0 = l0ok ? l0off - qw * l0stride : FOOB;   // + (qw + 16 qg + s) l0stride
    const int v1x = b1x >= 0 ? (rowoff(1, qn) + b1x) * 4 : FOOB, v1y = b1y >= 0 ? (rowoff(1, qn) + b1y) * 4 : FOOB;
    const int v2 = b2 >= 0 ? (rowoff(2, qn) + b2) * 4 : FOOB, v3 = b3 >= 0 ? (rowoff(3, qn) + b3) * 4 : FOOB;
    const int grpw = qwu >> 6;   // FULL: the wave's interleaved group (block-relative)
    const bool fast = fast_scale<MUL>(P, exq, ext, qw, lane);   // the scale step: build_tile.h
#pragma unroll
    for (int qg = 0; qg < 4; ++qg) {
        const int ql = qw + 16 * qg;   // block-local first query of the group
        const int nqe = query_exp<MUL>(P, exq, ql + qn);
        // v[tg][i] = quadrant pixel (tg >> 1, 4 (tg & 1) + i) of query ql + qn, quadrant kb
        float v[8][4];
        if (fast) {
            const float sq = exp2i(nqe);
#pragma unroll
            for (int tg = 0; tg < 8; ++tg) scale4_fast<MUL>(P, acc[qg][tg], sq, fst + 16 * tg + 4 * kb, v[tg]);
        } else {
#pragma unroll
            for (int tg = 0; tg < 8; ++tg) scale4_ldexp<MUL>(P, acc[qg][tg], nqe, ext + 16 * tg + 4 * kb, v[tg]);
        }
        // level 0: the line through the region (a wave's LDS accesses are processed in order, so
        // group qg + 2's writes cannot overtake group qg's reads of the same region)
        // (stored straight from the lanes instead -- 16-byte pieces of 64 lines per instruction --
        // the same pyramid took 4.8 ms and wrote 5.4 GB: profiles/r03_lab/r3h_*)
        char* const xr = xw + (qg & 1) * (64 * S16LS);
#pragma unroll
        for (int tg = 0; tg < 8; ++tg)
            *reinterpret_cast<floatx4*>(xr + lane * S16LS + 16 * tg) = floatx4{v[tg][0], v[tg][1], v[tg][2], v[tg][3]};
#pragma unroll
        for (int s = 0; s < 8; ++s) {
            const floatx4 x = *reinterpret_cast<const floatx4*>(xr + (s + 8 * jl) * S16LS + 16 * pc);
            if (FULL) store_piece(rl[0], v0, (qwu + 16 * qg + s) * l0stride, x);
            else store_piece_if(rl[0], l0ok && l0q + 16 * qg + s < nq, l0off + (16 * qg + s) * l0stride, x);
        }
        if (L < 2) continue;
        // this lane's query row in its interleaved group
        const int rr = rl0 + ql + qn;
        const bool qok = ql + qn < nq;
        // level 1: the quadrant's 2 x 4 block, l1[r][c] from quadrant rows 2r, 2r + 1, cols 2c, 2c + 1
        auto q0v = [&](int yy, int xx) { return v[2 * yy + (xx >> 2)][xx & 3]; };
        float l1[2][4];
#pragma unroll
        for (int r = 0; r < 2; ++r)
#pragma unroll
            for (int c = 0; c < 4; ++c)
                l1[r][c] = pool4(q0v(2 * r, 2 * c), q0v(2 * r, 2 * c + 1), q0v(2 * r + 1, 2 * c), q0v(2 * r + 1, 2 * c + 1));
        float l2[2];
        if (L >= 3) {
#pragma unroll
            for (int c = 0; c < 2; ++c) l2[c] = pool4(l1[0][2 * c], l1[0][2 * c + 1], l1[1][2 * c], l1[1][2 * c + 1]);
        }
        // level-1 stores: one swap of 16-lane rows (kb odd rows <-> kb even rows) leaves lane kb with
        // block row kb & 1 of the blocks of quadrants kb & ~1 (x) and kb | 1 (y): per instruction,
        // 16 queries x 32 B contiguous per block, two blocks
        {
            float x[4], y[4];
#pragma unroll
            for (int c = 0; c < 4; ++c) {
                const auto sw = __builtin_amdgcn_permlane16_swap(__float_as_uint(l1[0][c]), __float_as_uint(l1[1][c]), false, false);
                x[c] = __uint_as_float(sw[0]);
                y[c] = __uint_as_float(sw[1]);
            }
            if (FULL) {
                store_piece(rl[1], v1x, rowoff(1, (grpw << 6) + 16 * qg) * 4, floatx4{x[0], x[1], x[2], x[3]});
                store_piece(rl[1], v1y, rowoff(1, (grpw << 6) + 16 * qg) * 4, floatx4{y[0], y[1], y[2], y[3]});
            } else {
                const int base1 = rowoff(1, rr);
                store_piece_if(rl[1], qok && b1x >= 0, (base1 + b1x) * 4, floatx4{x[0], x[1], x[2], x[3]});
                store_piece_if(rl[1], qok && b1y >= 0, (base1 + b1y) * 4, floatx4{y[0], y[1], y[2], y[3]});
            }
        }
        if (L < 3) continue;
        // level 2: 4 lanes x 8 B = one query's 2 x 4 block (band: half of two)
        if (FULL) store_piece(rl[2], v2, rowoff(2, (grpw << 6) + 16 * qg) * 4, floatx2{l2[0], l2[1]});
        else store_piece_if(rl[2], qok && b2 >= 0, (rowoff(2, rr) + b2) * 4, floatx2{l2[0], l2[1]});
        if (L < 4 || tc.band) continue;
        // level 3 (regular tiles): pixel kb >> 1 of the tile's 1 x 2 from the 2 x 2 level-2 pixels of
        // lanes kb (row 0, kb even) and kb + 1 (row 1), brought over by a row swap; lane kb = 0 takes
        // pixel 1 from kb = 2 by a half swap and stores both
        const auto o0 = __builtin_amdgcn_permlane16_swap(__float_as_uint(l2[0]), __float_as_uint(l2[0]), false, false);
        const auto o1 = __builtin_amdgcn_permlane16_swap(__float_as_uint(l2[1]), __float_as_uint(l2[1]), false, false);
        const float p3 = pool4(l2[0], l2[1], __uint_as_float(o0[1]), __uint_as_float(o1[1]));
        const auto p3s = __builtin_amdgcn_permlane32_swap(__float_as_uint(p3), __float_as_uint(p3), false, false);
        if (FULL) store_piece(rl[3], v3, rowoff(3, (grpw << 6) + 16 * qg) * 4, floatx2{p3, __uint_as_float(p3s[1])});
        else store_piece_if(rl[3], qok && b3 >= 0, (rowoff(3, rr) + b3) * 4, floatx2{p3, __uint_as_float(p3s[1])});
    }
}

}  // namespace

}  // namespace ecorr
