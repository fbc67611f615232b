// build_split16_loop.h -- the body of the split16 kernels (build_split16_kernel in build.hip, the two
// build_split16_hi_kernel in build_hi.hip): the block's tile, the K loop and the epilogue call.  NOT a
// header: a fragment that each kernel includes as its function body, after
//     constexpr int TERMS = 3 | 1;   // MFMAs per product
// with `P` the kernel's BuildParams argument and MUL its template parameter.  It is text and not a
// __forceinline__ function because hipcc allocates registers and schedules the prologue differently
// through the call (build_split16_kernel must stay the instructions it was: profiles/hi_build/).
// TERMS = 3: hi*hi + lo*hi + hi*lo per product.  TERMS = 1: hi*hi alone, for panels whose lo halves
// are all +-0 -- the same ring, barrier and wait positions on half the traffic: the pair's 8 hi pieces
// of 1 KB (one per 16-target group, at 2048 g of the panel) go global -> LDS two per wave, the wave
// loads its 4 hi query fragments and issues one MFMA per (query group, target group).
    __shared__ __attribute__((aligned(16))) char smem[TILE_LDS];   // ALL its LDS (build_tile.h)

    const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
    int b, qt, nt;
    const NTile tc = block_tile<kGM16, true>(P, P.n_qt, b, qt, nt);
    const int q0 = qt * SQ;
    int eq = 0, et = 0;   // per-pixel exponents: loaded behind the K loop's last static wait

    const int64_t pstride = (int64_t)NCP * PANEL16;   // bytes of one 128-pixel tile's panels
    __amdgpu_buffer_rsrc_t rq, rt;
    panel_rsrc(P, pstride, b, qt, nt, rq, rt);
    // target panel of pair cp: DMA piece c = wave + 4 s of its 16 KB (lane-linear); the pair and
    // piece offsets ride in the scalar soffset, so one VGPR addresses every piece of the loop
    // (one term: piece s = the hi KB of target group wave + 4 s, to the LDS offset it has in the whole panel)
    constexpr int PIECE = TERMS == 3 ? 1024 : 2048;   // bytes from a piece of this wave's to the next wave's
    constexpr int COPIES = TERMS == 3 ? S16COPIES : S16COPIES / 2, QL = TERMS == 3 ? S16QL : S16QL / 2;
    const int tvo = wave * PIECE + lane * 16;
    auto issue = [&](int cp) {
        char* dst = smem + (cp % S16NB) * PANEL16;
#pragma unroll
        for (int s = 0; s < COPIES; ++s)
            __builtin_amdgcn_raw_ptr_buffer_load_lds(rt, (__attribute__((address_space(3))) void*)(dst + (wave + 4 * s) * PIECE),
                                                     16, tvo, cp * PANEL16 + s * 4 * PIECE, 0, 0);
    };

    floatx4 acc[4][8];
    zero_acc<false>(acc);   // in VGPRs (see mfma below)

    // query fragments of the wave's 4 groups (panel wave / 2, 16-query groups 4 (wave & 1) + g), one pair
    struct QF { halfx8 h[4], l[4]; };
    const int qgo = (wave >> 1) * (int)pstride + (wave & 1) * (4 * 2048) + lane * 16;
    auto load_q = [&](int cp, QF& q) {   // (pair, group) offset in the scalar soffset
#pragma unroll
        for (int g = 0; g < 4; ++g) {
            q.h[g] = __builtin_bit_cast(halfx8, __builtin_amdgcn_raw_buffer_load_b128(rq, qgo, cp * PANEL16 + g * 2048, 0));
            if constexpr (TERMS == 3)
                q.l[g] = __builtin_bit_cast(halfx8, __builtin_amdgcn_raw_buffer_load_b128(rq, qgo + 1024, cp * PANEL16 + g * 2048, 0));
        }
    };
    // target fragments of group tg from LDS (lane-linear ds_read_b128, conflict-free)
    struct AF { halfx8 h, l; };
    auto read_a = [&](int cp, int tg, AF& a) {
        const char* p = smem + (cp % S16NB) * PANEL16 + tg * 2048 + lane * 16;
        a.h = *reinterpret_cast<const halfx8*>(p);
        if constexpr (TERMS == 3) a.l = *reinterpret_cast<const halfx8*>(p + 1024);
    };
    // per element and pair: hi*hi, lo*hi, hi*lo.  Inline asm with the accumulator constrained to
    // VGPRs at every MFMA (gfx950's register file is unified: 128 accumulator VGPRs + the loop's
    // ~100 fit the 256 of two waves per SIMD, and the epilogue's VALU then reads them without 128
    // v_accvgpr_read per wave); with
    // the builtin, hipcc renames accumulator tiles between AGPRs and VGPRs inside the loop
    // (v_accvgpr copies, 48 spilled VGPRs).  Its waitcnt pass still covers the fragment operands.
    auto mfma = [&](floatx4& c, const halfx8& a, const halfx8& bq) {
        asm volatile("v_mfma_f32_16x16x32_f16 %0, %1, %2, %0" : "+v"(c) : "v"(a), "v"(bq));
    };
    // order: hh, lh per query group, then hl x4 -- every accumulator sums its three terms in the
    // same order (hh, lh, hl) wherever its queries sit, so a query-row slab build stays bitwise the
    // whole build (test_split_query_slab_matches_whole).  Round-3 A/B (same instructions and sums):
    // hh x4, lh x4, hl x4 605.9 us -> this order 597.7 us.  A Gray walk over the operand pairs
    // (every MFMA changing one operand of the one before) timed 1% faster again but summed the terms
    // in an order that depends on the query group's parity: not kept.
    auto mfma_tg = [&](const AF& a, const QF& q, int tg) {
#pragma unroll
        for (int g = 0; g < 4; ++g) {
            mfma(acc[g][tg], a.h, q.h[g]);
            if constexpr (TERMS == 3) mfma(acc[g][tg], a.l, q.h[g]);
        }
        if constexpr (TERMS == 3) {
#pragma unroll
            for (int g = 0; g < 4; ++g) mfma(acc[g][tg], a.h, q.l[g]);
        }
    };
#define PHASE __builtin_amdgcn_sched_barrier(0)
    QF qs[2];
    AF af[2];
#pragma unroll
    for (int k = 0; k < S16NB - 1; ++k) {
        issue(k);
        PHASE;
    }
    load_q(0, qs[0]);
    PHASE;
    wait_vm_n<true>(s16_vm_after(0, COPIES, QL));   // t(0) landed
    __builtin_amdgcn_s_barrier();
    PHASE;
    read_a(0, 0, af[0]);
    PHASE;
#pragma unroll
    for (int cp = 0; cp < NCP; ++cp) {
        if (cp + 1 < NCP) load_q(cp + 1, qs[(cp + 1) & 1]);
        PHASE;
#pragma unroll
        for (int tg = 0; tg < 8; ++tg) {
            if (tg == 6 && cp + 1 < NCP) {   // mid(cp): publish t(cp + 1), retire the reads of t(cp - 1)
                wait_vm_n<true>(s16_vm_after(cp + 1, COPIES, QL));
                __builtin_amdgcn_s_barrier();
                PHASE;
                if (cp + S16NB - 1 < NCP) issue(cp + S16NB - 1);
                if (cp + 2 == NCP) load_exponents<split16_target>(P, tc, b, q0, tid, eq, et);   // after the last static wait
                PHASE;
            }
            if (tg + 1 < 8) read_a(cp, tg + 1, af[(tg + 1) & 1]);
            else if (cp + 1 < NCP) read_a(cp + 1, 0, af[0]);
            PHASE;
            mfma_tg(af[tg & 1], qs[cp & 1], tg);
            PHASE;
        }
    }
#undef PHASE
    // the last MFMAs' results are read by the epilogue's VALU: the hazard recognizer does not see
    // into the asm, so pad the XDL write -> VALU read distance explicitly
    asm volatile("s_nop 15");
    asm volatile("s_nop 15");
    wait_vm<0, true>();   // the exponents have landed and this wave's reads are done ...
    publish_exponents(smem, tid, eq, et);
    __syncthreads();      // ... in every wave: the panel buffers are the epilogue's scratch
    pin_acc<false>(acc);
    // FULL: a whole query tile starting a 64-row group (block-uniform)
    if (q0 + SQ <= P.q_count && (((int64_t)b * P.q_count + q0) & (kGroup - 1)) == 0)
        split16_epilogue<MUL, true>(P, acc, smem, smem + wave * (2 * 64 * S16LS), wave * 64, tc, b, q0, lane);
    else
        split16_epilogue<MUL, false>(P, acc, smem, smem + wave * (2 * 64 * S16LS), wave * 64, tc, b, q0, lane);
