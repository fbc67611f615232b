// motion_enc_grad.hip -- the backward of motion_enc.hip (ecorr_motion_encoder_backward; autograd of
// update.py:75-81 behind convc1), fp32, first order.  Given g = dL/dout [B][128][H W] (a caller's batch stride):
//
//   go = relu'(o) g[:126]                      [gcor; gflo] = conv^T(go)       gc2 = relu'(cor) gcor, gf2 = relu'(flo) gflo
//   grad_c1 = convc2^T(gc2)                    gf1 = relu'(f1) convf2^T(gf2)   grad_flow = convf1^T(gf1) + g[126:128]
//   gW[o][c][t] = sum_{b,p} gpre[b][o][p] in[b][c][p + d(t)]  (valid shifted pixels only)     gb[o] = sum_{b,p} gpre[b][o][p]
//       (gpre, in) = (go, [cor | flo]) conv, (gc2, c1) convc2, (gf2, f1) convf2, (gf1, flow) convf1
//
// relu'(y) v = y <= 0 ? 0 : v on the ReLU's output y (torch's threshold_backward: a NaN y passes v).  Only c1 and
// flow come from the forward: launch_menc_recompute (motion_enc.hip) recomputes f1, cor and flo with the forward's
// kernels and pack, and conv's recompute writes go from its epilogue -- o itself is never stored.
//
//   menc_pack_t_kernel        the transposed, tap-flipped pack, once per weight set;
//   menc_dgrad_kernel<KO, MASK>  the data gradient of a 3x3 tap convolution: menc_gemm_kernel's loop (A fragments
//                             from the pack through two LDS buffers, B one dword per lane and k-step from global
//                             one chunk ahead, two-sided border predicates, invalid lanes steered past the buffer
//                             range) on that pack: gin[c][p] = sum_t' sum_o W[o][c][8 - t'] gpre[o][p + d(t')].  128
//                             rows x 128 pixels per workgroup, the row group in blockIdx.y; first-level chains of
//                             192 products (the forward's), summed in a second accumulator.  MASK: the epilogue
//                             multiplies by relu' of the row's forward activation;
//   menc_f1_dgrad_kernel      convf1^T on the VALU: 2 output rows, 49 taps x 128 channels; a wave sums 32 channels
//                             (a chain of 49 products per channel, the 32 added in ascending order), the four waves'
//                             sums are added in ascending order, then g's flow channels;
//   menc_bias_part_kernel, menc_bias_reduce_kernel   gru_grad.hip's scheme: per (batch item, 64-pixel block, channel)
//                             sums by a fixed xor tree, added in ascending order;
//   menc_wgrad_kernel<F1>     per tap an NT GEMM gpre x in^T on the frame of mfma_f32_frame.h, the pixel reduction
//                             split into slabs (gru_grad_slab, grad_slab.h), chains of at most 1024 pixels summed in
//                             a second accumulator.  F1: convf1's 128 x 98, the 98 shifted flow planes as columns;
//   menc_wgrad_reduce_kernel  adds the slab partials in ascending slab order into PyTorch's [o][c][ky][kx] layout.
//
// No atomics, one writer per cell, every summation order a function of the shape: two runs give the same bits, and
// a batch item's data gradients do not depend on B.  Every workspace element is written before it is read.
// Workspace (menc_grad_layout): cor f1 flo (the forward's order) | go | gc2 gf2 ([B][256][H W]) | gf1 | bias
// partials | weight slab partials (one region, the four gradients in turn).

#include "ecorr_device.h"
#include "ecorr_internal.h"
#include "grad_slab.h"
#include "mfma_f32_frame.h"
#include "motion_enc_shape.h"

namespace ecorr {

namespace {

constexpr int WK = kGradWK;
constexpr int BQ = 64;   // bias partials: pixels per workgroup

struct MencGradLayout {
    int nsl, slab;   // slabs per batch item, pixels per slab (a multiple of WK)
    int nqb;         // 64-pixel blocks per batch item
    int64_t px;      // B H W
    int64_t cor, f1, flo, go, gcf, gf1, bpart, wpart, total;   // byte offsets; total bytes
};

int64_t align256(int64_t v) { return (v + 255) & ~(int64_t)255; }

MencGradLayout menc_grad_layout(int B, int H, int W) {
    MencGradLayout L;
    const int HW = H * W;
    gru_grad_slab(B, HW, &L.nsl, &L.slab);
    L.nqb = (HW + BQ - 1) / BQ;
    L.px = (int64_t)B * HW;
    const int64_t n = L.px * 4;
    L.cor = 0;
    L.f1 = L.cor + MECOR * n;
    L.flo = L.f1 + MEF1 * n;
    L.go = L.flo + MEFLO * n;
    L.gcf = L.go + MEOUT * n;
    L.gf1 = L.gcf + (MECOR + MEFLO) * n;
    L.bpart = L.gf1 + MEF1 * n;   // 896 n: a multiple of 256
    L.wpart = L.bpart + align256((int64_t)B * L.nqb * MEGB * 4);
    L.total = L.wpart + (int64_t)B * L.nsl * kMeWPartFloats * 4;
    return L;
}

struct MencWeights {
    const float* weight[4];   // convc2 convf1 convf2 conv
};

// One matrix of the transposed pack: row groups of NK = 9 KO / 16 chunks (tap-major: kc = NC t' + c) of 128 x 16,
//   [row block rb][k quad kq][lane l][j] = W[o = 16 c + 8 kq + 2 j + (l >> 5)][channel 128 g + 32 rb + (l & 31)][tap 8 - t']
// over W [rows_o][C][9]; o past rows_o (conv's two padding rows) is 0.
__device__ __forceinline__ float menc_packed_t_at(const float* __restrict__ wt, int KO, int rows_o, int C, int r) {
    const int nc = KO / MEKC, nk = MET * nc;
    const int g = r / (nk * MEDCH);
    r -= g * nk * MEDCH;
    const int kc = r / MEDCH, e = r % MEDCH;
    const int j = e & 3, l = (e >> 2) & 63, kq = (e >> 8) & 1, rb = e >> 9;
    const int t = kc / nc, c = kc % nc;
    const int o = MEKC * c + 8 * kq + 2 * j + (l >> 5), ch = MEDR * g + 32 * rb + (l & 31);
    return o < rows_o ? wt[((int64_t)o * C + ch) * MET + (MET - 1 - t)] : 0.0f;
}

__global__ __launch_bounds__(MENT) void menc_pack_t_kernel(MencWeights T, float* __restrict__ packed) {
    for (int64_t i = (int64_t)blockIdx.x * MENT + threadIdx.x; i < kMePackTFloats; i += (int64_t)gridDim.x * MENT) {
        float v;
        if (i < kMeTC2At) v = menc_packed_t_at(T.weight[3], MEOUT, MECONV, MECOR + MEFLO, (int)(i - kMeTCvAt));
        else if (i < kMeTF2At) v = menc_packed_t_at(T.weight[0], MECOR, MECOR, MEC1, (int)(i - kMeTC2At));
        else v = menc_packed_t_at(T.weight[2], MEFLO, MEFLO, MEF1, (int)(i - kMeTF2At));
        packed[i] = v;
    }
}

// gin[row][p] = sum over taps t' and channels o < KO of W[o][row][8 - t'] gpre[o][p shifted by t']; gpre item b at
// gpre + b gpre_bs, [KO][H W]; mt: the matrix of the transposed pack; the row group is rg0 + blockIdx.y.
// MASK: gin[row] *= relu' of y[row], y = [y0 | y1] of c0n and c1n channels ([B][c0n][H W], [B][c1n][H W]; the split
// falls on a 32-row block).  out [B][out_ch][H W].
template <int KO, bool MASK>
__global__ __launch_bounds__(MENT, 2) void menc_dgrad_kernel(const float* __restrict__ gpre, int64_t gpre_bs,
                                                           const float* __restrict__ mt, int H, int W, int rg0,
                                                           const float* __restrict__ y0, int c0n,
                                                           const float* __restrict__ y1, int c1n,
                                                           float* __restrict__ out, int out_ch) {
    constexpr int NC = KO / MEKC;            // chunks per tap
    constexpr int NK = MET * NC;             // chunks
    constexpr int PT = 128;                  // pixels per workgroup
    constexpr int NS = MEDCH / (4 * MENT);   // 16-byte pieces per thread and chunk
    static_assert(NK % MEFL == 0 && NS * 4 * MENT == MEDCH, "whole chains");
    __shared__ __attribute__((aligned(16))) float wbuf[2][MEDCH];
    const int tid = threadIdx.x, lane = tid & 63, w = tid >> 6, kh = lane >> 5;
    const int rgp = rg0 + (int)blockIdx.y;
    const int HW = H * W, b = blockIdx.z;
    const int p = blockIdx.x * PT + 32 * w + (lane & 31);
    const bool pok = p < HW;
    const int py = p / W, px = p - py * W;
    const __amdgpu_buffer_rsrc_t rs =
        __builtin_amdgcn_make_buffer_rsrc(const_cast<float*>(gpre + (int64_t)b * gpre_bs), 0, KO * HW * 4, 0x00020000);
    const float* __restrict__ pk = mt + (int64_t)rgp * NK * MEDCH;

    // B operands of chunk kc: gpre[16 c + 2 ks + kh][pixel (py + dy, px + dx)], ks = 0..7; 0 where the shifted pixel
    // leaves the image on either axis, and for lanes past H W (motion_enc.hip's load_b)
    auto load_b = [&](int kc, float (&v)[8]) __attribute__((always_inline)) {
        const int t = kc / NC, c = kc - t * NC;
        const int ty = t / 3, dy = ty - 1, dx = t - 3 * ty - 1;
        const bool ok = pok && (unsigned)(px + dx) < (unsigned)W && (unsigned)(py + dy) < (unsigned)H;
        const int pix = p + dy * W + dx;
        const int ch = c * MEKC + kh;
        // an invalid lane starts at 2^31, past every range (at most 192 H W 4 bytes < 2^31; the 14 H W 4 bytes
        // added below cannot wrap)
        const unsigned off = ok ? (unsigned)(ch * HW + pix) * 4u : 0x80000000u;
#pragma unroll
        for (int ks = 0; ks < 8; ++ks)
            v[ks] = __uint_as_float(
                __builtin_amdgcn_raw_buffer_load_b32(rs, (int)(off + (unsigned)(2 * ks * HW) * 4u), 0, 0));
    };
    auto load_w = [&](int kc, f32x4 (&q)[NS]) __attribute__((always_inline)) {
        const f32x4* src = reinterpret_cast<const f32x4*>(pk + (int64_t)kc * MEDCH);
#pragma unroll
        for (int s = 0; s < NS; ++s) q[s] = src[s * MENT + tid];
    };
    auto store_w = [&](int buf, const f32x4 (&q)[NS]) __attribute__((always_inline)) {
#pragma unroll
        for (int s = 0; s < NS; ++s) reinterpret_cast<f32x4*>(wbuf[buf])[s * MENT + tid] = q[s];
    };

    f32x4 wr[NS];
    float bc[8], bn[8];
    load_w(0, wr);
    load_b(0, bc);
    store_w(0, wr);
    __syncthreads();

    f32x16 acc[4], tot[4];
#pragma unroll
    for (int i = 0; i < 4; ++i)
#pragma unroll
        for (int k = 0; k < 16; ++k) acc[i][k] = tot[i][k] = 0.f;

    auto compute = [&](int kc) __attribute__((always_inline)) {
        const float* wb = wbuf[kc & 1] + lane * 4;
        f32x4 a[4][2];
#pragma unroll
        for (int i = 0; i < 4; ++i)
#pragma unroll
            for (int kq = 0; kq < 2; ++kq) a[i][kq] = *reinterpret_cast<const f32x4*>(wb + (i * 2 + kq) * 256);
#pragma unroll
        for (int ks = 0; ks < 8; ++ks)
#pragma unroll
            for (int i = 0; i < 4; ++i)
                acc[i] = __builtin_amdgcn_mfma_f32_32x32x2f32(a[i][ks >> 2][ks & 3], bc[ks], acc[i], 0, 0, 0);
    };
    // chunk kc + 1 in flight to registers while chunk kc computes, then written to the other buffer (whose last
    // readers passed the barrier of step kc - 1)
    auto step = [&](int kc) __attribute__((always_inline)) {
        load_w(kc + 1, wr);
        load_b(kc + 1, bn);
        compute(kc);
        store_w((kc + 1) & 1, wr);
        __syncthreads();
#pragma unroll
        for (int ks = 0; ks < 8; ++ks) bc[ks] = bn[ks];
    };
    auto flush = [&]() __attribute__((always_inline)) {
#pragma unroll
        for (int i = 0; i < 4; ++i) {
            tot[i] += acc[i];
#pragma unroll
            for (int k = 0; k < 16; ++k) acc[i][k] = 0.f;
        }
    };
#pragma unroll 1
    for (int c = 0; c < NK / MEFL - 1; ++c) {
#pragma unroll 2
        for (int k = 0; k < MEFL; ++k) step(c * MEFL + k);
        flush();
    }
#pragma unroll 2
    for (int kc = NK - MEFL; kc < NK - 1; ++kc) step(kc);
    compute(NK - 1);
    flush();

    // ---- epilogue: lane holds pixel p, rows 128 rgp + 32 i + mfma_c_row(k, kh)
    if (!pok) return;
#pragma unroll
    for (int i = 0; i < 4; ++i) {
        const int r0 = MEDR * rgp + 32 * i;   // the block's first row: wave-uniform
        const float* __restrict__ yb = nullptr;
        if constexpr (MASK)
            yb = r0 < c0n ? y0 + ((int64_t)b * c0n + r0) * HW + p : y1 + ((int64_t)b * c1n + (r0 - c0n)) * HW + p;
        float* __restrict__ ob = out + ((int64_t)b * out_ch + r0) * HW + p;
#pragma unroll
        for (int k = 0; k < 16; ++k) {
            const int row = mfma_c_row(k, kh);
            float v = tot[i][k];
            if constexpr (MASK) v = yb[(int64_t)row * HW] <= 0.0f ? 0.0f : v;
            ob[(int64_t)row * HW] = v;
        }
    }
}

// grad_flow[c][p] = g[126 + c][p] + sum over o < 128 and the 49 taps of Wf1[o][c][ky][kx] gf1[o][p - (ky - 3, kx - 3)]
// (shifted pixels outside the image contribute 0).  64 pixels per workgroup (lane = pixel), wave w the channels
// 32 w .. 32 w + 31; wf: the forward pack's [128][100] rows (k = (7 c + ky) 7 + kx), read as wave-uniform values.
// g item b at g + b g_bs, [128][H W].
__global__ __launch_bounds__(MENT) void menc_f1_dgrad_kernel(const float* __restrict__ gf1, const float* __restrict__ wf,
                                                           const float* __restrict__ g, int64_t g_bs, int H, int W,
                                                           float* __restrict__ grad_flow) {
    __shared__ float part[4][2][64];
    const int tid = threadIdx.x, lane = tid & 63, w = tid >> 6;
    const int HW = H * W, b = blockIdx.z;
    const int p = blockIdx.x * 64 + lane;
    const bool pok = p < HW;
    const int py = p / W, px = p - py * W;
    const float* __restrict__ gb = gf1 + (int64_t)b * MEF1 * HW;
    float s0 = 0.0f, s1 = 0.0f;
#pragma unroll 1
    for (int o = 32 * w; o < 32 * w + 32; ++o) {
        const float* __restrict__ wr = wf + o * MEF1LD;
        const float* __restrict__ go = gb + (int64_t)o * HW;
        float a0 = 0.0f, a1 = 0.0f;
#pragma unroll
        for (int ky = 0; ky < 7; ++ky)
#pragma unroll
            for (int kx = 0; kx < 7; ++kx) {
                const int dy = MEF1R - ky, dx = MEF1R - kx;   // the forward's shift, negated
                const bool ok = pok && (unsigned)(px + dx) < (unsigned)W && (unsigned)(py + dy) < (unsigned)H;
                const float v = ok ? go[p + dy * W + dx] : 0.0f;
                a0 = fmaf(wr[ky * 7 + kx], v, a0);
                a1 = fmaf(wr[49 + ky * 7 + kx], v, a1);
            }
        s0 += a0;
        s1 += a1;
    }
    part[w][0][lane] = s0;
    part[w][1][lane] = s1;
    __syncthreads();
    if (w < 2 && pok) {   // wave c adds the four sums of flow channel c in ascending order, then g's
        const float t = ((part[0][w][lane] + part[1][w][lane]) + part[2][w][lane]) + part[3][w][lane];
        grad_flow[((int64_t)b * 2 + w) * HW + p] = t + g[(int64_t)b * g_bs + (int64_t)(MECONV + w) * HW + p];
    }
}

// bpart[(b nqb + qblk) 512 + coff + o] = the sum of gpre[b][o][64 qblk ..] (a fixed xor tree); gpre item b at
// gpre + b gpre_bs; grid (qblk, O / 16, b)
__global__ __launch_bounds__(MENT) void menc_bias_part_kernel(const float* __restrict__ gpre, int64_t gpre_bs, int HW,
                                                            int coff, float* __restrict__ bpart) {
    const int lane = threadIdx.x & 63, w = threadIdx.x >> 6;
    const int qblk = blockIdx.x, b = blockIdx.z, nqb = gridDim.x;
    const int p = qblk * BQ + lane;
#pragma unroll
    for (int i = 0; i < 4; ++i) {
        const int o = 16 * blockIdx.y + 4 * i + w;   // wave-uniform
        float s = p < HW ? gpre[(int64_t)b * gpre_bs + (int64_t)o * HW + p] : 0.f;
#pragma unroll
        for (int d = 32; d >= 1; d >>= 1) s += __shfl_xor(s, d);
        if (lane == 0) bpart[((int64_t)b * nqb + qblk) * MEGB + coff + o] = s;
    }
}

struct MencBiasOut {
    float* gb[4];   // convc2 [192], convf1 [128], convf2 [64], conv [126]
};

// gb[channel] = its np partials: wave w adds the w-th quarter in ascending order, then the four sums in
// ascending order.  Channels: go's 128 (the last two, conv's padding rows, are dropped) | gc2 | gf2 | gf1.  grid 8.
__global__ __launch_bounds__(MENT) void menc_bias_reduce_kernel(const float* __restrict__ bpart, int64_t np,
                                                              MencBiasOut O) {
    __shared__ float part[4][64];
    const int lane = threadIdx.x & 63, w = threadIdx.x >> 6;
    const int c = blockIdx.x * 64 + lane;
    const int64_t per = (np + 3) / 4, i0 = w * per, i1 = i0 + per < np ? i0 + per : np;
    float s = 0.f;
    for (int64_t i = i0; i < i1; ++i) s += bpart[i * MEGB + c];
    part[w][lane] = s;
    __syncthreads();
    if (w == 0) {
        const float t = ((part[0][lane] + part[1][lane]) + part[2][lane]) + part[3][lane];
        if (c < kMeGbC2) {
            if (c < MECONV) O.gb[3][c] = t;
        } else if (c < kMeGbF2) {
            O.gb[0][c - kMeGbC2] = t;
        } else if (c < kMeGbF1) {
            O.gb[2][c - kMeGbF2] = t;
        } else {
            O.gb[1][c - kMeGbF1] = t;
        }
    }
}

// grid (slab sl = b nsl + s, tap t, 64-column block).  3x3 (F1 false): part[sl][o][c][t] = the slab's sum over its
// pixels p of gpre[b][o][p] in[b][c][p + d(t)], in = [in0 | in1] of C0 and C1 channels (a column block reads one of
// them: C0 is a multiple of 64); F1: one tap block, column j = (7 c + ky) 7 + kx < 98 is flow channel c (in0, C0 = 2)
// shifted by (ky - 3, kx - 3): part[sl][o][j].  On the frame of mfma_f32_frame.h: A = gpre (row o < O, k = p; item b
// at gpre + b gpre_bs), B = the shifted planes (column, k = p), 0 where the shifted pixel leaves the image.  Rows past
// O, columns past 98 and pixels past the slab's end are staged as zeros.
template <bool F1>
__global__ __launch_bounds__(MENT) void menc_wgrad_kernel(const float* __restrict__ gpre, int64_t gpre_bs, int O,
                                                        const float* __restrict__ in0, int C0,
                                                        const float* __restrict__ in1, int C1, int H, int W, int nsl,
                                                        int slab, float* __restrict__ part) {
    __shared__ float ol[kFrameM * kFrameLd];
    __shared__ float tl[kFrameN * kFrameLd];
    const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
    const int HW = H * W;
    const int sl = blockIdx.x, b = sl / nsl, p0 = (sl - b * nsl) * slab, p1 = min(HW, p0 + slab);
    const int t = blockIdx.y, c0 = blockIdx.z * kFrameN;
    const int ty = t / 3, dy3 = ty - 1, dx3 = t - 3 * ty - 1;
    const float* __restrict__ A = gpre + (int64_t)b * gpre_bs;
    const bool low = F1 || c0 < C0;   // workgroup-uniform: the column block reads in0 or in1
    const float* __restrict__ Bm = F1    ? in0 + (int64_t)b * 2 * HW
                                   : low ? in0 + ((int64_t)b * C0 + c0) * HW
                                         : in1 + ((int64_t)b * C1 + (c0 - C0)) * HW;
    const int kl = tid & 31, dr = tid >> 5;   // staging: lane = p, 8 rows per step
    const int nchunks = (p1 - p0 + WK - 1) / WK;

    // F1: column dr + 8 i of the block: its flow plane and shift (a column past 98: never valid)
    int cpl[kFrameN / 8], cdy[kFrameN / 8], cdx[kFrameN / 8];
    if constexpr (F1) {
#pragma unroll
        for (int i = 0; i < kFrameN / 8; ++i) {
            const int j = c0 + dr + 8 * i;
            const int c = j / 49, r = j - 49 * c, ky = r / 7;
            cpl[i] = j < MEF1K ? c : -1;
            cdy[i] = ky - MEF1R;
            cdx[i] = r - 7 * ky - MEF1R;
        }
    }

    floatx16 acc[2][2], tot[2][2];
    ECORR_FRAME_CLEAR(tot)

    float ro[kFrameM / 8], rt[kFrameN / 8];
    int base = 0;
    auto load_chunk = [&](int kc) {
        const int p = p0 + (base + kc) * WK + kl;
        const bool pv = p < p1;
        const int py = p / W, px = p - py * W;
#pragma unroll
        for (int i = 0; i < kFrameM / 8; ++i) {
            const int o = dr + 8 * i;
            ro[i] = (pv && o < O) ? A[(int64_t)o * HW + p] : 0.0f;
        }
        if constexpr (F1) {
#pragma unroll
            for (int i = 0; i < kFrameN / 8; ++i) {
                const bool sv = pv && cpl[i] >= 0 && (unsigned)(px + cdx[i]) < (unsigned)W &&
                                (unsigned)(py + cdy[i]) < (unsigned)H;
                rt[i] = sv ? Bm[(int64_t)cpl[i] * HW + p + cdy[i] * W + cdx[i]] : 0.0f;
            }
        } else {
            const bool sv = pv && (unsigned)(px + dx3) < (unsigned)W && (unsigned)(py + dy3) < (unsigned)H;
            const int ps = p + dy3 * W + dx3;
#pragma unroll
            for (int i = 0; i < kFrameN / 8; ++i) rt[i] = sv ? Bm[(int64_t)(dr + 8 * i) * HW + ps] : 0.0f;
        }
    };
    auto store_chunk = [&]() {
#pragma unroll
        for (int i = 0; i < kFrameM / 8; ++i) ol[(dr + 8 * i) * kFrameLd + kl] = ro[i];
#pragma unroll
        for (int i = 0; i < kFrameN / 8; ++i) tl[(dr + 8 * i) * kFrameLd + kl] = rt[i];
    };

    // chains of at most kGradChain pixels, summed in tot
    for (base = 0; base < nchunks; base += kGradChain / WK) {
        const int nc = min(kGradChain / WK, nchunks - base);
        ECORR_FRAME_CLEAR(acc)
        ECORR_FRAME_K_LOOP(false, nc, ol, tl, lane, wave, acc, load_chunk, store_chunk)
#pragma unroll
        for (int i = 0; i < 2; ++i)
#pragma unroll
            for (int j = 0; j < 2; ++j) tot[i][j] += acc[i][j];
    }

    // epilogue: lane (n, kh) holds column c, rows mfma_c_row(k, kh) of each 32 x 32 tile
    const int C = F1 ? MEF1K : C0 + C1;           // columns of the gradient
    const int64_t TS = F1 ? 1 : MET;              // ... and taps per column
    float* __restrict__ P = part + (int64_t)sl * O * C * TS;
    const int kh = lane >> 5;
#pragma unroll
    for (int j = 0; j < 2; ++j) {
        const int c = c0 + 32 * j + (lane & 31);
        if (c >= C) continue;
#pragma unroll
        for (int i = 0; i < 2; ++i)
#pragma unroll
            for (int k = 0; k < 16; ++k) {
                const int o = mfma_c_row(k, kh, 64 * wave + 32 * i);
                if (o < O) P[((int64_t)o * C + c) * TS + (F1 ? 0 : t)] = tot[i][j][k];
            }
    }
}

// gw[i] = its nslab partials in ascending order
__global__ __launch_bounds__(MENT) void menc_wgrad_reduce_kernel(const float* __restrict__ part, int64_t nslab, int64_t n,
                                                               float* __restrict__ gw) {
    for (int64_t i = (int64_t)blockIdx.x * MENT + threadIdx.x; i < n; i += (int64_t)gridDim.x * MENT) {
        float s = 0.f;
        for (int64_t sl = 0; sl < nslab; ++sl) s += part[sl * n + i];
        gw[i] = s;
    }
}

unsigned grid1d(int64_t n) {
    const int64_t g = (n + MENT - 1) / MENT;
    return (unsigned)(g < 65536 ? g : 65536);
}

}  // namespace

int64_t menc_packed_t_bytes() { return kMePackTFloats * 4; }

int64_t menc_backward_workspace_bytes(int B, int H, int W) { return menc_grad_layout(B, H, W).total; }

int launch_menc_pack_t(const float* const weight[4], void* packed_t, hipStream_t stream) {
    MencWeights T;
    for (int i = 0; i < 4; ++i) T.weight[i] = weight[i];
    hipLaunchKernelGGL(menc_pack_t_kernel, dim3(512), dim3(MENT), 0, stream, T, (float*)packed_t);
    return hip_status();
}

int launch_menc_backward(const float* c1, const float* flow, const float* grad_out, int64_t grad_out_bs, int B, int H,
                         int W, const void* packed, const void* packed_t, float* grad_c1, float* grad_flow,
                         float* const* grad_weight, float* const* grad_bias, void* workspace, hipStream_t stream) {
    if (!menc_geometry_ok(B, H, W)) return ECORR_EINVAL;
    const MencGradLayout L = menc_grad_layout(B, H, W);
    const int HW = H * W;
    char* ws = (char*)workspace;
    float *cor = (float*)(ws + L.cor), *f1 = (float*)(ws + L.f1), *flo = (float*)(ws + L.flo);
    float *go = (float*)(ws + L.go), *gcf = (float*)(ws + L.gcf), *gf1 = (float*)(ws + L.gf1);
    const float* pt = (const float*)packed_t;
    const int64_t sgo = (int64_t)MEOUT * HW, sgcf = (int64_t)(MECOR + MEFLO) * HW, sgf1 = (int64_t)MEF1 * HW;
    const bool want_w = grad_weight != nullptr;
    int st = launch_menc_recompute(c1, flow, grad_out, grad_out_bs, B, H, W, packed, cor, f1, flo, go, stream);
    if (st != ECORR_OK) return st;
    const unsigned npb = (unsigned)((HW + 127) / 128);
    // conv^T -> gc2 | gf2: rows 0-127 feed only grad_c1 and convc2's weights
    const int rg0 = (grad_c1 || want_w) ? 0 : 1;
    hipLaunchKernelGGL((menc_dgrad_kernel<MEOUT, true>), dim3(npb, (unsigned)(2 - rg0), (unsigned)B), dim3(MENT), 0,
                       stream, go, sgo, pt + kMeTCvAt, H, W, rg0, cor, MECOR, flo, MEFLO, gcf, MECOR + MEFLO);
    if (grad_c1)
        hipLaunchKernelGGL((menc_dgrad_kernel<MECOR, false>), dim3(npb, 2, (unsigned)B), dim3(MENT), 0, stream, gcf,
                           sgcf, pt + kMeTC2At, H, W, 0, nullptr, 0, nullptr, 0, grad_c1, MEC1);
    if ((st = hip_status()) != ECORR_OK) return st;
    if (grad_flow || want_w) {
        hipLaunchKernelGGL((menc_dgrad_kernel<MEFLO, true>), dim3(npb, 1, (unsigned)B), dim3(MENT), 0, stream,
                           gcf + (int64_t)MECOR * HW, sgcf, pt + kMeTF2At, H, W, 0, f1, MEF1, nullptr, 0, gf1, MEF1);
        if (grad_flow)
            hipLaunchKernelGGL(menc_f1_dgrad_kernel, dim3((unsigned)((HW + 63) / 64), 1, (unsigned)B), dim3(MENT), 0,
                               stream, gf1, (const float*)packed + kMeF1At, grad_out, grad_out_bs, H, W, grad_flow);
        if ((st = hip_status()) != ECORR_OK) return st;
    }
    if (!want_w) return ECORR_OK;
    float* bpart = (float*)(ws + L.bpart);
    float* wpart = (float*)(ws + L.wpart);
    const dim3 gq((unsigned)L.nqb, 1, (unsigned)B);
    hipLaunchKernelGGL(menc_bias_part_kernel, dim3(gq.x, MEOUT / 16, gq.z), dim3(MENT), 0, stream, go, sgo, HW, kMeGbGo,
                       bpart);
    hipLaunchKernelGGL(menc_bias_part_kernel, dim3(gq.x, (MECOR + MEFLO) / 16, gq.z), dim3(MENT), 0, stream, gcf, sgcf,
                       HW, kMeGbC2, bpart);
    hipLaunchKernelGGL(menc_bias_part_kernel, dim3(gq.x, MEF1 / 16, gq.z), dim3(MENT), 0, stream, gf1, sgf1, HW, kMeGbF1,
                       bpart);
    MencBiasOut BO;
    for (int i = 0; i < 4; ++i) BO.gb[i] = grad_bias[i];
    hipLaunchKernelGGL(menc_bias_reduce_kernel, dim3(MEGB / 64), dim3(MENT), 0, stream, bpart, (int64_t)B * L.nqb, BO);
    if ((st = hip_status()) != ECORR_OK) return st;
    const int64_t nslab = (int64_t)B * L.nsl;
    const unsigned ns = (unsigned)nslab;
    // the four weight gradients in turn through the one partial region (stream order keeps them apart)
    int64_t n = (int64_t)MECONV * (MECOR + MEFLO) * MET;   // conv: go x [cor | flo]
    hipLaunchKernelGGL((menc_wgrad_kernel<false>), dim3(ns, MET, (MECOR + MEFLO) / kFrameN), dim3(MENT), 0, stream, go,
                       sgo, MECONV, cor, MECOR, flo, MEFLO, H, W, L.nsl, L.slab, wpart);
    hipLaunchKernelGGL(menc_wgrad_reduce_kernel, dim3(grid1d(n)), dim3(MENT), 0, stream, wpart, nslab, n, grad_weight[3]);
    n = (int64_t)MECOR * MEC1 * MET;                        // convc2: gc2 x c1
    hipLaunchKernelGGL((menc_wgrad_kernel<false>), dim3(ns, MET, MEC1 / kFrameN), dim3(MENT), 0, stream, gcf, sgcf, MECOR,
                       c1, MEC1, nullptr, 0, H, W, L.nsl, L.slab, wpart);
    hipLaunchKernelGGL(menc_wgrad_reduce_kernel, dim3(grid1d(n)), dim3(MENT), 0, stream, wpart, nslab, n, grad_weight[0]);
    if ((st = hip_status()) != ECORR_OK) return st;
    n = (int64_t)MEFLO * MEF1 * MET;                        // convf2: gf2 x f1
    hipLaunchKernelGGL((menc_wgrad_kernel<false>), dim3(ns, MET, MEF1 / kFrameN), dim3(MENT), 0, stream,
                       gcf + (int64_t)MECOR * HW, sgcf, MEFLO, f1, MEF1, nullptr, 0, H, W, L.nsl, L.slab, wpart);
    hipLaunchKernelGGL(menc_wgrad_reduce_kernel, dim3(grid1d(n)), dim3(MENT), 0, stream, wpart, nslab, n, grad_weight[2]);
    n = (int64_t)MEF1 * MEF1K;                              // convf1: gf1 x the 98 shifted flow planes
    hipLaunchKernelGGL((menc_wgrad_kernel<true>), dim3(ns, 1, (MEF1K + kFrameN - 1) / kFrameN), dim3(MENT), 0, stream,
                       gf1, sgf1, MEF1, flow, 2, nullptr, 0, H, W, L.nsl, L.slab, wpart);
    hipLaunchKernelGGL(menc_wgrad_reduce_kernel, dim3(grid1d(n)), dim3(MENT), 0, stream, wpart, nslab, n, grad_weight[1]);
    return hip_status();
}

}  // namespace ecorr
