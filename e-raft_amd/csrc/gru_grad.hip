// gru_grad.hip -- the backward of gru.hip's SepConvGRU (ecorr_sepconv_gru_backward; autograd of
// update.py:33-60), fp32, hidden 128 / input 256.  One half-step along axis a, given g = dL/dh':
//
//   gq = g z (1 - q^2)                      gz = g (q - h) z (1 - z)
//   [g_rh; gx_q]   = conv_q^T(gq)           gr = g_rh h r (1 - r)
//   [gh_zr; gx_zr] = conv_zr^T([gz; gr])
//   dh = g (1 - z) + g_rh r + gh_zr         dx = gx_q + gx_zr
//   gW[o][c][t] = sum_{b,p} gpre[b][o][p] in[b][c][p + (t - 2) e_a]  (valid shifted pixels only)
//   gb[o]       = sum_{b,p} gpre[b][o][p]     gpre = gz | gr | gq,  in = [h, x] (z, r) or [r h, x] (q)
//
// The y half-step runs first (g = grad_out, h = h1), then the x half-step (g = the first's dh); dx sums both.
// Only h and x come from the forward: launch_gru_gates (gru.hip) recomputes h1 and the six gates with the
// forward's own kernels.
//
//   gru_gate_grad_kernel     gq and gz, elementwise;
//   gru_dgrad_kernel<A, Q>   the data gradient of a gate convolution: the forward's GEMM loop (gru.hip: A fragments
//                            from a pre-laid-out pack through two LDS buffers, B one dword per lane and k-step from
//                            global one chunk ahead, per-lane border predicates, invalid lanes steered past the
//                            buffer range) on the transposed, tap-flipped pack: gin[c][p] = sum_t' sum_o
//                            W[o][c][4 - t'] gpre[o][p + (t' - 2) e_a].  128 input-channel rows x 128 pixels per
//                            workgroup, the row group (h | x low | x high) in blockIdx.y; K = 5 x 128 (q) or
//                            5 x 256 (z|r) in first-level chains of 160 products.  Epilogue, Q: gr and
//                            dh = g (1 - z) + g_rh r (rows 0-127), dx (rows 128-383); ZR: dh += gh_zr, dx += gx_zr;
//   gru_bias_part_kernel     per (batch item, 64-pixel block, channel) sums of gpre (a fixed xor tree),
//   gru_bias_reduce_kernel   added in ascending order;
//   gru_wgrad_kernel<A>      per tap an NT GEMM gpre x in^T on the frame of mfma_f32_frame.h, the pixel
//                            reduction split into slabs (gru_grad_slab: a function of B, H, W alone), chains of
//                            at most 1024 pixels summed in a second accumulator;
//   gru_wgrad_reduce_kernel  adds the slab partials in ascending slab order into PyTorch's [o][c][t] layout.
//
// No atomics, one writer per cell, every summation order a function of the shape: two runs give the same bits.
// Every workspace element is written before it is read.
// Workspace (floats, n = B 128 H W): h1 z1 r1 q1 z2 r2 q2 h' | r h | gq | gz gr ([B][256][H W]) | dh1 |
// bias partials | weight slab partials (gru_grad_layout).

#include "ecorr_device.h"
#include "ecorr_internal.h"
#include "grad_slab.h"   // gru_grad_slab
#include "gru_shape.h"
#include "mfma_f32_frame.h"

namespace ecorr {

namespace {

constexpr int DFL = 10;                  // chunks per first-level chain of the data gradient (160 products)
constexpr int DCH = GH * GKC;            // floats of one (row group, chunk) of the transposed pack
constexpr int kNkZr = GT * 2 * GH / GKC; // chunks of conv_zr^T: K = 5 x 256
constexpr int kNkQ = GT * GH / GKC;      // and of conv_q^T: K = 5 x 128
static_assert(kNkZr % DFL == 0 && kNkQ % DFL == 0 && DFL <= GFL, "whole chains, none longer than the forward's");
constexpr int64_t kZrTFloats = (int64_t)3 * kNkZr * DCH;   // transposed z|r matrix: 384 rows x 5 x 256
constexpr int64_t kQTFloats = (int64_t)3 * kNkQ * DCH;     // transposed q matrix: 384 rows x 5 x 128
constexpr int64_t kHalfTFloats = kZrTFloats + kQTFloats;
constexpr int64_t kPackTFloats = 2 * kHalfTFloats;

constexpr int WK = kGradWK;              // weight gradient: pixels per chunk
constexpr int kChain = kGradChain;       // ... and per first-level chain (grad_slab.h)
constexpr int BQ = 64;                   // bias partials: pixels per workgroup

struct GruGradLayout {
    int nsl, slab;       // slabs per batch item, pixels per slab (a multiple of WK)
    int nqb;             // 64-pixel blocks per batch item
    int64_t n;           // floats of one [B][128][H W] tensor
    int64_t gates, rh, gq, gzr, gh1, bpart, wpart, total;   // byte offsets; total bytes
};

int64_t align256(int64_t v) { return (v + 255) & ~(int64_t)255; }

GruGradLayout gru_grad_layout(int B, int H, int W) {
    GruGradLayout L;
    const int HW = H * W;
    gru_grad_slab(B, HW, &L.nsl, &L.slab);
    L.nqb = (HW + BQ - 1) / BQ;
    L.n = (int64_t)B * GH * HW;
    const int64_t nb = L.n * 4;   // a multiple of 512
    L.gates = 0;
    L.rh = 8 * nb;
    L.gq = 9 * nb;
    L.gzr = 10 * nb;
    L.gh1 = 12 * nb;
    L.bpart = 13 * nb;
    L.wpart = L.bpart + align256((int64_t)B * L.nqb * GC * 4);
    L.total = L.wpart + (int64_t)B * L.nsl * GT * 2 * GH * GC * 4;
    return L;
}

struct GruWeights {
    const float* weight[6];   // z1 r1 q1 z2 r2 q2, each [128][384][5]
};

// The transposed, tap-flipped pack: half-step s at s kHalfTFloats: the z|r matrix (K = 256 rows o per tap: z then
// r) then the q matrix (K = 128); a matrix is 3 row groups (input channels 128 g ..) of NK chunks (tap-major:
// kc = NC t' + c) of 128 x 16 floats,
//   [row block rb][k quad kq][lane l][j] =
//       W[o = 16 c + 8 kq + 2 j + (l >> 5)][channel 128 g + 32 rb + (l & 31)][tap 4 - t']
__global__ __launch_bounds__(GNT) void gru_pack_t_kernel(GruWeights T, float* __restrict__ packed) {
    for (int64_t i = (int64_t)blockIdx.x * GNT + threadIdx.x; i < kPackTFloats; i += (int64_t)gridDim.x * GNT) {
        const int s = (int)(i / kHalfTFloats);
        int r = (int)(i % kHalfTFloats);
        const bool isq = r >= kZrTFloats;
        if (isq) r -= (int)kZrTFloats;
        const int nk = isq ? kNkQ : kNkZr, nc = nk / GT;
        const int g = r / (nk * DCH);
        r -= g * nk * DCH;
        const int kc = r / DCH, e = r % DCH;
        const int j = e & 3, l = (e >> 2) & 63, kq = (e >> 8) & 1, rb = e >> 9;
        const int t = kc / nc, c = kc % nc;
        const int o = GKC * c + 8 * kq + 2 * j + (l >> 5), ch = GH * g + 32 * rb + (l & 31);
        const int conv = 3 * s + (isq ? 2 : o / GH);
        packed[i] = T.weight[conv][((int64_t)(o % GH) * GC + ch) * GT + (GT - 1 - t)];
    }
}

// gq = g z (1 - q^2) -> gq [B][128][H W]; gz = g (q - h) z (1 - z) -> channels 0-127 of gzr [B][256][H W]
__global__ __launch_bounds__(GNT) void gru_gate_grad_kernel(const float* __restrict__ g, const float* __restrict__ z,
                                                            const float* __restrict__ q, const float* __restrict__ h,
                                                            int64_t n, int64_t chw, float* __restrict__ gq,
                                                            float* __restrict__ gzr) {
    for (int64_t i = (int64_t)blockIdx.x * GNT + threadIdx.x; i < n; i += (int64_t)gridDim.x * GNT) {
        const float gv = g[i], zv = z[i], qv = q[i], hv = h[i];
        gq[i] = (gv * zv) * (1.0f - qv * qv);
        gzr[i + (i / chw) * chw] = ((gv * (qv - hv)) * zv) * (1.0f - zv);
    }
}

// QK: gpre = gq [B][128][H W]; rows 0-127: g_rh -> gr (channels 128-255 of gzr) and gh = g (1 - z) + g_rh r (when
// gh is not null); rows 128-383 -> gx (= or +=, gx_add).  ZR: gpre = gzr [B][256][H W]; rows 0-127: gh += ;
// rows 128-383: gx +=.  The row group is rg0 + blockIdx.y; gh, g, hp, z, r [B][128][H W], gx [B][256][H W].
template <int AXIS, bool QK>
__global__ __launch_bounds__(GNT, 2) void gru_dgrad_kernel(const float* __restrict__ gpre,
                                                        const float* __restrict__ packed_t, int H, int W, int rg0,
                                                        const float* __restrict__ g, const float* __restrict__ hp,
                                                        const float* __restrict__ z, const float* __restrict__ r,
                                                        float* __restrict__ gzr, float* __restrict__ gh,
                                                        float* __restrict__ gx, int gx_add) {
    constexpr int KO = QK ? GH : 2 * GH;    // reduction channels per tap
    constexpr int NC = KO / GKC;            // chunks per tap
    constexpr int NK = GT * NC;             // chunks
    constexpr int PT = 128;                 // pixels per workgroup
    constexpr int NS = DCH / (4 * GNT);     // 16-byte pieces per thread and chunk
    __shared__ __attribute__((aligned(16))) float wbuf[2][DCH];
    const int tid = threadIdx.x, lane = tid & 63, w = tid >> 6, kh = lane >> 5;
    const int rgp = rg0 + (int)blockIdx.y;
    const int HW = H * W, b = blockIdx.z;
    const int p = blockIdx.x * PT + 32 * w + (lane & 31);
    const bool pok = p < HW;
    const int py = p / W, px = p - py * W;
    const __amdgpu_buffer_rsrc_t rs =
        __builtin_amdgcn_make_buffer_rsrc(const_cast<float*>(gpre + (int64_t)b * KO * HW), 0, KO * HW * 4, 0x00020000);
    const float* __restrict__ pk = packed_t + (int64_t)rgp * NK * DCH;

    // B operands of chunk kc: gpre[16 c + 2 ks + kh][pixel p shifted by t' - 2 along AXIS]; 0 where the shifted
    // pixel leaves its row (AXIS 0) or the image (AXIS 1), and for lanes past H W (gru.hip's load_b)
    auto load_b = [&](int kc, float (&v)[8]) __attribute__((always_inline)) {
        const int t = kc / NC, c = kc - t * NC, d = t - 2;
        const bool ok = pok && (AXIS == 0 ? (unsigned)(px + d) < (unsigned)W : (unsigned)(py + d) < (unsigned)H);
        const int pix = p + (AXIS == 0 ? d : d * W);
        const int ch = c * GKC + kh;
        // an invalid lane starts at 2^31, past every range (at most 256 H W 4 bytes < 2^31; the 14 H W 4 bytes
        // added below cannot wrap)
        const unsigned off = ok ? (unsigned)(ch * HW + pix) * 4u : 0x80000000u;
#pragma unroll
        for (int ks = 0; ks < 8; ++ks)
            v[ks] = __uint_as_float(
                __builtin_amdgcn_raw_buffer_load_b32(rs, (int)(off + (unsigned)(2 * ks * HW) * 4u), 0, 0));
    };
    auto load_w = [&](int kc, f32x4 (&q)[NS]) __attribute__((always_inline)) {
        const f32x4* src = reinterpret_cast<const f32x4*>(pk + (int64_t)kc * DCH);
#pragma unroll
        for (int s = 0; s < NS; ++s) q[s] = src[s * GNT + tid];
    };
    auto store_w = [&](int buf, const f32x4 (&q)[NS]) __attribute__((always_inline)) {
#pragma unroll
        for (int s = 0; s < NS; ++s) reinterpret_cast<f32x4*>(wbuf[buf])[s * GNT + tid] = q[s];
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
    for (int c = 0; c < NK / DFL - 1; ++c) {
#pragma unroll 2
        for (int k = 0; k < DFL; ++k) step(c * DFL + k);
        flush();
    }
#pragma unroll 1
    for (int kc = NK - DFL; kc < NK - 1; ++kc) step(kc);
    compute(NK - 1);
    flush();

    // ---- epilogue: lane holds pixel p, input-channel rows 128 rgp + 32 i + mfma_c_row(k, kh)
    if (!pok) return;
#pragma unroll
    for (int i = 0; i < 4; ++i)
#pragma unroll
        for (int k = 0; k < 16; ++k) {
            const int row = 32 * i + mfma_c_row(k, kh);
            const float v = tot[i][k];
            if (rgp == 0) {
                const int64_t at = ((int64_t)b * GH + row) * HW + p;
                if constexpr (QK) {
                    const float rv = r[at];
                    gzr[((int64_t)b * 2 * GH + GH + row) * HW + p] = ((v * hp[at]) * rv) * (1.0f - rv);
                    if (gh) gh[at] = g[at] * (1.0f - z[at]) + v * rv;
                } else {
                    gh[at] = gh[at] + v;
                }
            } else {
                const int64_t at = ((int64_t)b * GX + GH * (rgp - 1) + row) * HW + p;
                gx[at] = gx_add ? gx[at] + v : v;
            }
        }
}

// bpart[(b nqb + qblk) 384 + coff + o] = the sum of gpre[b][o][64 qblk ..] (a fixed xor tree); grid (qblk, O / 16, b)
__global__ __launch_bounds__(GNT) void gru_bias_part_kernel(const float* __restrict__ gpre, int O, int HW, int coff,
                                                            float* __restrict__ bpart) {
    const int lane = threadIdx.x & 63, w = threadIdx.x >> 6;
    const int qblk = blockIdx.x, b = blockIdx.z, nqb = gridDim.x;
    const int p = qblk * BQ + lane;
#pragma unroll
    for (int i = 0; i < 4; ++i) {
        const int o = 16 * blockIdx.y + 4 * i + w;   // wave-uniform
        float s = p < HW ? gpre[((int64_t)b * O + o) * HW + p] : 0.f;
#pragma unroll
        for (int d = 32; d >= 1; d >>= 1) s += __shfl_xor(s, d);
        if (lane == 0) bpart[((int64_t)b * nqb + qblk) * GC + coff + o] = s;
    }
}

// gb[channel] = its np partials: wave w adds the w-th quarter in ascending order, then the four sums in
// ascending order.  Channels 0-127 -> gbz, 128-255 -> gbr, 256-383 -> gbq.  grid 6 (64 channels each).
__global__ __launch_bounds__(GNT) void gru_bias_reduce_kernel(const float* __restrict__ bpart, int64_t np,
                                                              float* __restrict__ gbz, float* __restrict__ gbr,
                                                              float* __restrict__ gbq) {
    __shared__ float part[4][64];
    const int lane = threadIdx.x & 63, w = threadIdx.x >> 6;
    const int c = blockIdx.x * 64 + lane;
    const int64_t per = (np + 3) / 4, i0 = w * per, i1 = i0 + per < np ? i0 + per : np;
    float s = 0.f;
    for (int64_t i = i0; i < i1; ++i) s += bpart[i * GC + c];
    part[w][lane] = s;
    __syncthreads();
    if (w == 0) {
        const float t = ((part[0][lane] + part[1][lane]) + part[2][lane]) + part[3][lane];
        float* out = c < GH ? gbz : c < 2 * GH ? gbr : gbq;
        out[c % GH] = t;
    }
}

// grid (slab sl = b nsl + s, tap t, 64-column c block): part[sl][o][c][t] = the slab's sum over its pixels p of
// gpre[b][o][p] in[b][c][p + (t - 2) e_AXIS], on the frame of mfma_f32_frame.h: A = gpre (row o < O, k = p), B = in
// (column c, k = p): c < 128 from in0 (times rmul where given: r h), the rest from x; 0 where the shifted pixel
// leaves its row (AXIS 0) or the image (AXIS 1).  Rows past O and pixels past the slab's end are staged as zeros.
template <int AXIS>
__global__ __launch_bounds__(GNT) void gru_wgrad_kernel(const float* __restrict__ gpre, int O,
                                                        const float* __restrict__ in0, const float* __restrict__ rmul,
                                                        const float* __restrict__ x, int H, int W, int nsl, int slab,
                                                        float* __restrict__ part) {
    __shared__ float ol[kFrameM * kFrameLd];
    __shared__ float tl[kFrameN * kFrameLd];
    const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
    const int HW = H * W;
    const int sl = blockIdx.x, b = sl / nsl, p0 = (sl - b * nsl) * slab, p1 = min(HW, p0 + slab);
    const int t = blockIdx.y, d = t - 2, c0 = blockIdx.z * kFrameN;
    const float* __restrict__ A = gpre + (int64_t)b * O * HW;
    const bool lowc = c0 < GH;   // workgroup-uniform: the column block reads in0 (and rmul) or x
    const float* __restrict__ Bm = lowc ? in0 + ((int64_t)b * GH + c0) * HW : x + ((int64_t)b * GX + c0 - GH) * HW;
    const float* __restrict__ Rm = lowc && rmul ? rmul + ((int64_t)b * GH + c0) * HW : nullptr;
    const int kl = tid & 31, dr = tid >> 5;     // staging: lane = p, 8 rows per step
    const int nchunks = (p1 - p0 + WK - 1) / WK;

    floatx16 acc[2][2], tot[2][2];
    ECORR_FRAME_CLEAR(tot)

    float ro[kFrameM / 8], rt[kFrameN / 8];
    int base = 0;
    auto load_chunk = [&](int kc) {
        const int p = p0 + (base + kc) * WK + kl;
        const bool pv = p < p1;
        const int py = p / W, px = p - py * W;
        const bool sv = pv && (AXIS == 0 ? (unsigned)(px + d) < (unsigned)W : (unsigned)(py + d) < (unsigned)H);
        const int ps = p + (AXIS == 0 ? d : d * W);
#pragma unroll
        for (int i = 0; i < kFrameM / 8; ++i) {
            const int o = dr + 8 * i;
            ro[i] = (pv && o < O) ? A[(int64_t)o * HW + p] : 0.0f;
        }
#pragma unroll
        for (int i = 0; i < kFrameN / 8; ++i) {
            const int64_t at = (int64_t)(dr + 8 * i) * HW + ps;
            float v = sv ? Bm[at] : 0.0f;
            if (Rm && sv) v = Rm[at] * v;   // r h as the forward stores it: one rounding
            rt[i] = v;
        }
    };
    auto store_chunk = [&]() {
#pragma unroll
        for (int i = 0; i < kFrameM / 8; ++i) ol[(dr + 8 * i) * kFrameLd + kl] = ro[i];
#pragma unroll
        for (int i = 0; i < kFrameN / 8; ++i) tl[(dr + 8 * i) * kFrameLd + kl] = rt[i];
    };

    // chains of at most kChain pixels, summed in tot
    for (base = 0; base < nchunks; base += kChain / WK) {
        const int nc = min(kChain / WK, nchunks - base);
        ECORR_FRAME_CLEAR(acc)
        ECORR_FRAME_K_LOOP(false, nc, ol, tl, lane, wave, acc, load_chunk, store_chunk)
#pragma unroll
        for (int i = 0; i < 2; ++i)
#pragma unroll
            for (int j = 0; j < 2; ++j) tot[i][j] += acc[i][j];
    }

    // epilogue: lane (n, kh) holds column c, rows mfma_c_row(k, kh) of each 32 x 32 tile
    float* __restrict__ P = part + (int64_t)sl * O * GC * GT;
    const int kh = lane >> 5;
#pragma unroll
    for (int j = 0; j < 2; ++j) {
        const int c = c0 + 32 * j + (lane & 31);
#pragma unroll
        for (int i = 0; i < 2; ++i)
#pragma unroll
            for (int k = 0; k < 16; ++k) {
                const int o = mfma_c_row(k, kh, 64 * wave + 32 * i);
                if (o < O) P[((int64_t)o * GC + c) * GT + t] = tot[i][j][k];
            }
    }
}

// element i of the first output (i < split) or i - split of the second = its nslab partials in ascending order
__global__ __launch_bounds__(GNT) void gru_wgrad_reduce_kernel(const float* __restrict__ part, int64_t nslab, int64_t n,
                                                               int64_t split, float* __restrict__ gw0,
                                                               float* __restrict__ gw1) {
    for (int64_t i = (int64_t)blockIdx.x * GNT + threadIdx.x; i < n; i += (int64_t)gridDim.x * GNT) {
        float s = 0.f;
        for (int64_t sl = 0; sl < nslab; ++sl) s += part[sl * n + i];
        if (i < split) gw0[i] = s;
        else gw1[i - split] = s;
    }
}

unsigned grid1d(int64_t n) {
    const int64_t g = (n + GNT - 1) / GNT;
    return (unsigned)(g < 65536 ? g : 65536);
}

// One half-step's backward.  g: dL/dh' of the half-step; hp its h; z r q its gates; pt its transposed pack.
// gh: where dh goes (null: not wanted); gx: where dx goes or is added (null: not wanted); gw / gb: the
// half-step's z r q weight and bias gradients (null: not wanted).
template <int AXIS>
int half_backward(const GruGradLayout& L, char* ws, const float* g, const float* hp, const float* x, const float* z,
                  const float* r, const float* q, const float* pt, int B, int H, int W, float* gh, float* gx,
                  int gx_add, float* const* gw, float* const* gb, hipStream_t stream) {
    const int HW = H * W;
    float* gq = (float*)(ws + L.gq);
    float* gzr = (float*)(ws + L.gzr);
    int st;
    hipLaunchKernelGGL(gru_gate_grad_kernel, dim3(grid1d(L.n)), dim3(GNT), 0, stream, g, z, q, hp, L.n,
                       (int64_t)GH * HW, gq, gzr);
    if ((st = hip_status()) != ECORR_OK) return st;
    const unsigned npb = (unsigned)((HW + 127) / 128);
    // conv_q^T: row group 0 always (gr feeds everything else); the x rows when dx is wanted
    hipLaunchKernelGGL((gru_dgrad_kernel<AXIS, true>), dim3(npb, gx ? 3 : 1, (unsigned)B), dim3(GNT), 0, stream, gq,
                       pt + kZrTFloats, H, W, 0, g, hp, z, r, gzr, gh, gx, gx_add);
    if ((st = hip_status()) != ECORR_OK) return st;
    // conv_zr^T: the h rows when dh is wanted, the x rows when dx is
    const int rg0 = gh ? 0 : 1, nrg = (gh ? 1 : 0) + (gx ? 2 : 0);
    if (nrg > 0) {
        hipLaunchKernelGGL((gru_dgrad_kernel<AXIS, false>), dim3(npb, (unsigned)nrg, (unsigned)B), dim3(GNT), 0, stream,
                           gzr, pt, H, W, rg0, nullptr, nullptr, nullptr, nullptr, nullptr, gh, gx, 1);
        if ((st = hip_status()) != ECORR_OK) return st;
    }
    if (!gw) return ECORR_OK;
    float* bpart = (float*)(ws + L.bpart);
    float* wpart = (float*)(ws + L.wpart);
    hipLaunchKernelGGL(gru_bias_part_kernel, dim3((unsigned)L.nqb, 2 * GH / 16, (unsigned)B), dim3(GNT), 0, stream, gzr,
                       2 * GH, HW, 0, bpart);
    hipLaunchKernelGGL(gru_bias_part_kernel, dim3((unsigned)L.nqb, GH / 16, (unsigned)B), dim3(GNT), 0, stream, gq, GH,
                       HW, 2 * GH, bpart);
    hipLaunchKernelGGL(gru_bias_reduce_kernel, dim3(GC / 64), dim3(GNT), 0, stream, bpart, (int64_t)B * L.nqb, gb[0],
                       gb[1], gb[2]);
    if ((st = hip_status()) != ECORR_OK) return st;
    const int64_t nslab = (int64_t)B * L.nsl, nw = (int64_t)GH * GC * GT;
    const dim3 gg((unsigned)nslab, GT, GC / kFrameN);
    hipLaunchKernelGGL((gru_wgrad_kernel<AXIS>), gg, dim3(GNT), 0, stream, gzr, 2 * GH, hp, nullptr, x, H, W, L.nsl,
                       L.slab, wpart);
    hipLaunchKernelGGL(gru_wgrad_reduce_kernel, dim3(grid1d(2 * nw)), dim3(GNT), 0, stream, wpart, nslab, 2 * nw, nw,
                       gw[0], gw[1]);
    if ((st = hip_status()) != ECORR_OK) return st;
    hipLaunchKernelGGL((gru_wgrad_kernel<AXIS>), gg, dim3(GNT), 0, stream, gq, GH, hp, r, x, H, W, L.nsl, L.slab,
                       wpart);
    hipLaunchKernelGGL(gru_wgrad_reduce_kernel, dim3(grid1d(nw)), dim3(GNT), 0, stream, wpart, nslab, nw, nw, gw[2],
                       nullptr);
    return hip_status();
}

}  // namespace

int64_t gru_packed_t_bytes() { return kPackTFloats * 4; }

int64_t gru_backward_workspace_bytes(int B, int H, int W) { return gru_grad_layout(B, H, W).total; }

int launch_gru_pack_t(const float* const weight[6], void* packed_t, hipStream_t stream) {
    GruWeights T;
    for (int i = 0; i < 6; ++i) T.weight[i] = weight[i];
    hipLaunchKernelGGL(gru_pack_t_kernel, dim3(1024), dim3(GNT), 0, stream, T, (float*)packed_t);
    return hip_status();
}

int launch_gru_backward(const float* h, const float* x, const float* grad_out, int B, int H, int W, const void* packed,
                        const void* packed_t, float* grad_h, float* grad_x, float* const* grad_weight,
                        float* const* grad_bias, void* workspace, hipStream_t stream) {
    if (!gru_geometry_ok(B, H, W)) return ECORR_EINVAL;
    const GruGradLayout L = gru_grad_layout(B, H, W);
    char* ws = (char*)workspace;
    float* gates = (float*)(ws + L.gates);
    const float *h1 = gates, *z1 = gates + L.n, *r1 = gates + 2 * L.n, *q1 = gates + 3 * L.n, *z2 = gates + 4 * L.n,
                *r2 = gates + 5 * L.n, *q2 = gates + 6 * L.n;
    float* gh1 = (float*)(ws + L.gh1);
    const float* pt = (const float*)packed_t;
    int st = launch_gru_gates(h, x, B, H, W, packed, gates, (float*)(ws + L.rh), stream);
    if (st != ECORR_OK) return st;
    // the y half-step: its dh is the x half-step's g, always needed
    st = half_backward<1>(L, ws, grad_out, h1, x, z2, r2, q2, pt + kHalfTFloats, B, H, W, gh1, grad_x, 0,
                          grad_weight ? grad_weight + 3 : nullptr, grad_bias ? grad_bias + 3 : nullptr, stream);
    if (st != ECORR_OK) return st;
    return half_backward<0>(L, ws, gh1, h, x, z1, r1, q1, pt, B, H, W, grad_h, grad_x, 1, grad_weight, grad_bias,
                            stream);
}

}  // namespace ecorr
