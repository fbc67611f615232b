// motion_enc.hip -- the rest of BasicMotionEncoder (update.py:68-81) behind convc1, on fp32 NCHW tensors:
//
//   cor = relu(convc2(c1))     3x3, 256 -> 192        f1  = relu(convf1(flow))   7x7, 2 -> 128
//   flo = relu(convf2(f1))     3x3, 128 -> 64         out = [relu(conv([cor, flo])), flow]   3x3, 256 -> 126, + 2
//
// c1 = relu(convc1(corr)) [B][256][H W] comes from motion.hip (or torch); out [B][128][H W] with a caller's
// batch stride, so that it can be the upper half of the GRU's x -- neither torch.cat runs.
//
// A 3x3 convolution over NCHW is nine 1x1 convolutions on shifted pixels: a GEMM over K = 9 taps x C channels
// whose B operand is read in place.  menc_gemm_kernel<M, C0, C1, FLOW> is gru.hip's gru_gemm_kernel with nine
// 2-D taps: v_mfma_f32_32x32x2_f32 on exact fp32 operands, a wave owns 32 pixels x RBW row blocks of 32,
// weights pre-laid-out per (tap, 16-channel chunk) and double-buffered through LDS one chunk ahead, B values one
// dword per lane and k-step straight from global through range-checked buffer resources, one chunk ahead.  K is
// tap-major (kc = NC t + c, t = 3 ky + kx); chunk c reads channels 16 c .. 16 c + 15 of in0 (c < C0 / 16) or of
// in1 -- conv's [cor | flo] split falls on the chunk edge 192 / 16 = 12, wave-uniform.  Chains of 12 chunks
// (192 products) are summed in a second accumulator: 12 chains for K = 2304, 6 for K = 1152.
//
//   convc2   M = 192, 64 pixels per workgroup:  2 pixel blocks x 2 row groups of 3 row blocks
//   convf2   M = 64, 128 pixels per workgroup:  4 pixel blocks x 2 row blocks
//   conv     M = 128, 128 pixels per workgroup: 4 pixel blocks x 4 row blocks; rows 126 and 127 have zero
//            weights, their accumulators are dropped and out's channels 126, 127 are flow's bits
//
//   borders  every lane has a two-sided predicate per tap: px + dx in [0, W) and py + dy in [0, H); an invalid
//            lane's offset is steered past the buffer range so it reads 0.  The range check alone is not the
//            zero padding: p +- 1 of a row end is the neighbouring row, p - W of row 0 the previous channel's
//            last row, all in range (gru.hip).
//   relu     v < 0 ? 0 : v (conv.hip): a NaN stays a NaN, as in torch.relu; fmaxf would drop it.
//
// convf1 (K = 98, 1.5 % of the flops) is a VALU kernel: a lane holds its pixel's 98 taps in registers, a wave
// walks 32 output channels whose weights ([128][100] in LDS, 50 KB) it reads as broadcast 16-byte pieces, one
// k-ordered fmaf chain per output.  Padding K to the GEMM's chunks (2 channels -> 16) would run 8 times the
// MFMAs for it, and its A operand would not fit the (tap, 16-channel) pack.
// Four launches (convf1, convc2, convf2, conv), grid z = batch item.  No atomics: two runs give the same bits.

#include "ecorr_device.h"
#include "ecorr_internal.h"
#include "mfma_f32_frame.h"
#include "motion_enc_shape.h"

namespace ecorr {

namespace {

struct MencTensors {
    const float* weight[4];   // convc2 [192][256][3][3], convf1 [128][2][7][7], convf2 [64][128][3][3], conv [126][256][3][3]
    const float* bias[4];
};

// A tap-GEMM matrix of M rows over C channels: MET * C / MEKC chunks (tap-major) of M * MEKC floats,
//   [row block rb][k quad kq][lane l][j] = W[row 32 rb + (l & 31)][channel 16 c + 8 kq + 2 j + (l >> 5)][tap t]
// (gru.hip's order); rows past `rows` are 0.
__device__ __forceinline__ float menc_packed_at(const float* __restrict__ wt, int M, int rows, int C, int r) {
    const int chf = M * MEKC;
    const int kc = r / chf, e = r % chf;
    const int j = e & 3, l = (e >> 2) & 63, kq = (e >> 8) & 1, rb = e >> 9;
    const int nc = C / MEKC, t = kc / nc, c = kc % nc;
    const int row = 32 * rb + (l & 31), ch = MEKC * c + 8 * kq + 2 * j + (l >> 5);
    return row < rows ? wt[((int64_t)row * C + ch) * MET + t] : 0.0f;
}

__global__ __launch_bounds__(MENT) void menc_pack_kernel(MencTensors T, float* __restrict__ packed) {
    for (int64_t i = (int64_t)blockIdx.x * MENT + threadIdx.x; i < kMePackFloats; i += (int64_t)gridDim.x * MENT) {
        float v;
        if (i < kMeF2At) {
            v = menc_packed_at(T.weight[0], MECOR, MECOR, MEC1, (int)(i - kMeC2At));
        } else if (i < kMeCvAt) {
            v = menc_packed_at(T.weight[2], MEFLO, MEFLO, MEF1, (int)(i - kMeF2At));
        } else if (i < kMeF1At) {
            v = menc_packed_at(T.weight[3], MEOUT, MECONV, MECOR + MEFLO, (int)(i - kMeCvAt));
        } else if (i < kMeBiasAt) {   // convf1: [o][k = (7 c + ky) 7 + kx] as stored, rows padded to 100
            const int r = (int)(i - kMeF1At), o = r / MEF1LD, k = r % MEF1LD;
            v = k < MEF1K ? T.weight[1][o * MEF1K + k] : 0.0f;
        } else {
            const int k = (int)(i - kMeBiasAt);
            if (k < kMeBiasF1) v = T.bias[0][k];
            else if (k < kMeBiasF2) v = T.bias[1][k - kMeBiasF1];
            else if (k < kMeBiasCv) v = T.bias[2][k - kMeBiasF2];
            else v = k - kMeBiasCv < MECONV ? T.bias[3][k - kMeBiasCv] : 0.0f;
        }
        packed[i] = v;
    }
}

__device__ __forceinline__ float menc_relu(float v) { return v < 0.0f ? 0.0f : v; }

// f1 = relu(convf1(flow)): flow [B][2][H W] -> f1 [B][128][H W].  64 pixels per workgroup (lane = pixel), wave w
// the output channels 32 w .. 32 w + 31; wf = the packed [128][100] rows.
__global__ __launch_bounds__(MENT) void menc_convf1_kernel(const float* __restrict__ flow, const float* __restrict__ wf,
                                                         const float* __restrict__ bias, int H, int W,
                                                         float* __restrict__ f1) {
    __shared__ __attribute__((aligned(16))) float ws[MEF1 * MEF1LD];
    const int tid = threadIdx.x, lane = tid & 63, w = tid >> 6;
    const int HW = H * W, b = blockIdx.z;
    for (int i = tid; i < MEF1 * MEF1LD / 4; i += MENT)
        reinterpret_cast<f32x4*>(ws)[i] = reinterpret_cast<const f32x4*>(wf)[i];
    const int p = blockIdx.x * 64 + lane;
    const bool pok = p < HW;
    const int py = p / W, px = p - py * W;
    const float* fb = flow + (int64_t)b * 2 * HW;
    float v[MEF1K];
#pragma unroll
    for (int c = 0; c < 2; ++c)
#pragma unroll
        for (int ky = 0; ky < 7; ++ky)
#pragma unroll
            for (int kx = 0; kx < 7; ++kx) {
                const int dy = ky - MEF1R, dx = kx - MEF1R;
                const bool ok = pok && (unsigned)(px + dx) < (unsigned)W && (unsigned)(py + dy) < (unsigned)H;
                v[(c * 7 + ky) * 7 + kx] = ok ? fb[c * HW + p + dy * W + dx] : 0.0f;
            }
    __syncthreads();
    if (!pok) return;
    float* ob = f1 + (int64_t)b * MEF1 * HW + p;
#pragma unroll 1
    for (int o = 32 * w; o < 32 * w + 32; ++o) {
        const f32x4* wr = reinterpret_cast<const f32x4*>(ws + o * MEF1LD);
        float acc = 0.0f;
#pragma unroll
        for (int q = 0; q < MEF1LD / 4; ++q) {
            const f32x4 wv = wr[q];
#pragma unroll
            for (int j = 0; j < 4; ++j)
                if (4 * q + j < MEF1K) acc = fmaf(wv[j], v[4 * q + j], acc);
        }
        ob[(int64_t)o * HW] = menc_relu(acc + bias[o]);
    }
}

// out[o][p] = relu(bias[o] + sum over taps t and channels c of W[o][c][t] in[c][p shifted by t]), in = [in0 | in1]
// of C0 and C1 channels ([B][C0][H W] and [B][C1][H W]; in1 unused when C1 = 0); out [b] at out + b out_bs,
// [M][H W].  FLOW: rows 126 and 127 are flow's ([B][2][H W]) instead.
// GO (the backward's recompute of conv, launch_menc_recompute): nothing of the result is stored; `flow` is
// grad_out, item b at flow + b out_bs, and out [B][M][H W] gets go = relu'(result) grad_out on rows 0-125 -- the
// result <= 0 ? 0 : g of torch's threshold_backward: a NaN result passes g -- and 0 on rows 126 and 127.
template <int M, int C0, int C1, bool FLOW, bool GO = false>
__global__ __launch_bounds__(MENT, 2) void menc_gemm_kernel(const float* __restrict__ in0, const float* __restrict__ in1,
                                                          const float* __restrict__ packed,
                                                          const float* __restrict__ bias, int H, int W,
                                                          const float* __restrict__ flow, float* __restrict__ out,
                                                          int64_t out_bs) {
    constexpr int RBW = M == 192 ? 3 : M / 32;   // row blocks per wave
    constexpr int RG = M / 32 / RBW;             // row groups
    constexpr int PB = 4 / RG;                   // 32-pixel blocks
    constexpr int PT = 32 * PB;                  // pixels per workgroup
    constexpr int NC = (C0 + C1) / MEKC;         // chunks per tap
    constexpr int NK = MET * NC;                 // chunks
    constexpr int CHF = M * MEKC;                // floats per weight chunk
    constexpr int NS = CHF / (4 * MENT);         // 16-byte pieces per thread and chunk
    static_assert(RG * RBW * 32 == M && PB * RG == 4 && NS * 4 * MENT == CHF && NK % MEFL == 0 && C0 % MEKC == 0 &&
                  C1 % MEKC == 0, "tile");
    __shared__ __attribute__((aligned(16))) float wbuf[2][CHF];
    const int tid = threadIdx.x, lane = tid & 63, w = tid >> 6, kh = lane >> 5;
    const int pb = w % PB;   // the wave's 32-pixel block
    const int rg = w / PB;   // and its group of RBW row blocks
    const int HW = H * W, b = blockIdx.z;
    const int p = blockIdx.x * PT + 32 * pb + (lane & 31);
    const bool pok = p < HW;
    const int py = p / W, px = p - py * W;
    const __amdgpu_buffer_rsrc_t rs0 =
        __builtin_amdgcn_make_buffer_rsrc(const_cast<float*>(in0 + (int64_t)b * C0 * HW), 0, C0 * HW * 4, 0x00020000);
    const __amdgpu_buffer_rsrc_t rs1 =
        C1 > 0 ? __builtin_amdgcn_make_buffer_rsrc(const_cast<float*>(in1 + (int64_t)b * C1 * HW), 0, C1 * HW * 4,
                                                   0x00020000)
               : rs0;

    // B operands of chunk kc: in[16 c + 2 ks + kh][pixel (py + dy, px + dx)], ks = 0..7; 0 where the shifted pixel
    // leaves the image on either axis, and for lanes past H W
    auto load_b = [&](int kc, float (&v)[8]) __attribute__((always_inline)) {
        const int t = kc / NC, c = kc - t * NC;
        const int ty = t / 3, dy = ty - 1, dx = t - 3 * ty - 1;
        const bool ok = pok && (unsigned)(px + dx) < (unsigned)W && (unsigned)(py + dy) < (unsigned)H;
        const int pix = p + dy * W + dx;
        const bool from0 = C1 == 0 || c < C0 / MEKC;   // wave-uniform
        const int ch = (from0 ? c * MEKC : c * MEKC - C0) + kh;
        // everything in the vector offset: an invalid lane starts at 2^31, past every range (a range is at
        // most 256 H W 4 bytes < 2^31, and the 14 H W 4 bytes added below cannot wrap)
        const unsigned off = ok ? (unsigned)(ch * HW + pix) * 4u : 0x80000000u;
        const __amdgpu_buffer_rsrc_t rs = from0 ? rs0 : rs1;
#pragma unroll
        for (int ks = 0; ks < 8; ++ks)
            v[ks] = __uint_as_float(
                __builtin_amdgcn_raw_buffer_load_b32(rs, (int)(off + (unsigned)(2 * ks * HW) * 4u), 0, 0));
    };
    auto load_w = [&](int kc, f32x4 (&r)[NS]) __attribute__((always_inline)) {
        const f32x4* src = reinterpret_cast<const f32x4*>(packed + (int64_t)kc * CHF);
#pragma unroll
        for (int s = 0; s < NS; ++s) r[s] = src[s * MENT + tid];
    };
    auto store_w = [&](int buf, const f32x4 (&r)[NS]) __attribute__((always_inline)) {
#pragma unroll
        for (int s = 0; s < NS; ++s) reinterpret_cast<f32x4*>(wbuf[buf])[s * MENT + tid] = r[s];
    };

    f32x4 wr[NS];
    float bc[8], bn[8];
    load_w(0, wr);
    load_b(0, bc);
    store_w(0, wr);
    __syncthreads();

    f32x16 acc[RBW], tot[RBW];
#pragma unroll
    for (int i = 0; i < RBW; ++i)
#pragma unroll
        for (int r = 0; r < 16; ++r) acc[i][r] = tot[i][r] = 0.f;

    // chunk kc's 8 RBW MFMAs: its weights from wbuf[kc & 1] (published by the barrier before), B values in bc
    auto compute = [&](int kc) __attribute__((always_inline)) {
        const float* wb = wbuf[kc & 1] + lane * 4;
        f32x4 a[RBW][2];
#pragma unroll
        for (int i = 0; i < RBW; ++i)
#pragma unroll
            for (int kq = 0; kq < 2; ++kq)
                a[i][kq] = *reinterpret_cast<const f32x4*>(wb + ((RBW * rg + i) * 2 + kq) * 256);
#pragma unroll
        for (int ks = 0; ks < 8; ++ks)
#pragma unroll
            for (int i = 0; i < RBW; ++i)
                acc[i] = __builtin_amdgcn_mfma_f32_32x32x2f32(a[i][ks >> 2][ks & 3], bc[ks], acc[i], 0, 0, 0);
    };
    // step kc < NK - 1: chunk kc + 1's weights in flight to registers while chunk kc computes, then written to
    // the other buffer (whose last readers passed the barrier of step kc - 1); its B values likewise
    auto step = [&](int kc) __attribute__((always_inline)) {
        load_w(kc + 1, wr);
        load_b(kc + 1, bn);
        compute(kc);
        store_w((kc + 1) & 1, wr);
        __syncthreads();
#pragma unroll
        for (int ks = 0; ks < 8; ++ks) bc[ks] = bn[ks];
    };
    // a finished chain of MEFL chunks joins the second-level sum
    auto flush = [&]() __attribute__((always_inline)) {
#pragma unroll
        for (int i = 0; i < RBW; ++i) {
            tot[i] += acc[i];
#pragma unroll
            for (int r = 0; r < 16; ++r) acc[i][r] = 0.f;
        }
    };
#pragma unroll 1
    for (int g = 0; g < NK / MEFL - 1; ++g) {
#pragma unroll 2
        for (int k = 0; k < MEFL; ++k) step(g * MEFL + k);
        flush();
    }
#pragma unroll 2
    for (int kc = NK - MEFL; kc < NK - 1; ++kc) step(kc);
    compute(NK - 1);   // the last chunk: nothing left to fetch, no barrier
    flush();

    // ---- epilogue: lane holds pixel p, rows 32 rb + mfma_c_row(r, kh)
    if (!pok) return;
    if constexpr (GO) {
        const float* gb = flow + (int64_t)b * out_bs + p;
        float* gob = out + (int64_t)b * M * HW + p;
#pragma unroll
        for (int i = 0; i < RBW; ++i)
#pragma unroll
            for (int r = 0; r < 16; ++r) {
                const int o = 32 * (RBW * rg + i) + mfma_c_row(r, kh);
                float v = 0.0f;
                if (o < MECONV) {
                    const float y = menc_relu(tot[i][r] + bias[o]);
                    v = y <= 0.0f ? 0.0f : gb[(int64_t)o * HW];
                }
                gob[(int64_t)o * HW] = v;
            }
        return;
    }
    float* ob = out + (int64_t)b * out_bs + p;
#pragma unroll
    for (int i = 0; i < RBW; ++i)
#pragma unroll
        for (int r = 0; r < 16; ++r) {
            const int o = 32 * (RBW * rg + i) + mfma_c_row(r, kh);
            if (FLOW && o >= MECONV)   // the zero rows' sums are dropped: flow, bit for bit
                ob[(int64_t)o * HW] = flow[((int64_t)b * 2 + (o - MECONV)) * HW + p];
            else
                ob[(int64_t)o * HW] = menc_relu(tot[i][r] + bias[o]);
        }
}

}  // namespace

bool menc_geometry_ok(int B, int H, int W) {
    if (B <= 0 || H <= 0 || W <= 0 || B > 65535) return false;
    // 32-bit buffer offsets (and int pixel arithmetic) within one batch item of the widest tensor, c1; the batch
    // offsets are 64-bit
    return (int64_t)MEC1 * H * W * 4 <= 0x7fffffffLL;
}

int64_t menc_packed_bytes() { return kMePackFloats * 4; }

int64_t menc_workspace_bytes(int B, int H, int W) { return (int64_t)(MECOR + MEF1 + MEFLO) * B * H * W * 4; }

int launch_menc_pack(const float* const weight[4], const float* const bias[4], void* packed, hipStream_t stream) {
    MencTensors T;
    for (int i = 0; i < 4; ++i) {
        T.weight[i] = weight[i];
        T.bias[i] = bias[i];
    }
    hipLaunchKernelGGL(menc_pack_kernel, dim3(512), dim3(MENT), 0, stream, T, (float*)packed);
    return hip_status();
}

int launch_menc(const float* c1, const float* flow, int B, int H, int W, const void* packed, float* out,
                int64_t out_batch_stride, void* workspace, hipStream_t stream) {
    if (!menc_geometry_ok(B, H, W)) return ECORR_EINVAL;
    const int HW = H * W;
    float* cor = (float*)workspace;
    float* f1 = cor + (int64_t)B * MECOR * HW;
    float* flo = f1 + (int64_t)B * MEF1 * HW;
    const float* pk = (const float*)packed;
    const float* bs = pk + kMeBiasAt;
    const dim3 g64((unsigned)((HW + 63) / 64), 1, (unsigned)B), g128((unsigned)((HW + 127) / 128), 1, (unsigned)B);
    hipLaunchKernelGGL(menc_convf1_kernel, g64, dim3(MENT), 0, stream, flow, pk + kMeF1At, bs + kMeBiasF1, H, W, f1);
    hipLaunchKernelGGL((menc_gemm_kernel<MECOR, MEC1, 0, false>), g64, dim3(MENT), 0, stream, c1, nullptr,
                       pk + kMeC2At, bs + kMeBiasC2, H, W, nullptr, cor, (int64_t)MECOR * HW);
    hipLaunchKernelGGL((menc_gemm_kernel<MEFLO, MEF1, 0, false>), g128, dim3(MENT), 0, stream, f1, nullptr,
                       pk + kMeF2At, bs + kMeBiasF2, H, W, nullptr, flo, (int64_t)MEFLO * HW);
    hipLaunchKernelGGL((menc_gemm_kernel<MEOUT, MECOR, MEFLO, true>), g128, dim3(MENT), 0, stream, cor, flo,
                       pk + kMeCvAt, bs + kMeBiasCv, H, W, flow, out, out_batch_stride);
    return hip_status();
}

// The backward's recompute (motion_enc_grad.hip): launch_menc's first three launches into cor, f1 and flo, then
// conv's GEMM with the GO epilogue: go [B][128][H W] from grad_out (item b at grad_out + b grad_out_bs); conv's
// own result is never stored.
int launch_menc_recompute(const float* c1, const float* flow, const float* grad_out, int64_t grad_out_bs, int B, int H,
                          int W, const void* packed, float* cor, float* f1, float* flo, float* go, hipStream_t stream) {
    if (!menc_geometry_ok(B, H, W)) return ECORR_EINVAL;
    const int HW = H * W;
    const float* pk = (const float*)packed;
    const float* bs = pk + kMeBiasAt;
    const dim3 g64((unsigned)((HW + 63) / 64), 1, (unsigned)B), g128((unsigned)((HW + 127) / 128), 1, (unsigned)B);
    hipLaunchKernelGGL(menc_convf1_kernel, g64, dim3(MENT), 0, stream, flow, pk + kMeF1At, bs + kMeBiasF1, H, W, f1);
    hipLaunchKernelGGL((menc_gemm_kernel<MECOR, MEC1, 0, false>), g64, dim3(MENT), 0, stream, c1, nullptr,
                       pk + kMeC2At, bs + kMeBiasC2, H, W, nullptr, cor, (int64_t)MECOR * HW);
    hipLaunchKernelGGL((menc_gemm_kernel<MEFLO, MEF1, 0, false>), g128, dim3(MENT), 0, stream, f1, nullptr,
                       pk + kMeF2At, bs + kMeBiasF2, H, W, nullptr, flo, (int64_t)MEFLO * HW);
    hipLaunchKernelGGL((menc_gemm_kernel<MEOUT, MECOR, MEFLO, false, true>), g128, dim3(MENT), 0, stream, cor, flo,
                       pk + kMeCvAt, bs + kMeBiasCv, H, W, grad_out, go, grad_out_bs);
    return hip_status();
}

}  // namespace ecorr
