// gru.hip -- SepConvGRU (update.py:33-60) on fp32 NCHW tensors, hidden 128, input 256:
//
//   half-step(h, x; z, r, q convs of 5 taps along one axis, zero padding 2):
//     z  = sigmoid(conv_z([h, x]))        r = sigmoid(conv_r([h, x]))
//     q  = tanh(conv_q([r * h, x]))       h' = (1 - z) * h + z * q
//   h1 = half-step along x (1x5 kernels), h_out = half-step(h1) along y (5x1 kernels).
//
// A 1x5 / 5x1 convolution over NCHW is five 1x1 convolutions on shifted pixels, so each gate is a
// GEMM over K = 5 taps x 384 channels whose B operand is read from the two input tensors in place
// (no torch.cat): channels below 128 from h (or r * h), the rest from x, both as range-checked buffer
// resources.  Two launches per half-step (q at a pixel needs r * h at its four neighbours along the
// tap axis, which other workgroups produce), four per GRU:
//
//   gru_gemm_kernel<AXIS, false>  256 output rows (z: 0-127, r: 128-255), 64 pixels per workgroup;
//                                 epilogue: z = sigmoid(acc + bias) and r * h stored;
//   gru_gemm_kernel<AXIS, true>   128 output rows over (r * h, x), 128 pixels per workgroup;
//                                 epilogue: q = tanh(acc + bias), h' = (1 - z) * h + z * q stored.
//
// Products run on v_mfma_f32_32x32x2_f32: exact fp32 operands, no split and therefore no shared
// exponent -- a shifted tap multiplies a different input pixel into the same accumulator, so conv.hip's
// per-pixel exponents cannot be carried over, and without one a NaN stays on its own pixel column
// (the reference's footprint, nothing more).  Every wave owns 32 pixels (the MFMA's N) x 4 row
// blocks of 32 (M): 4 accumulator tiles.  The k-ordered fmaf chain of one accumulator would be 1920
// long; it is cut into 10 chains of 192 (GFL chunks) that are summed in a second accumulator, which
// keeps the rounding error at the blocked-summation level the 1e-5 bar against fp64 assumes.
//
//   weights   pre-laid-out once by gru_pack_kernel in A-fragment order per (tap, 16-channel chunk):
//             [row block][k quad][lane][4 k-steps], 16 KB (8 KB for q) per chunk; a chunk goes global ->
//             registers one chunk ahead (16-byte loads), then to the other of two LDS buffers, one
//             __syncthreads() per chunk; A fragments are ds_read_b128 (4 k-steps per read).
//   inputs    one dword per lane and k-step straight from global, one chunk ahead; the five taps
//             re-read the same lines out of L2 (5 x 384 x 4 B per pixel and launch), which stays far
//             below what the fp32 MFMA consumes (8 dwords per lane against 32 MFMAs of 64 cycles).
//   borders   every lane has its own column (AXIS 0) or row (AXIS 1) predicate per tap; an invalid
//             lane's offset is steered past the buffer range so it reads 0 -- the flattened neighbour
//             p +- 1 of a row end is the next row, and p - W of row 0 is the previous channel's last
//             row, both in range, so the range check alone would not give the zero padding.
// No atomics: two runs give the same bits.
//
// launch_gru_gates is the same four launches with the kernels' SAVE flag, which also stores r and q: the gate
// recompute of the backward (gru_grad.hip), whose h' is the forward's bit for bit.

#include "ecorr_device.h"
#include "ecorr_internal.h"
#include "gru_shape.h"
#include "mfma_f32_frame.h"

namespace ecorr {

namespace {

struct GruTensors {
    const float* weight[6];   // z1 r1 q1 z2 r2 q2, each [128][384][5]
    const float* bias[6];
};

// Packed weights: half-step s at s kHalfFloats: the z|r matrix (M = 256 rows: z then r) then the q
// matrix (M = 128); a matrix is GNK chunks (tap-major: kc = 24 t + c) of M * 16 floats,
//   [row block rb][k quad kq][lane l][j] = W[row 32 rb + (l & 31)][channel 16 c + 8 kq + 2 j + (l >> 5)][tap t]
// -- element j of the 16 bytes lane l reads is its A operand of k-step 4 kq + j.  Then the biases
// [z1 r1 q1 z2 r2 q2][128].
__global__ __launch_bounds__(GNT) void gru_pack_kernel(GruTensors T, float* __restrict__ packed) {
    const int64_t n = kPackFloats + 6 * GH;
    for (int64_t i = (int64_t)blockIdx.x * GNT + threadIdx.x; i < n; i += (int64_t)gridDim.x * GNT) {
        if (i >= kPackFloats) {
            const int k = (int)(i - kPackFloats);
            packed[i] = T.bias[k / GH][k % GH];
            continue;
        }
        const int s = (int)(i / kHalfFloats);
        int r = (int)(i % kHalfFloats);
        const bool isq = r >= kZrFloats;
        if (isq) r -= (int)kZrFloats;
        const int chf = (isq ? GH : 2 * GH) * GKC;   // floats per chunk
        const int kc = r / chf, e = r % chf;
        const int j = e & 3, l = (e >> 2) & 63, kq = (e >> 8) & 1, rb = e >> 9;
        const int t = kc / GNC, c = kc % GNC;
        const int row = 32 * rb + (l & 31), ch = GKC * c + 8 * kq + 2 * j + (l >> 5);
        const int conv = 3 * s + (isq ? 2 : row / GH);
        packed[i] = T.weight[conv][((int64_t)(row % GH) * GC + ch) * GT + t];
    }
}

// ZR (QK = false): in0 = h, outputs out0 = z, out1 = r * h.  Q (QK = true): in0 = r * h, zin = z,
// hprev = h, output out0 = h'.  All of them [B][128][H W]; x [B][256][H W].
// SAVE (the backward's gate recompute, launch_gru_gates): the same arithmetic and the same stores, and the gate
// itself is stored as well -- ZR: r at zin's address (zin is not read there), Q: q at out1.
template <int AXIS, bool QK, bool SAVE = false>
__global__ __launch_bounds__(GNT, 2) void gru_gemm_kernel(const float* __restrict__ in0, const float* __restrict__ x,
                                                       const float* __restrict__ packed,
                                                       const float* __restrict__ bias, int H, int W,
                                                       const float* __restrict__ hprev,
                                                       const float* __restrict__ zin, float* __restrict__ out0,
                                                       float* __restrict__ out1) {
    constexpr int M = QK ? GH : 2 * GH;     // output rows
    constexpr int PT = QK ? 128 : 64;       // pixels per workgroup
    constexpr int CHF = M * GKC;            // floats per weight chunk
    constexpr int NS = CHF / (4 * GNT);     // 16-byte pieces per thread and chunk
    __shared__ __attribute__((aligned(16))) float wbuf[2][CHF];
    const int tid = threadIdx.x, lane = tid & 63, w = tid >> 6, kh = lane >> 5;
    const int pb = QK ? w : (w & 1);        // the wave's 32-pixel block
    const int rg = QK ? 0 : (w >> 1);       // and its group of 4 row blocks
    const int HW = H * W, b = blockIdx.z;
    const int p = blockIdx.x * PT + 32 * pb + (lane & 31);
    const bool pok = p < HW;
    const int py = p / W, px = p - py * W;
    const __amdgpu_buffer_rsrc_t rs0 =
        __builtin_amdgcn_make_buffer_rsrc(const_cast<float*>(in0 + (int64_t)b * GH * HW), 0, GH * HW * 4, 0x00020000);
    const __amdgpu_buffer_rsrc_t rsx =
        __builtin_amdgcn_make_buffer_rsrc(const_cast<float*>(x + (int64_t)b * GX * HW), 0, GX * HW * 4, 0x00020000);

    // B operands of chunk kc: in[16 c + 2 ks + kh][pixel p shifted by tap t - 2 along AXIS], ks = 0..7;
    // 0 where the shifted pixel leaves its row (AXIS 0) or the image (AXIS 1), and for lanes past H W
    auto load_b = [&](int kc, float (&v)[8]) __attribute__((always_inline)) {
        const int t = kc / GNC, c = kc - t * GNC, d = t - 2;
        const bool ok = pok && (AXIS == 0 ? (unsigned)(px + d) < (unsigned)W : (unsigned)(py + d) < (unsigned)H);
        const int pix = p + (AXIS == 0 ? d : d * W);
        const bool from0 = c < GH / GKC;   // wave-uniform
        const int ch = (from0 ? c * GKC : c * GKC - GH) + kh;
        // everything in the vector offset: an invalid lane starts at 2^31, past every range
        // (a range is at most 256 H W 4 bytes < 2^31, and the 14 H W 4 bytes added below cannot wrap)
        const unsigned off = ok ? (unsigned)(ch * HW + pix) * 4u : 0x80000000u;
        const __amdgpu_buffer_rsrc_t rs = from0 ? rs0 : rsx;
#pragma unroll
        for (int ks = 0; ks < 8; ++ks)
            v[ks] = __uint_as_float(
                __builtin_amdgcn_raw_buffer_load_b32(rs, (int)(off + (unsigned)(2 * ks * HW) * 4u), 0, 0));
    };
    auto load_w = [&](int kc, f32x4 (&r)[NS]) __attribute__((always_inline)) {
        const f32x4* src = reinterpret_cast<const f32x4*>(packed + (int64_t)kc * CHF);
#pragma unroll
        for (int s = 0; s < NS; ++s) r[s] = src[s * GNT + tid];
    };
    auto store_w = [&](int buf, const f32x4 (&r)[NS]) __attribute__((always_inline)) {
#pragma unroll
        for (int s = 0; s < NS; ++s) reinterpret_cast<f32x4*>(wbuf[buf])[s * GNT + tid] = r[s];
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
        for (int r = 0; r < 16; ++r) acc[i][r] = tot[i][r] = 0.f;

    // chunk kc's 32 MFMAs: its weights from wbuf[kc & 1] (published by the barrier before), B values in bc
    auto compute = [&](int kc) __attribute__((always_inline)) {
        const float* wb = wbuf[kc & 1] + lane * 4;
        f32x4 a[4][2];
#pragma unroll
        for (int i = 0; i < 4; ++i)
#pragma unroll
            for (int kq = 0; kq < 2; ++kq)
                a[i][kq] = *reinterpret_cast<const f32x4*>(wb + ((4 * rg + i) * 2 + kq) * 256);
#pragma unroll
        for (int ks = 0; ks < 8; ++ks)
#pragma unroll
            for (int i = 0; i < 4; ++i)
                acc[i] = __builtin_amdgcn_mfma_f32_32x32x2f32(a[i][ks >> 2][ks & 3], bc[ks], acc[i], 0, 0, 0);
    };
    // step kc < GNK - 1: chunk kc + 1's weights in flight to registers while chunk kc computes, then written
    // to the other buffer (whose last readers passed the barrier of step kc - 1); its B values likewise one
    // chunk ahead
    auto step = [&](int kc) __attribute__((always_inline)) {
        load_w(kc + 1, wr);
        load_b(kc + 1, bn);
        compute(kc);
        store_w((kc + 1) & 1, wr);
        __syncthreads();
#pragma unroll
        for (int ks = 0; ks < 8; ++ks) bc[ks] = bn[ks];
    };
    // a finished chain of GFL chunks joins the second-level sum
    auto flush = [&]() __attribute__((always_inline)) {
#pragma unroll
        for (int i = 0; i < 4; ++i) {
            tot[i] += acc[i];
#pragma unroll
            for (int r = 0; r < 16; ++r) acc[i][r] = 0.f;
        }
    };
#pragma unroll 1
    for (int g = 0; g < GNK / GFL - 1; ++g) {
#pragma unroll 2
        for (int k = 0; k < GFL; ++k) step(g * GFL + k);
        flush();
    }
#pragma unroll 2
    for (int kc = GNK - GFL; kc < GNK - 1; ++kc) step(kc);
    compute(GNK - 1);   // the last chunk: nothing left to fetch, no barrier
    flush();

    // ---- epilogue: lane holds pixel p, rows 32 rb + mfma_c_row(r, kh)
    if (!pok) return;
    const int64_t ib = (int64_t)b * GH * HW + p;   // (b, channel 0, p) of every [B][128][H W] tensor
#pragma unroll
    for (int i = 0; i < 4; ++i)
#pragma unroll
        for (int r = 0; r < 16; ++r) {
            const int o = 32 * (4 * rg + i) + mfma_c_row(r, kh);
            const float v = tot[i][r] + bias[o];
            if constexpr (QK) {
                const float q = tanhf(v);
                const int64_t at = ib + (int64_t)o * HW;
                const float z = zin[at], hp = hprev[at];
                out0[at] = (1.0f - z) * hp + z * q;
                if constexpr (SAVE) out1[at] = q;
            } else {
                const float s = 1.0f / (1.0f + expf(-v));
                if (rg == 0) {
                    out0[ib + (int64_t)o * HW] = s;
                } else {
                    const int64_t at = ib + (int64_t)(o - GH) * HW;
                    out1[at] = s * hprev[at];
                    if constexpr (SAVE) const_cast<float*>(zin)[at] = s;
                }
            }
        }
}

}  // namespace

bool gru_sizes_ok(int hidden, int input) { return hidden == GH && input == GX; }

bool gru_geometry_ok(int B, int H, int W) {
    if (B <= 0 || H <= 0 || W <= 0 || B > 65535) return false;
    // 32-bit buffer offsets (and int pixel arithmetic) within one batch item; the ABI's limit covers the batch
    return (int64_t)B * GC * H * W * 4 <= 0x7fffffffLL;
}

int64_t gru_packed_bytes() { return (kPackFloats + 6 * GH) * 4; }

int64_t gru_workspace_bytes(int B, int H, int W) { return (int64_t)3 * B * GH * H * W * 4; }

int launch_gru_pack(const float* const weight[6], const float* const bias[6], void* packed, hipStream_t stream) {
    GruTensors T;
    for (int i = 0; i < 6; ++i) {
        T.weight[i] = weight[i];
        T.bias[i] = bias[i];
    }
    hipLaunchKernelGGL(gru_pack_kernel, dim3(1024), dim3(GNT), 0, stream, T, (float*)packed);
    return hip_status();
}

int launch_gru(const float* h, const float* x, int B, int H, int W, const void* packed, float* h_out, void* workspace,
               hipStream_t stream) {
    if (!gru_geometry_ok(B, H, W)) return ECORR_EINVAL;
    const int HW = H * W;
    const int64_t n = (int64_t)B * GH * HW;
    float* h1 = (float*)workspace;
    float* z = h1 + n;
    float* rh = z + n;
    const float* pk = (const float*)packed;
    const float* bs = pk + kPackFloats;
    const dim3 gzr((unsigned)((HW + 63) / 64), 1, (unsigned)B), gq((unsigned)((HW + 127) / 128), 1, (unsigned)B);
    hipLaunchKernelGGL((gru_gemm_kernel<0, false>), gzr, dim3(GNT), 0, stream, h, x, pk, bs, H, W, h, nullptr, z, rh);
    hipLaunchKernelGGL((gru_gemm_kernel<0, true>), gq, dim3(GNT), 0, stream, rh, x, pk + kZrFloats, bs + 2 * GH, H, W,
                       h, z, h1, nullptr);
    hipLaunchKernelGGL((gru_gemm_kernel<1, false>), gzr, dim3(GNT), 0, stream, h1, x, pk + kHalfFloats, bs + 3 * GH, H,
                       W, h1, nullptr, z, rh);
    hipLaunchKernelGGL((gru_gemm_kernel<1, true>), gq, dim3(GNT), 0, stream, rh, x, pk + kHalfFloats + kZrFloats,
                       bs + 5 * GH, H, W, h1, z, h_out, nullptr);
    return hip_status();
}

// The forward again for the backward (gru_grad.hip), every gate kept: g = [h1 z1 r1 q1 z2 r2 q2 h'] and r * h
// (of the half-step under way) in rh, each [B][128][H W].  The launches of launch_gru with SAVE: h' has its bits.
int launch_gru_gates(const float* h, const float* x, int B, int H, int W, const void* packed, float* g, float* rh,
                     hipStream_t stream) {
    if (!gru_geometry_ok(B, H, W)) return ECORR_EINVAL;
    const int HW = H * W;
    const int64_t n = (int64_t)B * GH * HW;
    float *h1 = g, *z1 = g + n, *r1 = g + 2 * n, *q1 = g + 3 * n, *z2 = g + 4 * n, *r2 = g + 5 * n, *q2 = g + 6 * n,
          *ho = g + 7 * n;
    const float* pk = (const float*)packed;
    const float* bs = pk + kPackFloats;
    const dim3 gzr((unsigned)((HW + 63) / 64), 1, (unsigned)B), gq((unsigned)((HW + 127) / 128), 1, (unsigned)B);
    hipLaunchKernelGGL((gru_gemm_kernel<0, false, true>), gzr, dim3(GNT), 0, stream, h, x, pk, bs, H, W, h, r1, z1, rh);
    hipLaunchKernelGGL((gru_gemm_kernel<0, true, true>), gq, dim3(GNT), 0, stream, rh, x, pk + kZrFloats, bs + 2 * GH,
                       H, W, h, z1, h1, q1);
    hipLaunchKernelGGL((gru_gemm_kernel<1, false, true>), gzr, dim3(GNT), 0, stream, h1, x, pk + kHalfFloats,
                       bs + 3 * GH, H, W, h1, r2, z2, rh);
    hipLaunchKernelGGL((gru_gemm_kernel<1, true, true>), gq, dim3(GNT), 0, stream, rh, x,
                       pk + kHalfFloats + kZrFloats, bs + 5 * GH, H, W, h1, z2, ho, q2);
    return hip_status();
}

}  // namespace ecorr
