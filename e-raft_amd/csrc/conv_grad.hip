// conv_grad.hip -- the backward of conv.hip's out[b][o][p] = relu(bias[o] + sum_c W[o][c] in[b][c][p])
// (ecorr_conv1x1_relu_backward; autograd of update.py:67,74), given grad_out and the forward's out:
//
//   gm[b][o][p]       = out[b][o][p] <= 0 ? 0 : grad_out[b][o][p]      (ATen threshold_backward)
//   grad_in[b][c][p]  = sum_o     W[o][c]     gm[b][o][p]
//   grad_weight[o][c] = sum_{b,p} gm[b][o][p] in[b][c][p]
//   grad_bias[o]      = sum_{b,p} gm[b][o][p]
//
//   relu_mask_kernel         one pass over grad_out and out, lane = query as the forward stores them:
//                            writes gm, the per-query partial maxima qmax[B][G][Q] of |gm| over groups
//                            of 32 channels (what conv1x1_split_kernel takes for its column exponents)
//                            and one partial bias sum per (batch item, 64-query block, channel);
//   bias_reduce_kernel       adds those partials in ascending order;
//   grad_in                  conv.hip's split-f16 kernel without its ReLU on gm and the packed
//                            TRANSPOSED weight (launch_conv1x1_split_linear): the mask is materialized
//                            because the conv's K loop counts its loads (no load may be added to it);
//   grad_weight_kernel       an NT GEMM (both operands contiguous along p) on v_mfma_f32_32x32x2_f32,
//                            the frame of grad.hip's build_backward_kernel (mfma_f32_frame.h); split-K: a workgroup
//                            reduces one slab of at most 1024 queries of one batch item (256 .. 1024 by
//                            the shape, conv_grad_layout), so no fp32 accumulator chains more than
//                            1024 terms (a 5000-term chain is 8e-6 .. 1e-5 normwise from fp64, slabs
//                            of 1024 2.6e-6);
//   weight_reduce_kernel     adds the slab partials in ascending slab order.
//
// Deterministic: no atomics, one writer per cell, every summation order a fixed function of the
// shape (never of the device).  Every element of a requested output is overwritten.
// Workspace: gm | qmax | bias partials | weight slab partials (conv_grad_layout).

#include "ecorr_device.h"
#include "ecorr_internal.h"
#include "mfma_f32_frame.h"

namespace ecorr {

namespace {

constexpr int MNT = 256;     // threads of every kernel here but the bias reduce
constexpr int BNT = 1024;    // bias reduce: 16 waves
constexpr int MQ = 64;       // mask pass: queries per workgroup (lane = query)
constexpr int MR = 32;       // mask pass: channels per workgroup = one qmax group
constexpr int WO = kFrameM;  // grad_weight: o rows per workgroup (4 waves x 64)
constexpr int WC = kFrameN;  // grad_weight: c columns per workgroup
constexpr int WK = kFrameK;  // grad_weight: reduction chunk
constexpr int WLD = kFrameLd;   // LDS row stride (floats)
constexpr int kSlabMax = 1024;   // most reduction terms of one fp32 accumulator
constexpr int kSlabMin = 256;    // the slab cap is halved down to this while the grid stays small
constexpr int kSlabGrid = 480;   // ... below this many workgroups (a constant, not a device query)

struct ConvGradLayout {
    int G;            // qmax groups: ceil(O / MR)
    int nqb;          // 64-query blocks per batch item
    int nsl, slab;    // slabs per batch item, queries per slab (a multiple of WK, <= kSlabMax)
    int nsl_max;      // slabs per batch item the workspace has room for (the smallest slab cap)
    int64_t gm, qmax, bpart, wpart, total;   // byte offsets; total bytes
};

int64_t align256(int64_t n) { return (n + 255) & ~(int64_t)255; }

// The status of the geometry (the same for the size query and the call) and the workspace layout.
int conv_grad_layout(int B, int C, int Q, int O, ConvGradLayout* L) {
    if (B < 1 || B > 65535 || C < 1 || Q < 1 || O < 1) return ECORR_EINVAL;
    const int64_t G = ((int64_t)O + MR - 1) / MR;
    if (G > 65535 || ((int64_t)C + WC - 1) / WC > 65535) return ECORR_EINVAL;   // 16-bit grid axes
    // grad_in: the split conv with the roles of C and O swapped (K = O, C output rows)
    if (!conv1x1_split_geometry_ok(B, O, Q, C, (int)G)) return ECORR_EINVAL;
    L->G = (int)G;
    L->nqb = (Q + MQ - 1) / MQ;
    // the slab cap: 1024 queries, halved (to 256 at the least) while the grid would stay below
    // kSlabGrid workgroups -- at DSEC B = 4 a cap of 1024 gives 120 workgroups of 30 chunks; a fixed
    // function of the shape.  Then balanced slabs of whole chunks under the cap.
    const int64_t tiles = (((int64_t)O + WO - 1) / WO) * (((int64_t)C + WC - 1) / WC);
    int cap = kSlabMax;
    while (cap > kSlabMin && (int64_t)B * ((Q + cap - 1) / cap) * tiles < kSlabGrid) cap >>= 1;
    const int n = (Q + cap - 1) / cap;
    L->slab = ((Q + n - 1) / n + WK - 1) / WK * WK;
    L->nsl = (Q + L->slab - 1) / L->slab;
    L->nsl_max = (Q + kSlabMin - 1) / kSlabMin;   // >= nsl for every cap: the size is monotone in B, C, Q, O
    if ((int64_t)B * L->nsl_max > 0x7fffffffLL) return ECORR_EINVAL;
    L->gm = 0;
    L->qmax = L->gm + align256((int64_t)B * O * Q * 4);
    L->bpart = L->qmax + align256((int64_t)B * G * Q * 4);
    L->wpart = L->bpart + align256((int64_t)B * L->nqb * O * 4);
    L->total = L->wpart + align256((int64_t)B * L->nsl_max * O * C * 4);
    return ECORR_OK;
}

// grid (64-query block, 32-channel group g, batch item b); wave w owns the rows w, w + 4, .. of the group
__global__ __launch_bounds__(MNT) void relu_mask_kernel(const float* __restrict__ go, const float* __restrict__ out,
                                                        int O, int Q, float* __restrict__ gm,
                                                        float* __restrict__ qmax, float* __restrict__ bpart) {
    __shared__ float smax[MNT / kWave][MQ];
    const int lane = threadIdx.x & 63, w = threadIdx.x >> 6;
    const int qblk = blockIdx.x, g = blockIdx.y, b = blockIdx.z, nqb = gridDim.x, G = gridDim.y;
    const int q = qblk * MQ + lane;
    const bool qok = q < Q;
    float m = 0.f;
#pragma unroll
    for (int i = 0; i < MR / 4; ++i) {
        const int o = g * MR + w + 4 * i;          // wave-uniform
        const bool ok = qok && o < O;
        const int64_t idx = ((int64_t)b * O + o) * Q + q;
        float v = 0.f;
        if (ok) {
            const float gv = go[idx], ov = out[idx];
            v = ov <= 0.f ? 0.f : gv;               // a NaN out passes the gradient through
            gm[idx] = v;
        }
        m = fmaxf(m, fabsf(v));                     // NaN ignored
        float s = v;                                // the row's 64 queries: a fixed xor tree
#pragma unroll
        for (int d = 32; d >= 1; d >>= 1) s += __shfl_xor(s, d);
        if (lane == 0 && o < O) bpart[((int64_t)b * nqb + qblk) * O + o] = s;
    }
    smax[w][lane] = m;
    __syncthreads();
    if (w == 0 && qok)
        qmax[((int64_t)b * G + g) * Q + q] = fmaxf(fmaxf(smax[0][lane], smax[1][lane]), fmaxf(smax[2][lane], smax[3][lane]));
}

// grad_bias[o] = the np partials of channel o: a workgroup of 16 waves owns 64 channels, wave w adds
// the w-th sixteenth of the partials in ascending order (8 loads in flight: the chain is latency
// bound -- with 4 waves and one load at a time the mask pass + this took 37.8 us at DSEC B = 4 and
// 119.6 us at B = 16, most of it here), then one thread per channel adds the sixteen sums in
// ascending order
__global__ __launch_bounds__(BNT) void bias_reduce_kernel(const float* __restrict__ bpart, int64_t np, int O,
                                                          float* __restrict__ gb) {
    __shared__ float part[BNT / kWave][kWave];
    const int lane = threadIdx.x & 63, w = threadIdx.x >> 6;
    const int o = blockIdx.x * kWave + lane;
    constexpr int NW = BNT / kWave;
    const int64_t per = (np + NW - 1) / NW, i0 = w * per, i1 = i0 + per < np ? i0 + per : np;
    float s = 0.f;
    if (o < O) {
        int64_t i = i0;
        for (; i + 8 <= i1; i += 8) {
            float v[8];
#pragma unroll
            for (int j = 0; j < 8; ++j) v[j] = bpart[(i + j) * O + o];
#pragma unroll
            for (int j = 0; j < 8; ++j) s += v[j];
        }
        for (; i < i1; ++i) s += bpart[i * O + o];
    }
    part[w][lane] = s;
    __syncthreads();
    if (w == 0 && o < O) {
        float t = part[0][lane];
#pragma unroll
        for (int k = 1; k < NW; ++k) t += part[k][lane];
        gb[o] = t;
    }
}

// grid (slab sl = b * nsl + s, 256-row o block, 64-column c block): part[sl][o][c] = the slab's
// sum_p gm[b][o][p] in[b][c][p], on the frame of mfma_f32_frame.h: A = gm (row o, k = p), B = in (column c, k = p).
// Rows past O, columns past C and queries past the slab's end are staged as zeros.
__global__ __launch_bounds__(MNT) void grad_weight_kernel(const float* __restrict__ gm, const float* __restrict__ in,
                                                          int O, int C, int Q, int nsl, int slab,
                                                          float* __restrict__ part) {
    __shared__ float ol[WO * WLD];
    __shared__ float tl[WC * WLD];
    const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
    const int sl = blockIdx.x, b = sl / nsl, p0 = (sl - b * nsl) * slab, p1 = min(Q, p0 + slab);
    const int o0 = blockIdx.y * WO, c0 = blockIdx.z * WC;
    const float* __restrict__ A = gm + (int64_t)b * O * Q;
    const float* __restrict__ Bm = in + (int64_t)b * C * Q;
    const int kl = tid & 31, dr = tid >> 5;     // staging: lane = p, 8 rows per step
    const int nchunks = (p1 - p0 + WK - 1) / WK;

    floatx16 acc[2][2];
    ECORR_FRAME_CLEAR(acc)

    float ro[WO / 8], rt[WC / 8];
    auto load_chunk = [&](int kc) {
        const int p = p0 + kc * WK + kl;
        const bool pv = p < p1;
#pragma unroll
        for (int i = 0; i < WO / 8; ++i) {
            const int o = o0 + dr + 8 * i;
            ro[i] = (pv && o < O) ? A[(int64_t)o * Q + p] : 0.0f;
        }
#pragma unroll
        for (int i = 0; i < WC / 8; ++i) {
            const int c = c0 + dr + 8 * i;
            rt[i] = (pv && c < C) ? Bm[(int64_t)c * Q + p] : 0.0f;
        }
    };
    auto store_chunk = [&]() {
#pragma unroll
        for (int i = 0; i < WO / 8; ++i) ol[(dr + 8 * i) * WLD + kl] = ro[i];
#pragma unroll
        for (int i = 0; i < WC / 8; ++i) tl[(dr + 8 * i) * WLD + kl] = rt[i];
    };

    ECORR_FRAME_K_LOOP(false, nchunks, ol, tl, lane, wave, acc, load_chunk, store_chunk)

    // epilogue: lane (n, kh) holds column c, rows mfma_c_row(r, kh) of each 32 x 32 tile
    float* __restrict__ P = part + (int64_t)sl * O * C;
    const int kh = lane >> 5;
#pragma unroll
    for (int j = 0; j < 2; ++j) {
        const int c = c0 + 32 * j + (lane & 31);
        if (c >= C) continue;
#pragma unroll
        for (int i = 0; i < 2; ++i)
#pragma unroll
            for (int r = 0; r < 16; ++r) {
                const int o = mfma_c_row(r, kh, o0 + 64 * wave + 32 * i);
                if (o < O) P[(int64_t)o * C + c] = acc[i][j][r];
            }
    }
}

// grad_weight[i] = the nslab partials of element i in ascending slab order
__global__ __launch_bounds__(MNT) void weight_reduce_kernel(const float* __restrict__ part, int64_t nslab, int64_t n,
                                                            float* __restrict__ gw) {
    for (int64_t i = (int64_t)blockIdx.x * MNT + threadIdx.x; i < n; i += (int64_t)gridDim.x * MNT) {
        float s = 0.f;
        for (int64_t sl = 0; sl < nslab; ++sl) s += part[sl * n + i];
        gw[i] = s;
    }
}

}  // namespace

int conv1x1_relu_backward_workspace_bytes(int B, int C, int Q, int O, int64_t* bytes) {
    ConvGradLayout L;
    const int st = conv_grad_layout(B, C, Q, O, &L);
    if (st == ECORR_OK) *bytes = L.total;
    return st;
}

int launch_conv1x1_relu_backward(const float* grad_out, const float* out, const float* in, const void* packed_t, int B,
                                 int C, int Q, int O, float* grad_in, float* grad_weight, float* grad_bias,
                                 void* workspace, hipStream_t stream) {
    ConvGradLayout L;
    int st = conv_grad_layout(B, C, Q, O, &L);
    if (st != ECORR_OK) return st;
    char* ws = (char*)workspace;
    float* gm = (float*)(ws + L.gm);
    float* qmax = (float*)(ws + L.qmax);
    float* bpart = (float*)(ws + L.bpart);
    float* wpart = (float*)(ws + L.wpart);

    hipLaunchKernelGGL(relu_mask_kernel, dim3((unsigned)L.nqb, (unsigned)L.G, (unsigned)B), dim3(MNT), 0, stream,
                       grad_out, out, O, Q, gm, qmax, bpart);
    if ((st = hip_status()) != ECORR_OK) return st;
    if (grad_bias) {
        hipLaunchKernelGGL(bias_reduce_kernel, dim3((unsigned)((O + kWave - 1) / kWave)), dim3(BNT), 0, stream, bpart,
                           (int64_t)B * L.nqb, O, grad_bias);
        if ((st = hip_status()) != ECORR_OK) return st;
    }
    if (grad_in) {
        st = launch_conv1x1_split_linear(gm, B, O, Q, qmax, L.G, packed_t, C, grad_in, stream);
        if (st != ECORR_OK) return st;
    }
    if (grad_weight) {
        const int64_t nslab = (int64_t)B * L.nsl, n = (int64_t)O * C;
        hipLaunchKernelGGL(grad_weight_kernel,
                           dim3((unsigned)nslab, (unsigned)((O + WO - 1) / WO), (unsigned)((C + WC - 1) / WC)),
                           dim3(MNT), 0, stream, gm, in, O, C, Q, L.nsl, L.slab, wpart);
        if ((st = hip_status()) != ECORR_OK) return st;
        const int64_t g = (n + MNT - 1) / MNT;
        hipLaunchKernelGGL(weight_reduce_kernel, dim3((unsigned)(g < 65536 ? g : 65536)), dim3(MNT), 0, stream, wpart,
                           nslab, n, grad_weight);
    }
    return hip_status();
}

}  // namespace ecorr
