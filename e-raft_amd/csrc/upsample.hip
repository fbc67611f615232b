// upsample.hip -- SURVEY §8f row 4: convex 8x flow upsampling and the DSEC 16-bit PNG flow codec.
//
// ERAFT.upsample_flow (model/eraft.py:74-85), run after every GRU iteration (eraft.py:137-139):
//   mask  [N][9*64][H][W] viewed [N][1][9][8][8][H][W], softmax over the 9
//   unfold(8 * flow, 3x3, padding 1) viewed [N][2][9][1][1][H][W]
//   out[n][c][8h+i][8w+j] = sum_k softmax(mask[n][k*64 + i*8 + j][h][w])_k * 8 flow[n][c][h+ky-1][w+kx-1]
// with k = 3 ky + kx and zero padding.  The reference runs it as softmax, unfold, a broadcast
// multiply into a [N][2][9][8][8][H][W] tensor, a sum and a permute copy -- ~6 passes over
// 2x the mask size.  Here it is one pass: thread = (n, i, pixel p) with lanes on consecutive
// pixels, so each of its 72 mask loads is a coalesced 256-byte wave row, the 3x3 flow window
// comes from L1/L2, and the 8 sub-pixels j of a row leave as two float4 stores (a wave writes
// 64 x 32 contiguous bytes).  HBM-bound: 2304 B of mask in + 512 B of flow out per pixel.  The mask
// loads use the default cache policy (non-temporal loads: 42.2 vs 36.7 us at DSEC B = 16,
// profiles/r05_lab/up_ab_policy.txt); the output stores stay non-temporal.
//
// Numerics: softmax as max, exp(x - max), in-order sum, times the sum's reciprocal; then the
// in-order sum of the 9 products -- the reference's expression order.  exp is the hardware's
// exp2-based __expf and the division a v_rcp_f32 multiply (round 4: 42.9 vs 51.8 us per call at
// DSEC B=16, profiles/r04_lab/; normwise error vs an fp64 evaluation unchanged, 1.69e-6), so
// results agree with the reference within a few ulp rather than bit for bit (test bar 2e-6).
//
// The backward (ecorr_upsample_flow_backward; replaces autograd of eraft.py:74-85).  With s the
// forward's softmax, recomputed from mask by the same softmax9 (nothing mask-sized is saved), f8 the
// forward's window and g = grad_out[n][c][8h+i][8w+j]:
//   a_k = g_0 f8[0][k] + g_1 f8[1][k]
//   grad_mask[n][k*64+i*8+j][h][w] = s_k (a_k - sum_k' s_k' a_k')            (sum with k' ascending)
//   t[n][c][k][h][w] = sum_{i,j} s_k g_c                                       (64 terms per pixel)
//   grad_flow[n][c][y][x] = 8 sum_k t[n][c][k][y-ky+1][x-kx+1]                (sources inside the map)
// upsample_backward_kernel: one 512-thread workgroup owns 64 consecutive pixels, wave i their sub-row
// i, lanes on consecutive pixels: the 72 mask loads and the 72 grad_mask stores are whole 256-byte
// wave rows, a thread's 8 sub-pixels of grad_out two 16-byte loads per channel.  The grad_mask stores
// are non-temporal (69.1 vs 83.6 us with the default policy at DSEC B = 16).  upsample_flow_grad_kernel
// then gathers the 9 taps of t (float[N][18][H*W] in the caller's workspace, 72 B per pixel).
// Determinism: no atomics; every cell of grad_mask, t and grad_flow has one writer, and the sums run
// in one fixed order: j ascending (each thread, in registers), then i ascending (the 8 waves' partial
// t through LDS, one thread per (c, k, pixel)), then k ascending (the gather); times 8 last.
// Outputs are overwritten.  HBM-bound: 2304 B mask in + 512 B grad_out in + 2304 B grad_mask out per
// pixel, + 144 B of t out and back.  A non-finite logit stays in its sub-pixel's 9 grad_mask taps and
// its pixel's t, so in the 3x3 neighbourhood of grad_flow (the gather selects, it never multiplies by 0).
//
// DSEC submission codec (utils/visualization.py:75-93, utils/dsec_utils.py:66-83):
//   encode  uint16[h][w][3] = (u16)(int32)rint(flow * 128 + 2^15), channel 2 = 0 -- numpy's
//           float32 -> uint16 cast on x86 (cvttss2si, low 16 bits; NaN / out-of-int32 -> 0)
//   decode  flow[h][w][2] = (v - 2^15) / 128 where channel 2 == 1, else 0; valid = channel 2 == 1;
//           channel 2 outside {0, 1} is the reference's assertion failure (counted).
// Both are exact integer/byte work (bit-exact).
#include "ecorr_device.h"
#include "ecorr_internal.h"
#include "split_f16.h"

namespace ecorr {

namespace {

constexpr int NTU = 256;

// The softmax over the 9 taps of one sub-pixel, in place: max, exp(x - max), in-order sum, times the
// sum's reciprocal (header, Numerics).  The one definition: the forward and its backward both call it.
__device__ __forceinline__ void softmax9(float (&m)[9]) {
    float mx = m[0];
#pragma unroll
    for (int k = 1; k < 9; ++k) mx = fmaxf(mx, m[k]);
    float s = 0.0f;
#pragma unroll
    for (int k = 0; k < 9; ++k) {
        m[k] = __expf(__fsub_rn(m[k], mx));
        s = __fadd_rn(s, m[k]);
    }
    const float rs = __builtin_amdgcn_rcpf(s);
#pragma unroll
    for (int k = 0; k < 9; ++k) m[k] = __fmul_rn(m[k], rs);   // softmax output
}

__global__ __launch_bounds__(NTU) void upsample_kernel(const float* __restrict__ flow, const float* __restrict__ mask,
                                                      int H, int W, float* __restrict__ out) {
    const int HW = H * W;
    const int p = blockIdx.x * NTU + threadIdx.x;
    const int i = blockIdx.y, n = blockIdx.z;
    if (p >= HW) return;
    const int h = p / W, w = p - h * W;

    // 8 * flow over the 3x3 window, zero padded (F.unfold(8 * flow, [3,3], padding=1))
    float f8[2][9];
#pragma unroll
    for (int c = 0; c < 2; ++c) {
        const float* fc = flow + ((int64_t)n * 2 + c) * HW;
#pragma unroll
        for (int k = 0; k < 9; ++k) {
            const int y = h + k / 3 - 1, x = w + k % 3 - 1;
            const bool in = (unsigned)y < (unsigned)H && (unsigned)x < (unsigned)W;
            f8[c][k] = in ? __fmul_rn(8.0f, fc[y * W + x]) : 0.0f;
        }
    }

    const float* mrow = mask + ((int64_t)n * 576 + i * 8) * HW + p;
    float res[2][8];
#pragma unroll
    for (int j = 0; j < 8; ++j) {
        float m[9];
#pragma unroll
        for (int k = 0; k < 9; ++k) m[k] = mrow[((int64_t)k * 64 + j) * HW];   // default policy: 36.7 vs 42.2 us non-temporal
        softmax9(m);
#pragma unroll
        for (int c = 0; c < 2; ++c) {
            float acc = 0.0f;
#pragma unroll
            for (int k = 0; k < 9; ++k) acc = __fadd_rn(acc, __fmul_rn(m[k], f8[c][k]));
            res[c][j] = acc;
        }
    }
    const int W8 = 8 * W;
#pragma unroll
    for (int c = 0; c < 2; ++c) {
        float* o = out + (((int64_t)n * 2 + c) * 8 * H + 8 * h + i) * W8 + 8 * w;
        __builtin_nontemporal_store(floatx4{res[c][0], res[c][1], res[c][2], res[c][3]}, (floatx4*)o);
        __builtin_nontemporal_store(floatx4{res[c][4], res[c][5], res[c][6], res[c][7]}, (floatx4*)(o + 4));
    }
}

// ---- the backward (ecorr_upsample_flow_backward; header: "The backward") ----
constexpr int UBP = 64;         // coarse pixels per workgroup: one wave row
constexpr int NTB = 8 * UBP;    // wave i of the workgroup owns sub-row i of those pixels

// grad_mask (MASK) and t[n][c*9+k][p] = sum_{i,j} s_k g_c (FLOW).  Thread = (pixel p, sub-row i) with
// lanes on consecutive pixels, as the forward: the mask loads and the grad_mask stores are whole
// 256-byte wave rows.  t: each thread sums its 8 j in order, then the 8 waves' partials meet in LDS
// and are summed with i ascending by one thread per (c, k, pixel).
template <bool MASK, bool FLOW>
__global__ __launch_bounds__(NTB) void upsample_backward_kernel(const float* __restrict__ grad_out,
                                                               const float* __restrict__ flow,
                                                               const float* __restrict__ mask, int H, int W,
                                                               float* __restrict__ grad_mask, float* __restrict__ t) {
    __shared__ float red[FLOW ? 8 * 18 * UBP : 1];
    const int HW = H * W;
    const int lane = threadIdx.x & (UBP - 1), i = threadIdx.x / UBP;
    const int p0 = blockIdx.x * UBP, n = blockIdx.y;
    const int p = p0 + lane;

    float tt[2][9];
#pragma unroll
    for (int c = 0; c < 2; ++c)
#pragma unroll
        for (int k = 0; k < 9; ++k) tt[c][k] = 0.0f;

    if (p < HW) {   // no early return: every thread reaches the barrier below
        const int h = p / W, w = p - h * W;
        float f8[2][9];   // the forward's window of 8 * flow (only grad_mask reads it)
        if constexpr (MASK) {
#pragma unroll
            for (int c = 0; c < 2; ++c) {
                const float* fc = flow + ((int64_t)n * 2 + c) * HW;
#pragma unroll
                for (int k = 0; k < 9; ++k) {
                    const int y = h + k / 3 - 1, x = w + k % 3 - 1;
                    const bool in = (unsigned)y < (unsigned)H && (unsigned)x < (unsigned)W;
                    f8[c][k] = in ? __fmul_rn(8.0f, fc[y * W + x]) : 0.0f;
                }
            }
        }
        float g[2][8];   // grad_out[n][c][8h+i][8w .. 8w+7]: two 16-byte loads per channel
#pragma unroll
        for (int c = 0; c < 2; ++c) {
            const float* gp = grad_out + (((int64_t)n * 2 + c) * 8 * H + 8 * h + i) * (8 * W) + 8 * w;
            const floatx4 lo = *(const floatx4*)gp, hi = *(const floatx4*)(gp + 4);
            g[c][0] = lo[0]; g[c][1] = lo[1]; g[c][2] = lo[2]; g[c][3] = lo[3];
            g[c][4] = hi[0]; g[c][5] = hi[1]; g[c][6] = hi[2]; g[c][7] = hi[3];
        }
        const int64_t row = ((int64_t)n * 576 + i * 8) * HW + p;
        const float* mrow = mask + row;
#pragma unroll
        for (int j = 0; j < 8; ++j) {
            float m[9];
#pragma unroll
            for (int k = 0; k < 9; ++k) m[k] = mrow[((int64_t)k * 64 + j) * HW];
            softmax9(m);
            if constexpr (MASK) {
                float a[9], dot = 0.0f;
#pragma unroll
                for (int k = 0; k < 9; ++k) {
                    a[k] = __fadd_rn(__fmul_rn(g[0][j], f8[0][k]), __fmul_rn(g[1][j], f8[1][k]));
                    dot = __fadd_rn(dot, __fmul_rn(m[k], a[k]));
                }
#pragma unroll
                for (int k = 0; k < 9; ++k)
                    __builtin_nontemporal_store(__fmul_rn(m[k], __fsub_rn(a[k], dot)),
                                                &grad_mask[row + ((int64_t)k * 64 + j) * HW]);   // 69.1 vs 83.6 us plain
            }
            if constexpr (FLOW) {
#pragma unroll
                for (int c = 0; c < 2; ++c)
#pragma unroll
                    for (int k = 0; k < 9; ++k) tt[c][k] = __fadd_rn(tt[c][k], __fmul_rn(m[k], g[c][j]));
            }
        }
    }

    if constexpr (FLOW) {
#pragma unroll
        for (int c = 0; c < 2; ++c)
#pragma unroll
            for (int k = 0; k < 9; ++k) red[(i * 18 + c * 9 + k) * UBP + lane] = tt[c][k];
        __syncthreads();
        for (int e = threadIdx.x; e < 18 * UBP; e += NTB) {
            const int ck = e / UBP, l = e & (UBP - 1);
            float acc = red[ck * UBP + l];
#pragma unroll
            for (int ii = 1; ii < 8; ++ii) acc = __fadd_rn(acc, red[(ii * 18 + ck) * UBP + l]);
            if (p0 + l < HW) t[((int64_t)n * 18 + ck) * HW + p0 + l] = acc;
        }
    }
}

// grad_flow[n][c][y][x] = 8 * sum_k t[n][c*9+k][y-ky+1][x-kx+1], k ascending, over the pixels inside
// the map (pixel (y-ky+1, x-kx+1) read (y, x) as its tap k).  Thread = (n, c, pixel).
__global__ __launch_bounds__(NTU) void upsample_flow_grad_kernel(const float* __restrict__ t, int H, int W,
                                                                float* __restrict__ grad_flow) {
    const int HW = H * W;
    const int p = blockIdx.x * NTU + threadIdx.x;
    const int c = blockIdx.y, n = blockIdx.z;
    if (p >= HW) return;
    const int y = p / W, x = p - y * W;
    const float* tc = t + ((int64_t)n * 18 + c * 9) * HW;
    float acc = 0.0f;
#pragma unroll
    for (int k = 0; k < 9; ++k) {
        const int sy = y - k / 3 + 1, sx = x - k % 3 + 1;
        if ((unsigned)sy < (unsigned)H && (unsigned)sx < (unsigned)W)
            acc = __fadd_rn(acc, tc[(int64_t)k * HW + sy * W + sx]);
    }
    grad_flow[((int64_t)n * 2 + c) * HW + p] = __fmul_rn(8.0f, acc);
}

// numpy float32 -> uint16 on x86: cvttss2si (NaN / beyond int32 -> INT_MIN), keep the low 16 bits.
__device__ __forceinline__ uint16_t x86_f32_to_u16(float v) {
    const int iv = (v >= -2147483648.0f && v < 2147483648.0f) ? (int)v : (int)0x80000000u;
    return (uint16_t)(iv & 0xffff);
}

__global__ __launch_bounds__(NTU) void png16_encode_kernel(const float* __restrict__ flow, int64_t HW, int64_t n,
                                                           uint16_t* __restrict__ out) {
    for (int64_t q = blockIdx.x * (int64_t)NTU + threadIdx.x; q < n; q += (int64_t)gridDim.x * NTU) {
        const int64_t b = q / HW, p = q - b * HW;
        const float u = flow[(b * 2 + 0) * HW + p], v = flow[(b * 2 + 1) * HW + p];
        // visualization.py:82 numpy.rint(flow*128 + 2**15) in float32
        out[3 * q + 0] = x86_f32_to_u16(rintf(__fadd_rn(__fmul_rn(u, 128.0f), 32768.0f)));
        out[3 * q + 1] = x86_f32_to_u16(rintf(__fadd_rn(__fmul_rn(v, 128.0f), 32768.0f)));
        out[3 * q + 2] = 0;   // :84 the third channel is written as zeros
    }
}

__global__ __launch_bounds__(NTU) void png16_decode_kernel(const uint16_t* __restrict__ in, int64_t n,
                                                           float* __restrict__ flow, uint8_t* __restrict__ valid,
                                                           int* __restrict__ bad) {
    for (int64_t q = blockIdx.x * (int64_t)NTU + threadIdx.x; q < n; q += (int64_t)gridDim.x * NTU) {
        const unsigned u = in[3 * q], v = in[3 * q + 1], m = in[3 * q + 2];
        const bool ok = m == 1;   // dsec_utils.py:73
        if (m > 1) atomicAdd(bad, 1);   // :75 assert np.all(flow_16bit[~valid2D, -1] == 0)
        // :79-80 (v - 2**15) / 128, exact in float32
        flow[2 * q + 0] = ok ? (float)((int)u - 32768) * 0.0078125f : 0.0f;
        flow[2 * q + 1] = ok ? (float)((int)v - 32768) * 0.0078125f : 0.0f;
        valid[q] = ok;
    }
}

inline unsigned grid_for(int64_t n) {
    const int64_t g = (n + NTU - 1) / NTU;
    return (unsigned)(g < 16384 ? (g > 0 ? g : 1) : 16384);
}

}  // namespace

int launch_upsample_flow(const float* flow, const float* mask, int N, int H, int W, float* out, hipStream_t stream) {
    const dim3 grid((unsigned)((H * W + NTU - 1) / NTU), 8, (unsigned)N);
    hipLaunchKernelGGL(upsample_kernel, grid, dim3(NTU), 0, stream, flow, mask, H, W, out);
    return hip_status();
}

int64_t upsample_backward_workspace_bytes(int N, int H, int W) { return (int64_t)N * 18 * H * W * sizeof(float); }

int launch_upsample_flow_backward(const float* grad_out, const float* flow, const float* mask, int N, int H, int W,
                                  float* grad_flow, float* grad_mask, void* workspace, hipStream_t stream) {
    const int HW = H * W;
    const dim3 grid((unsigned)((HW + UBP - 1) / UBP), (unsigned)N);
    float* t = static_cast<float*>(workspace);
    if (grad_flow && grad_mask)
        hipLaunchKernelGGL((upsample_backward_kernel<true, true>), grid, dim3(NTB), 0, stream, grad_out, flow, mask, H,
                           W, grad_mask, t);
    else if (grad_mask)
        hipLaunchKernelGGL((upsample_backward_kernel<true, false>), grid, dim3(NTB), 0, stream, grad_out, flow, mask,
                           H, W, grad_mask, t);
    else
        hipLaunchKernelGGL((upsample_backward_kernel<false, true>), grid, dim3(NTB), 0, stream, grad_out, flow, mask,
                           H, W, grad_mask, t);
    if (grad_flow) {
        const dim3 ggrid((unsigned)((HW + NTU - 1) / NTU), 2, (unsigned)N);
        hipLaunchKernelGGL(upsample_flow_grad_kernel, ggrid, dim3(NTU), 0, stream, t, H, W, grad_flow);
    }
    return hip_status();
}

int launch_png16_encode(const float* flow, int B, int h, int w, uint16_t* out, hipStream_t stream) {
    const int64_t HW = (int64_t)h * w, n = (int64_t)B * HW;
    hipLaunchKernelGGL(png16_encode_kernel, dim3(grid_for(n)), dim3(NTU), 0, stream, flow, HW, n, out);
    return hip_status();
}

int launch_png16_decode(const uint16_t* in, int B, int h, int w, float* flow, uint8_t* valid, int* bad,
                        hipStream_t stream) {
    const int64_t n = (int64_t)B * h * w;
    hipLaunchKernelGGL(png16_decode_kernel, dim3(grid_for(n)), dim3(NTU), 0, stream, in, n, flow, valid, bad);
    return hip_status();
}

}  // namespace ecorr
