// lookup.hip -- CorrBlock.__call__ on gfx950: radius-r bilinear window lookup over the pyramid.
//
// Replaces corr.py:29-50 (+ utils.py:7-21 bilinear_sampler, ATen grid_sampler_2d): for query p,
// level i, offsets a (x) and b (y) in [0, 2r]:
//   out[b][i*(2r+1)^2 + a*(2r+1) + b][p] = bilinear(level_i[p], x/2^i + a - r, y/2^i + b - r)
// bit-exact with the reference on CPU (same fp32 op sequence, ecorr_device.h).
//
// The lookup is an HBM-bound gather: each query reads its own (2r+2)^2 window per level and
// nothing is shared between queries.  One workgroup = 64 consecutive queries x 1 level; the
// window staging (phases 0-1) is lookup_stage.h; phase 2 writes every output from LDS with lanes
// = 64 consecutive queries, so each channel store is one 256-byte coalesced row of the NCHW
// output, stored non-temporally.  The lookup kernels themselves are templates in lookup_kernels.h
// (this file instantiates their fp32 forms, lookup_half.hip the 16-bit outputs of ecorr_lookup_as).
#include "ecorr_device.h"
#include "ecorr_internal.h"
#include "lookup_kernels.h"
#include "lookup_stage.h"
#include "split_f16.h"

namespace ecorr {

namespace {

// Partial maxima for the lookups without a QMAX instantiation: thread = (b, query), the max of |out|
// over all C channels into group 0, zeros into the other 3 * levels - 1.
__global__ __launch_bounds__(NT) void qmax_kernel(LookupParams P, int B) {
    const int64_t i = blockIdx.x * (int64_t)NT + threadIdx.x;
    if (i >= (int64_t)B * P.q_count) return;
    const int64_t b = i / P.q_count, p = i % P.q_count, Q = P.q_count, G = 3 * P.levels;
    float m = 0.0f;
    for (int c = 0; c < P.C; ++c) m = fmaxf(m, fabsf(P.out[(b * P.C + c) * Q + p]));
    for (int g = 0; g < G; ++g) P.qmax[(b * G + g) * Q + p] = g == 0 ? m : 0.0f;
}

// utils.py:7-21 for arbitrary img [N][C][h][w] and pixel grid [N][Hg][Wg][2].
__global__ __launch_bounds__(NT) void sampler_kernel(const float* __restrict__ img, int N, int C, int h, int w,
                                                     const float* __restrict__ coords, int64_t G,
                                                     float* __restrict__ out, float* __restrict__ mask) {
    const int64_t n = (int64_t)N * G;
    for (int64_t i = blockIdx.x * (int64_t)NT + threadIdx.x; i < n; i += (int64_t)gridDim.x * NT) {
        const int64_t ni = i / G, gi = i - ni * G;
        const float x = coords[2 * i], y = coords[2 * i + 1];
        for (int c = 0; c < C; ++c)
            out[(ni * C + c) * G + gi] = sample_px(img + (ni * C + c) * (int64_t)h * w, h, w, x, y);
        if (mask) {  // utils.py:17-19, on the normalized coordinates
            const float gx = __fsub_rn(__fdiv_rn(__fmul_rn(2.0f, x), (float)(w - 1)), 1.0f);
            const float gy = __fsub_rn(__fdiv_rn(__fmul_rn(2.0f, y), (float)(h - 1)), 1.0f);
            mask[i] = ((gx > -1.0f) & (gy > -1.0f) & (gx < 1.0f) & (gy < 1.0f)) ? 1.0f : 0.0f;
        }
    }
}

// utils.py:24-27
__global__ __launch_bounds__(NT) void coords_grid_kernel(int B, int H, int W, float* __restrict__ out) {
    const int64_t hw = (int64_t)H * W, n = (int64_t)B * 2 * hw;
    for (int64_t i = blockIdx.x * (int64_t)NT + threadIdx.x; i < n; i += (int64_t)gridDim.x * NT) {
        const int64_t pix = i % hw;
        const int ch = (int)((i / hw) & 1);
        out[i] = ch == 0 ? (float)(pix % W) : (float)(pix / W);
    }
}

// Presplit column exponents (ecorr_split_column_scale).  Every sample of query p (any level: pooled
// averages and bilinear blends of level-0 values) is bounded by max_t |corr0[p][t]| <=
// sqrt(D) m1_p M2 (Cauchy-Schwarz on |f| <= max |f|), m1_p = max_d |f1[d][p]|, M2 = max |f2| over
// the batch item; with m < 2^(15 - split_exponent(m)) and sqrt(D) <= 2^hd the scale
// 2^(e1 + E2 - 15 - hd) puts every sample below 2^15 (f16 max 65504: 2x headroom for rounding).
// A loose bound only lowers the samples' magnitude, not their 22-bit hi + lo precision, until lo
// falls under f16's normal range (scaled |x| < 2^-3).  The maxima are over finite values: a sample
// touching a non-finite fmap value is non-finite itself (and NaNs its query in the conv, the split
// contract), every other sample is bounded by the finite values it was made of.

// max |f2| (finite) per batch item as float bits (non-negative floats order as unsigned ints)
__global__ __launch_bounds__(NT) void colscale_m2_kernel(const float* __restrict__ f2, int64_t n,
                                                         unsigned* __restrict__ m2) {
    __shared__ unsigned red[NT / 64];
    const int b = blockIdx.y;
    const float* x = f2 + (int64_t)b * n;
    unsigned m = 0;
    auto take = [&](float v) {   // finite values only (below)
        const unsigned u = __float_as_uint(v) & 0x7fffffffu;
        m = u < 0x7f800000u ? max(m, u) : m;
    };
    if (n % 4 == 0 && (reinterpret_cast<uintptr_t>(x) & 15) == 0) {   // 16-byte loads
        const float4* x4 = reinterpret_cast<const float4*>(x);
#pragma unroll 4
        for (int64_t i = blockIdx.x * (int64_t)NT + threadIdx.x; i < n / 4; i += (int64_t)gridDim.x * NT) {
            const float4 v = x4[i];
            take(v.x), take(v.y), take(v.z), take(v.w);
        }
    } else {
        for (int64_t i = blockIdx.x * (int64_t)NT + threadIdx.x; i < n; i += (int64_t)gridDim.x * NT) take(x[i]);
    }
#pragma unroll
    for (int d = 32; d > 0; d >>= 1) m = max(m, (unsigned)__shfl_xor((int)m, d));
    if ((threadIdx.x & 63) == 0) red[threadIdx.x >> 6] = m;
    __syncthreads();
    if (threadIdx.x == 0) {
        for (int w = 1; w < NT / 64; ++w) m = max(m, red[w]);
        atomicMax(&m2[b], m);
    }
}

__global__ __launch_bounds__(NT) void colscale_kernel(const float* __restrict__ f1, int B, int D, int Q, int hd,
                                                      const unsigned* __restrict__ m2, int* __restrict__ scale) {
    const int64_t i = blockIdx.x * (int64_t)NT + threadIdx.x;
    if (i >= (int64_t)B * Q) return;
    const int64_t b = i / Q, p = i - b * Q;
    const float* x = f1 + b * D * Q + p;
    unsigned m = 0;
#pragma unroll 16
    for (int d = 0; d < D; ++d) {   // 16 loads in flight per thread (coalesced over the queries)
        const unsigned u = __float_as_uint(x[(int64_t)d * Q]) & 0x7fffffffu;
        m = u < 0x7f800000u ? max(m, u) : m;
    }
    const int s = split_exponent(__uint_as_float(m)) + split_exponent(__uint_as_float(m2[b])) - 15 - hd;
    scale[i] = s < -126 ? -126 : (s > 126 ? 126 : s);
}

}  // namespace

int launch_lookup(const LookupParams& P, int B, hipStream_t stream, int out_format) {
    if (out_format != ECORR_OUT_F32) {
        if (P.qmax || P.scale) return ECORR_EINVAL;
        return launch_lookup_half(P, B, stream, out_format);   // lookup_half.hip
    }
    const dim3 grid((unsigned)((P.q_count + 63) / 64), (unsigned)P.levels, (unsigned)B);
    bool pair;
    if (P.radius == 4 && (P.scale || P.qmax) && lookup_takes_cols(P, 4, &pair)) {
        if (P.scale) {
            if (pair) hipLaunchKernelGGL((lookup_cols_reg<4, 64, true, false, true>), grid, dim3(192), 0, stream, P);
            else hipLaunchKernelGGL((lookup_cols_reg<4, 64, false, false, true>), grid, dim3(192), 0, stream, P);
        } else {
            if (pair) hipLaunchKernelGGL((lookup_cols_reg<4, 64, true, true>), grid, dim3(192), 0, stream, P);
            else hipLaunchKernelGGL((lookup_cols_reg<4, 64, false, true>), grid, dim3(192), 0, stream, P);
        }
        return hip_status();
    }
    // the paths without a QMAX instantiation: the lookup, then qmax_kernel over its output
    const int st = launch_lookup_plain<ECORR_OUT_F32>(P, B, stream);
    if (st != ECORR_OK || !P.qmax) return st;
    hipLaunchKernelGGL(qmax_kernel, dim3(grid_for((int64_t)B * P.q_count)), dim3(NT), 0, stream, P, B);
    return hip_status();
}

int launch_bilinear_sampler(const float* img, int N, int C, int h, int w, const float* coords,
                            int Hg, int Wg, float* out, float* mask, hipStream_t stream) {
    const int64_t G = (int64_t)Hg * Wg;
    hipLaunchKernelGGL(sampler_kernel, dim3(grid_for((int64_t)N * G)), dim3(NT), 0, stream, img, N, C, h,
                       w, coords, G, out, mask);
    return hip_status();
}

int launch_coords_grid(int B, int H, int W, float* out, hipStream_t stream) {
    hipLaunchKernelGGL(coords_grid_kernel, dim3(grid_for((int64_t)B * 2 * H * W)), dim3(NT), 0, stream, B,
                       H, W, out);
    return hip_status();
}

int launch_split_column_scale(const float* f1, const float* f2, int B, int D, int H, int W, int* scale,
                              hipStream_t stream) {
    const int64_t Q = (int64_t)H * W;
    if (B <= 0 || D <= 0 || Q <= 0 || B > 65535 || Q > 0x7fffffff) return ECORR_EINVAL;
    int hd = 0;
    while (((int64_t)1 << (2 * hd)) < D) ++hd;   // sqrt(D) <= 2^hd
    unsigned* m2 = reinterpret_cast<unsigned*>(scale + B * Q);
    const hipError_t e = hipMemsetAsync(m2, 0, (size_t)B * 4, stream);
    if (e != hipSuccess) return ECORR_EHIP - (int)e;
    const int64_t n = (int64_t)D * Q;
    const unsigned gx = (unsigned)std::min<int64_t>((n + NT * 64 - 1) / (NT * 64), 1024);
    hipLaunchKernelGGL(colscale_m2_kernel, dim3(gx, B), dim3(NT), 0, stream, f2, n, m2);
    hipLaunchKernelGGL(colscale_kernel, dim3((unsigned)((B * Q + NT - 1) / NT)), dim3(NT), 0, stream, f1, B, D, (int)Q,
                       hd, m2, scale);
    return hip_status();
}

}  // namespace ecorr
