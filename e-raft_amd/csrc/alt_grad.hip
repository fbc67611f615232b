// alt_grad.hip -- the backward of the volume-free lookup (ecorr_alt_backward_workspace_size,
// ecorr_alt_lookup_backward, ecorr_alt_pack_backward, include/ecorr.h).
//
// With s = 1 / sqrt(D), F2_i the pooled fmap2 level i and Wg_i[p] the (2r+3)^2 window gradient of query
// p on level i (the volume lookup's backward window, lookup_grad_window.h):
//   grad_f1[p,:]   = s sum_i sum_{t in window} Wg_i[p][t] F2_i[t,:]
//   grad_F2_i[t,:] = s sum_p Wg_i[p][t] f1[p,:]
// and grad_fmap2 is the fold T_0 = g_0 + 1/4 up(g_1 + 1/4 up(g_2 + ...)) of the grad_F2_i (the chain of
// floor-mode avg_pool2d backwards: a dropped odd last row / column gets no coarse term).
//   alt_window_grad_kernel  lookup_backward_kernel's grid and its phases 0 - 2 (the shared device
//                           function); writes each query's window and origin to the workspace
//   alt_grad_f1_kernel      one wave per query: levels in order, window cells in row order, the lanes
//                           hold a float4 of channels; grad_feat.f1[p] += s acc (one owner)
//   alt_grad_f2_kernel      one workgroup per (batch item, level, target pixel): its 8 waves scan fixed
//                           eighths of the queries in ascending order (64 origins per step, a ballot of
//                           the hits), the partial sums are added in wave order through LDS
//   alt_fold_kernel, alt_untranspose_kernel   the pack's pooling and transposes reversed
// No atomics; every sum has a fixed order, so equal inputs give bitwise equal gradients.  Every load
// address is computed for in-image pixels only; every store is a plain vector store.
#include <algorithm>

#include "ecorr_device.h"
#include "ecorr_internal.h"
#include "lookup_grad_window.h"

namespace ecorr {

namespace {

constexpr int NT = 256;
constexpr int F2_NW = 8;   // waves of one grad_F2 workgroup = fixed chunks of the query range
constexpr int F2_SG = 4;   // scan steps (64 origins each) whose loads a grad_F2 wave keeps in flight together

// ---- (a) the window gradients ----------------------------------------------------------------
// RT >= 0: compile-time radius (r = 4), RT < 0: P.radius.
template <int RT>
__global__ __launch_bounds__(NT) void alt_window_grad_kernel(AltGradParams P, int QB) {
    extern __shared__ float lds[];
    const int r = RT >= 0 ? RT : P.radius;
    const int K = 2 * r + 1, S = K + 2, KK = K * K, SS = S * S;
    const int QP = QB + 1;
    const GradWindowLds L = grad_window_carve(lds, K, S, QB);

    const int tid = threadIdx.x;
    const int lv = blockIdx.y, b = blockIdx.z;
    const int q0 = blockIdx.x * QB;
    const int h = P.lh[lv], w = P.lw[lv];
    const float inv = 1.0f / (float)(1 << lv);
    const int64_t Q = P.Q;
    const float* __restrict__ cxp = P.coords + ((int64_t)b * 2 + 0) * Q;
    const float* __restrict__ cyp = P.coords + ((int64_t)b * 2 + 1) * Q;
    const float* __restrict__ gout = P.grad_out + ((int64_t)b * P.C + (int64_t)lv * KK) * Q;

    grad_window_phases<NT>(L, cxp, cyp, gout, Q, P.Q, q0, h, w, inv, r, QB);

    // the block's queries are consecutive rows of the workspace: the window cells go out in memory order
    const int nq = min(QB, P.Q - q0);
    const int64_t row0 = ((int64_t)b * P.levels + lv) * Q + q0;
    for (int g = tid; g < nq; g += NT) {
        const bool ok = L.org[2 * QB + g] == 0;   // NaN / inf / huge coordinates: nothing is in range, no window
        int2 o;
        o.x = ok ? L.org[g] : kAltNoWindow;
        o.y = ok ? L.org[QB + g] : 0;
        P.org[row0 + g] = o;
    }
    for (int it = tid; it < nq * SS; it += NT) {
        const int g = it / SS, cell = it - g * SS;
        P.win[row0 * SS + it] = L.win[cell * QP + g];
    }
}

// acc += wt[k] * row ri[k] of base ([..][Dp] floats, this lane's float4 at channel d) for the set
// lanes k of mask, in ascending k.  mask is wave-uniform; four rows are loaded before they are added,
// so their latencies overlap; the adds keep the order.
__device__ __forceinline__ void alt_axpy_hits(unsigned long long mask, float wt, int ri, const float* __restrict__ base,
                                              int Dp, int d, bool lok, float4& acc) {
    while (mask) {
        int kk[4];
        bool on[4];
#pragma unroll
        for (int u = 0; u < 4; ++u) {
            on[u] = mask != 0;
            kk[u] = on[u] ? (int)__builtin_ctzll(mask) : 0;
            mask &= mask - 1;
        }
        float4 v[4];
        float ws[4];
#pragma unroll
        for (int u = 0; u < 4; ++u) {
            const int row = __builtin_amdgcn_readlane(ri, kk[u]);
            ws[u] = __int_as_float(__builtin_amdgcn_readlane(__float_as_int(wt), kk[u]));
            v[u] = make_float4(0.0f, 0.0f, 0.0f, 0.0f);
            if (on[u] && lok) v[u] = *reinterpret_cast<const float4*>(base + (int64_t)row * Dp + d);
        }
#pragma unroll
        for (int u = 0; u < 4; ++u) {
            if (!on[u]) continue;
            acc.x = __builtin_fmaf(ws[u], v[u].x, acc.x);
            acc.y = __builtin_fmaf(ws[u], v[u].y, acc.y);
            acc.z = __builtin_fmaf(ws[u], v[u].z, acc.z);
            acc.w = __builtin_fmaf(ws[u], v[u].w, acc.w);
        }
    }
}

// *dst += scale step of acc (one owner: a plain read-modify-write)
__device__ __forceinline__ void alt_add_scaled(const AltGradParams& P, float* dst, const float4& acc) {
    float4 v = *reinterpret_cast<float4*>(dst);
    v.x = __fadd_rn(v.x, scale_step(P.scale_is_mul, P.scale, acc.x));
    v.y = __fadd_rn(v.y, scale_step(P.scale_is_mul, P.scale, acc.y));
    v.z = __fadd_rn(v.z, scale_step(P.scale_is_mul, P.scale, acc.z));
    v.w = __fadd_rn(v.w, scale_step(P.scale_is_mul, P.scale, acc.w));
    *reinterpret_cast<float4*>(dst) = v;
}

// ---- (b) grad_f1 -----------------------------------------------------------------------------
// Wave = query q of batch item b; 256 channels per pass.  A zero weight or a cell outside the level is
// skipped without a load; each needed F2_i pixel is one coalesced 16-byte-per-lane load.
__global__ __launch_bounds__(NT) void alt_grad_f1_kernel(AltGradParams P) {
    const int lane = threadIdx.x & (kWave - 1), wv = threadIdx.x / kWave;
    const int q = blockIdx.x * (NT / kWave) + wv, b = blockIdx.y;
    if (q >= P.Q) return;   // wave-uniform
    const int S = 2 * P.radius + 3, SS = S * S, Dp = P.Dp;
    for (int c0 = 0; c0 < Dp; c0 += 4 * kWave) {
        const int d = c0 + 4 * lane;
        const bool lok = d < Dp;
        float4 acc = make_float4(0.0f, 0.0f, 0.0f, 0.0f);
        for (int lv = 0; lv < P.levels; ++lv) {
            const int64_t row = ((int64_t)b * P.levels + lv) * P.Q + q;
            const int2 o = P.org[row];
            const int x0 = __builtin_amdgcn_readfirstlane(o.x), y0 = __builtin_amdgcn_readfirstlane(o.y);
            if (x0 == kAltNoWindow) continue;
            const int h = P.lh[lv], w = P.lw[lv];
            const float* __restrict__ lvb = P.lvl[lv] + (int64_t)b * h * w * Dp;
            const float* __restrict__ wrow = P.win + row * SS;
            for (int t0 = 0; t0 < SS; t0 += kWave) {
                const int t = t0 + lane;
                float wt = 0.0f;
                int pix = -1;
                if (t < SS) {
                    const int j = t / S, i = t - j * S;
                    const int y = y0 + j, x = x0 + i;
                    if ((unsigned)y < (unsigned)h && (unsigned)x < (unsigned)w) {
                        pix = y * w + x;
                        wt = wrow[t];
                    }
                }
                const unsigned long long mask = __ballot(pix >= 0 && wt != 0.0f);
                alt_axpy_hits(mask, wt, pix, lvb, Dp, d, lok, acc);
            }
        }
        if (lok) alt_add_scaled(P, P.g1 + ((int64_t)b * P.Q + q) * Dp + d, acc);
    }
}

// ---- (c) grad_F2 -----------------------------------------------------------------------------
// Workgroup = target pixel t of level lv of batch item b: the destination owns the sum.  Wave k scans
// the queries [k QC, (k + 1) QC) in ascending order, 64 origins per step; a lane's query hits when t is
// inside its window and the weight there is not zero.  The partial sums are added in wave order.
__global__ __launch_bounds__(F2_NW * kWave) void alt_grad_f2_kernel(AltGradParams P) {
    __shared__ float4 part[F2_NW][kWave];
    const int lane = threadIdx.x & (kWave - 1), wv = threadIdx.x / kWave;
    const int b = blockIdx.y;
    int t = blockIdx.x;
    int lv = 0;
    while (lv + 1 < P.levels && t >= P.lt0[lv + 1]) ++lv;
    t -= P.lt0[lv];
    const int h = P.lh[lv], w = P.lw[lv];
    const int ty = t / w, tx = t - ty * w;
    const int S = 2 * P.radius + 3, SS = S * S, Dp = P.Dp, Q = P.Q;
    const int QC = (((Q + F2_NW - 1) / F2_NW) + kWave - 1) & ~(kWave - 1);
    const int pb = min(Q, wv * QC), pe = min(Q, pb + QC);
    const int64_t row0 = ((int64_t)b * P.levels + lv) * Q;
    const float* __restrict__ f1b = P.f1 + (int64_t)b * Q * Dp;
    for (int c0 = 0; c0 < Dp; c0 += 4 * kWave) {
        const int d = c0 + 4 * lane;
        const bool lok = d < Dp;
        float4 acc = make_float4(0.0f, 0.0f, 0.0f, 0.0f);
        // F2_SG steps of 64 origins at a time: their origin loads, then their weight loads, are in flight
        // together (a step alone is a chain of dependent L2 round trips); the hits keep ascending order
        for (int p0 = pb; p0 < pe; p0 += F2_SG * kWave) {
            int2 o[F2_SG];
#pragma unroll
            for (int u = 0; u < F2_SG; ++u) {
                const int p = p0 + u * kWave + lane;
                o[u] = make_int2(kAltNoWindow, 0);
                if (p < pe) o[u] = P.org[row0 + p];
            }
            float wt[F2_SG];
#pragma unroll
            for (int u = 0; u < F2_SG; ++u) {
                const int p = p0 + u * kWave + lane;
                wt[u] = 0.0f;
                if (o[u].x != kAltNoWindow) {
                    const int i = tx - o[u].x, j = ty - o[u].y;
                    if ((unsigned)i < (unsigned)S && (unsigned)j < (unsigned)S) wt[u] = P.win[(row0 + p) * SS + j * S + i];
                }
            }
#pragma unroll
            for (int u = 0; u < F2_SG; ++u) {
                const unsigned long long mask = __ballot(wt[u] != 0.0f);
                alt_axpy_hits(mask, wt[u], p0 + u * kWave + lane, f1b, Dp, d, lok, acc);
            }
        }
        part[wv][lane] = acc;
        __syncthreads();
        if (wv == 0 && lok) {
            float4 s = part[0][lane];
#pragma unroll
            for (int k = 1; k < F2_NW; ++k) {
                const float4 u = part[k][lane];
                s.x = __fadd_rn(s.x, u.x);
                s.y = __fadd_rn(s.y, u.y);
                s.z = __fadd_rn(s.z, u.z);
                s.w = __fadd_rn(s.w, u.w);
            }
            alt_add_scaled(P, P.glvl[lv] + ((int64_t)b * h * w + t) * Dp + d, s);
        }
        __syncthreads();   // the next pass rewrites part
    }
}

// ---- (d) the pack's backward -------------------------------------------------------------------
// fine [B][hf wf][Dp] += 1/4 of its coarse parent [B][hc wc][Dp], hc = hf >> 1, wc = wf >> 1; a pixel of a
// dropped odd last row / column has no parent.  One float4 of channels per thread.
__global__ __launch_bounds__(NT) void alt_fold_kernel(float* __restrict__ fine, const float* __restrict__ coarse, int B,
                                                      int hf, int wf, int Dp) {
    const int hc = hf >> 1, wc = wf >> 1, d4 = Dp >> 2;
    const int64_t total = (int64_t)B * hf * wf * d4;
    for (int64_t i = (int64_t)blockIdx.x * NT + threadIdx.x; i < total; i += (int64_t)gridDim.x * NT) {
        const int c = (int)(i % d4);
        const int64_t pb = i / d4;
        const int p = (int)(pb % ((int64_t)hf * wf));
        const int64_t b = pb / ((int64_t)hf * wf);
        const int y = p / wf, x = p - y * wf;
        const int yy = y >> 1, xx = x >> 1;
        if (yy >= hc || xx >= wc) continue;
        const float4 u = reinterpret_cast<const float4*>(coarse)[(b * hc * wc + (int64_t)yy * wc + xx) * d4 + c];
        float4 v = reinterpret_cast<float4*>(fine)[i];
        v.x = __fadd_rn(v.x, __fmul_rn(0.25f, u.x));
        v.y = __fadd_rn(v.y, __fmul_rn(0.25f, u.y));
        v.z = __fadd_rn(v.z, __fmul_rn(0.25f, u.z));
        v.w = __fadd_rn(v.w, __fmul_rn(0.25f, u.w));
        reinterpret_cast<float4*>(fine)[i] = v;
    }
}

// src [B][Q][Dp] fp32 -> dst [B][D][Q] through a 32 x 32 LDS tile; the pad channels D .. Dp - 1 are dropped.
__global__ __launch_bounds__(NT) void alt_untranspose_kernel(const float* __restrict__ src, float* __restrict__ dst,
                                                             int D, int Dp, int Q) {
    __shared__ float tile[32][33];
    const int tx = threadIdx.x & 31, ty = threadIdx.x >> 5;
    const int q0 = blockIdx.x * 32, d0 = blockIdx.y * 32;
    const int64_t b = blockIdx.z;
#pragma unroll
    for (int j = 0; j < 4; ++j) {
        const int q = q0 + ty + 8 * j, d = d0 + tx;
        tile[ty + 8 * j][tx] = (q < Q && d < Dp) ? src[(b * Q + q) * Dp + d] : 0.0f;
    }
    __syncthreads();
#pragma unroll
    for (int j = 0; j < 4; ++j) {
        const int d = d0 + ty + 8 * j, q = q0 + tx;
        if (d < D && q < Q) dst[(b * D + d) * Q + q] = tile[tx][ty + 8 * j];
    }
}

}  // namespace

int64_t alt_backward_workspace_bytes(int B, int64_t Q, int levels, int radius) {
    const int64_t S = 2 * radius + 3;
    return (int64_t)B * levels * Q * (int64_t)(sizeof(int2) + S * S * sizeof(float));
}

int launch_alt_lookup_backward(const AltGradParams& P, hipStream_t stream) {
    const int QB = grad_window_queries(P.radius);
    const size_t lds = grad_window_lds_bytes(P.radius, QB);
    const dim3 wgrid((unsigned)((P.Q + QB - 1) / QB), (unsigned)P.levels, (unsigned)P.B);
    if (P.radius == 4) hipLaunchKernelGGL((alt_window_grad_kernel<4>), wgrid, dim3(NT), lds, stream, P, QB);
    else hipLaunchKernelGGL((alt_window_grad_kernel<-1>), wgrid, dim3(NT), lds, stream, P, QB);
    int st = hip_status();
    if (st != ECORR_OK) return st;
    const int wpb = NT / kWave;
    hipLaunchKernelGGL(alt_grad_f1_kernel, dim3((unsigned)((P.Q + wpb - 1) / wpb), (unsigned)P.B), dim3(NT), 0, stream, P);
    st = hip_status();
    if (st != ECORR_OK) return st;
    hipLaunchKernelGGL(alt_grad_f2_kernel, dim3((unsigned)P.lt0[P.levels], (unsigned)P.B), dim3(F2_NW * kWave), 0, stream,
                       P);
    return hip_status();
}

int launch_alt_pack_backward(float* grad_feat, int B, int D, int H, int W, const AltGeom& g, float* grad_fmap1,
                             float* grad_fmap2, hipStream_t stream) {
    const int Q = H * W;
    if (grad_fmap2) {   // coarsest first: level i - 1 += 1/4 up(level i)
        for (int i = g.levels - 1; i >= 1; --i) {
            const int64_t n = (int64_t)B * g.h[i - 1] * g.w[i - 1] * (g.Dp / 4);
            const unsigned blocks = (unsigned)std::min<int64_t>((n + NT - 1) / NT, 8192);
            hipLaunchKernelGGL(alt_fold_kernel, dim3(blocks), dim3(NT), 0, stream, grad_feat + g.off[i - 1],
                               grad_feat + g.off[i], B, g.h[i - 1], g.w[i - 1], g.Dp);
        }
    }
    const dim3 grid((unsigned)((Q + 31) / 32), (unsigned)((D + 31) / 32), (unsigned)B);
    if (grad_fmap1) hipLaunchKernelGGL(alt_untranspose_kernel, grid, dim3(NT), 0, stream, grad_feat, grad_fmap1, D, g.Dp, Q);
    if (grad_fmap2)
        hipLaunchKernelGGL(alt_untranspose_kernel, grid, dim3(NT), 0, stream, grad_feat + g.off[0], grad_fmap2, D, g.Dp, Q);
    return hip_status();
}

}  // namespace ecorr
