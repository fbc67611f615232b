// alt.hip -- the volume-free lookup (ecorr_alt_size / ecorr_alt_pack_as / ecorr_alt_lookup_as,
// include/ecorr.h): the block keeps the feature maps channel-last and every lookup
// computes the correlation values its samples need, so memory grows with Q = H W, not Q^2.
//
// avg_pool2d over the target axes is linear: level i of the volume is fmap1^T pool^i(fmap2) / sqrt(D).
// Sample positions, floors, fractions and in-image tests are the volume lookup's own device functions
// (ecorr_device.h: coord_chain, window_fit, in_image, blend), so which samples are NaN, which are
// exactly zero and which corners contribute are the volume lookup's by construction; only the corner
// values are computed differently (an fp32 dot product per corner), hence equal up to rounding.
//   alt_transpose_kernel   [B][D][Q] fmaps (fp32 / f16 / bf16) -> [B][Q][Dp] fp32, pad channels zero
//   alt_pool_kernel        one pooled fmap2 level from the one below, (((a+b)+c)+d) * 0.25f
//   alt_window_kernel<R>   r <= 4: one wave per (query, level): the (2r+3)^2 window's dot products as
//                          64 per-lane partial sums per batch, reduced by a halving butterfly that
//                          leaves tap l's sum in lane l; then the block's threads blend from LDS
//   alt_generic_kernel     any radius: per sample, its up to four in-image corner dots and the blend
// No atomics anywhere; every sum has a fixed order, so a result is bitwise reproducible.
#include <algorithm>

#include "ecorr_device.h"
#include "ecorr_internal.h"
#include "out_elem.h"
#include "split_f16.h"

namespace ecorr {

namespace {

constexpr int ALT_NT = 256;              // threads of every kernel here
constexpr int ALT_QB = 16;               // consecutive queries of one window-kernel block (4 per wave)
constexpr int ALT_OOB = 0x7ffffff0;      // buffer offset beyond any level: loads 0, touches nothing

__device__ __forceinline__ float alt_pool4(float a, float b, float c, float d) {
    return __fmul_rn(__fadd_rn(__fadd_rn(__fadd_rn(a, b), c), d), 0.25f);
}

// The build's scale step on a finished dot product (ecorr_device.h scale_step).
__device__ __forceinline__ float alt_scale(const AltParams& P, float s) {
    return scale_step(P.scale_is_mul, P.scale, s);
}

// One output element at index i of out ([B][C][Q] order), fmt = ECORR_OUT_* (uniform).
__device__ __forceinline__ void alt_store(void* out, int fmt, int64_t i, float v) {
    if (fmt == ECORR_OUT_F32) static_cast<float*>(out)[i] = out_elem<ECORR_OUT_F32>(v);
    else if (fmt == ECORR_OUT_F16) static_cast<unsigned short*>(out)[i] = out_elem<ECORR_OUT_F16>(v);
    else static_cast<unsigned short*>(out)[i] = out_elem<ECORR_OUT_BF16>(v);
}

// ---- pack ----------------------------------------------------------------------------------
// src [B][D][Q] elements of T -> dst [B][Q][Dp] fp32 through a 32 x 32 LDS tile; channels D .. Dp - 1 zero.
template <typename T>
__global__ __launch_bounds__(ALT_NT) void alt_transpose_kernel(const T* __restrict__ src, float* __restrict__ dst,
                                                               int D, int Dp, int Q) {
    __shared__ float tile[32][33];
    const int tx = threadIdx.x & 31, ty = threadIdx.x >> 5;
    const int q0 = blockIdx.x * 32, d0 = blockIdx.y * 32;
    const int64_t b = blockIdx.z;
#pragma unroll
    for (int j = 0; j < 4; ++j) {
        const int d = d0 + ty + 8 * j, q = q0 + tx;
        tile[ty + 8 * j][tx] = (d < D && q < Q) ? (float)src[(b * D + d) * Q + q] : 0.0f;
    }
    __syncthreads();
#pragma unroll
    for (int j = 0; j < 4; ++j) {
        const int q = q0 + ty + 8 * j, d = d0 + tx;
        if (q < Q && d < Dp) dst[(b * Q + q) * Dp + d] = tile[tx][ty + 8 * j];
    }
}

// in [B][hi wi][Dp] -> out [B][ho wo][Dp], ho = hi >> 1, wo = wi >> 1: one float4 of channels per thread
__global__ __launch_bounds__(ALT_NT) void alt_pool_kernel(const float* __restrict__ in, float* __restrict__ out,
                                                          int B, int hi, int wi, int Dp) {
    const int ho = hi >> 1, wo = wi >> 1, d4 = Dp >> 2;
    const int64_t total = (int64_t)B * ho * wo * d4;
    for (int64_t i = (int64_t)blockIdx.x * ALT_NT + threadIdx.x; i < total; i += (int64_t)gridDim.x * ALT_NT) {
        const int c = (int)(i % d4);
        const int64_t pb = i / d4;
        const int p = (int)(pb % ((int64_t)ho * wo));
        const int64_t b = pb / ((int64_t)ho * wo);
        const int y = p / wo, x = p - y * wo;
        const float4* src = reinterpret_cast<const float4*>(in + (b * hi * wi + (int64_t)(2 * y) * wi + 2 * x) * Dp) + c;
        const float4 v00 = src[0], v01 = src[d4], v10 = src[(int64_t)wi * d4], v11 = src[(int64_t)(wi + 1) * d4];
        float4 r;
        r.x = alt_pool4(v00.x, v01.x, v10.x, v11.x);
        r.y = alt_pool4(v00.y, v01.y, v10.y, v11.y);
        r.z = alt_pool4(v00.z, v01.z, v10.z, v11.z);
        r.w = alt_pool4(v00.w, v01.w, v10.w, v11.w);
        reinterpret_cast<float4*>(out)[i] = r;
    }
}

// ---- the generic path: one sample from its floors and fractions ----------------------------
// The corner value at float floors (fx, fy) of level image lvb ([h w][Dp]) for query vector qv: 0
// outside the image (never read), else the scaled fp32 dot product, an fmaf chain in channel order.
__device__ __forceinline__ float alt_corner(const AltParams& P, const float* __restrict__ qv,
                                            const float* __restrict__ lvb, int h, int w, float fx, float fy) {
    if (!in_image(h, w, fx, fy)) return 0.0f;
    const float* __restrict__ t = lvb + ((int64_t)(int)fy * w + (int)fx) * P.Dp;
    float s = 0.0f;
    for (int d = 0; d < P.Dp; d += 4) {
        const float4 a = *reinterpret_cast<const float4*>(qv + d);
        const float4 v = *reinterpret_cast<const float4*>(t + d);
        s = __builtin_fmaf(a.x, v.x, s);
        s = __builtin_fmaf(a.y, v.y, s);
        s = __builtin_fmaf(a.z, v.z, s);
        s = __builtin_fmaf(a.w, v.w, s);
    }
    return alt_scale(P, s);
}

// The sample of query q of batch item b on level lv at floors (xa, yb), fractions (wa, nb): the volume
// lookup's sample_direct with computed corners.
__device__ __forceinline__ float alt_sample(const AltParams& P, int b, int q, int lv, float xa, float yb, float wa,
                                            float nb) {
    const int h = P.lh[lv], w = P.lw[lv];
    const float* __restrict__ qv = P.f1 + ((int64_t)b * P.Q + q) * P.Dp;
    const float* __restrict__ lvb = P.lvl[lv] + (int64_t)b * h * w * P.Dp;
    const float xa1 = __fadd_rn(xa, 1.0f), yb1 = __fadd_rn(yb, 1.0f);
    return blend(alt_corner(P, qv, lvb, h, w, xa, yb), alt_corner(P, qv, lvb, h, w, xa1, yb),
                 alt_corner(P, qv, lvb, h, w, xa, yb1), alt_corner(P, qv, lvb, h, w, xa1, yb1), wa, nb);
}

// One thread per output element, queries fastest (grid-stride).
__global__ __launch_bounds__(ALT_NT) void alt_generic_kernel(AltParams P, int fmt) {
    const int K = 2 * P.radius + 1, KK = K * K;
    const int64_t total = (int64_t)P.B * P.C * P.Q;
    for (int64_t i = (int64_t)blockIdx.x * ALT_NT + threadIdx.x; i < total; i += (int64_t)gridDim.x * ALT_NT) {
        const int q = (int)(i % P.Q);
        const int64_t bc = i / P.Q;
        const int c = (int)(bc % P.C), b = (int)(bc / P.C);
        const int lv = c / KK, k = c - lv * KK;
        const int a = k / K, bb = k - a * K;
        const float inv = 1.0f / (float)(1 << lv);   // coords / 2**i is an exact scaling
        const float cx = __fmul_rn(P.coords[((int64_t)b * 2 + 0) * P.Q + q], inv);
        const float cy = __fmul_rn(P.coords[((int64_t)b * 2 + 1) * P.Q + q], inv);
        float xa, wa, yb, nb;
        coord_chain(cx, a - P.radius, (float)(P.lw[lv] - 1), xa, wa);
        coord_chain(cy, bb - P.radius, (float)(P.lh[lv] - 1), yb, nb);
        alt_store(P.out, fmt, i, alt_sample(P, b, q, lv, xa, yb, wa, nb));
    }
}

// ---- the window kernel ---------------------------------------------------------------------
template <int R>
struct AltStage {
    static constexpr int K = 2 * R + 1, KK = K * K;
    static constexpr int S = 2 * R + 3, SS = S * S;   // window side: window_fit's span S - 2 plus its slack
    static constexpr int SP = SS | 1;                 // odd per-query stride: lanes = queries hit distinct banks
    static constexpr int NB = (SS + 63) / 64;         // batches of 64 taps
    float grid[ALT_QB * SP];                          // scaled corner values of each query's window, 0 outside
    float fx[ALT_QB][K], wx[ALT_QB][K], fy[ALT_QB][K], wy[ALT_QB][K];
    int org[ALT_QB][3];                               // mode (0 window, 1 generic, 2 past the range), origin x, y
};

// 64 partial-sum arrays (one per lane) -> lane l holds tap l's sum over all lanes.  Stage k exchanges
// half of the live registers with lane ^ k and adds: 63 exchanges and 63 adds in a fixed order.
template <int KS>
__device__ __forceinline__ void alt_reduce_stage(float (&p)[64], int lane) {
    const bool up = (lane & KS) != 0;
#pragma unroll
    for (int i = 0; i < KS; ++i) {
        const float keep = up ? p[i + KS] : p[i];
        const float send = up ? p[i] : p[i + KS];
        p[i] = __fadd_rn(keep, __shfl_xor(send, KS));
    }
}
__device__ __forceinline__ float alt_transpose_reduce(float (&p)[64], int lane) {
    alt_reduce_stage<32>(p, lane);
    alt_reduce_stage<16>(p, lane);
    alt_reduce_stage<8>(p, lane);
    alt_reduce_stage<4>(p, lane);
    alt_reduce_stage<2>(p, lane);
    alt_reduce_stage<1>(p, lane);
    return p[0];
}

// Block = ALT_QB consecutive queries of batch item b on level lv.  Wave wv serves queries 4 wv .. 4 wv + 3
// one after the other: the lanes hold the query vector (a float4 each per 256-channel chunk), every
// needed in-image window pixel is one coalesced buffer load (an offset beyond the level for every
// other tap: 0 without a read, without a branch), four FMAs into that tap's partial sum.
template <int R>
__global__ __launch_bounds__(ALT_NT) void alt_window_kernel(AltParams P, int fmt) {
    using ST = AltStage<R>;
    constexpr int K = ST::K, KK = ST::KK, S = ST::S, SS = ST::SS, SP = ST::SP;
    __shared__ ST st;
    const int tid = threadIdx.x, lane = tid & (kWave - 1), wv = tid / kWave;
    const int nqb = (P.Q + ALT_QB - 1) / ALT_QB;
    const int qb = blockIdx.x % nqb, lb = blockIdx.x / nqb;
    const int lv = lb % P.levels, b = lb / P.levels;
    const int q0 = qb * ALT_QB;
    const int h = P.lh[lv], w = P.lw[lv], Dp = P.Dp, Q = P.Q;
    const float inv = 1.0f / (float)(1 << lv);   // coords / 2**i is an exact scaling
    const __amdgpu_buffer_rsrc_t rsrc = __builtin_amdgcn_make_buffer_rsrc(
        const_cast<float*>(P.lvl[lv] + (int64_t)b * h * w * Dp), 0, (int)((int64_t)h * w * Dp * 4), 0x00020000);

    for (int gi = 0; gi < ALT_QB / 4; ++gi) {
        const int g = wv * (ALT_QB / 4) + gi, q = q0 + g;
        if (q >= Q) {   // wave-uniform
            if (lane == 0) st.org[g][0] = 2;
            continue;
        }
        // the 2 K coordinate chains, one per lane: x offsets in lanes 0 .. K - 1, y offsets in K .. 2 K - 1
        const bool isx = lane < K;
        const int o = isx ? lane : lane - K;
        const float cs = __fmul_rn(P.coords[((int64_t)b * 2 + (isx ? 0 : 1)) * Q + q], inv);
        float f, wgt;
        coord_chain(cs, o - R, (float)((isx ? w : h) - 1), f, wgt);
        if (lane < 2 * K) {
            if (isx) { st.fx[g][o] = f; st.wx[g][o] = wgt; }
            else     { st.fy[g][o] = f; st.wy[g][o] = wgt; }
        }
        const WindowFit wf = window_fit(__shfl(f, 0), __shfl(f, K - 1), __shfl(f, K), __shfl(f, 2 * K - 1), S - 2);
        const int md = __builtin_amdgcn_readfirstlane(wf.md);
        const int x0 = __builtin_amdgcn_readfirstlane(wf.x0), y0 = __builtin_amdgcn_readfirstlane(wf.y0);
        const int nx = __builtin_amdgcn_readfirstlane(wf.nx), ny = __builtin_amdgcn_readfirstlane(wf.ny);
        if (lane == 0) {
            st.org[g][0] = md;
            st.org[g][1] = x0;
            st.org[g][2] = y0;
        }
        if (md != 0) continue;   // NaN / inf / huge: the blend phase takes the generic path

        const float* __restrict__ qv = P.f1 + ((int64_t)b * Q + q) * Dp;
#pragma unroll
        for (int bt = 0; bt < ST::NB; ++bt) {
            float p[64];
#pragma unroll
            for (int t = 0; t < 64; ++t) p[t] = 0.0f;
            for (int c0 = 0; c0 < Dp; c0 += 4 * kWave) {
                const int d = c0 + 4 * lane;
                const bool lok = d < Dp;
                float4 qq = {0.0f, 0.0f, 0.0f, 0.0f};
                if (lok) qq = *reinterpret_cast<const float4*>(qv + d);
#pragma unroll
                for (int tt = 0; tt < 64; ++tt) {
                    const int t = 64 * bt + tt;
                    if (t < SS) {
                        const int j = t / S, i = t - j * S;
                        const int y = y0 + j, x = x0 + i;
                        // only the needed corner rectangle inside the image is read
                        const bool in = j < ny && i < nx && (unsigned)y < (unsigned)h && (unsigned)x < (unsigned)w;
                        const int voff = in && lok ? ((y * w + x) * Dp + d) * 4 : ALT_OOB;
                        const uint4v u = __builtin_amdgcn_raw_buffer_load_b128(rsrc, voff, 0, 0);
                        float s = p[tt];
                        s = __builtin_fmaf(__uint_as_float(u.x), qq.x, s);
                        s = __builtin_fmaf(__uint_as_float(u.y), qq.y, s);
                        s = __builtin_fmaf(__uint_as_float(u.z), qq.z, s);
                        s = __builtin_fmaf(__uint_as_float(u.w), qq.w, s);
                        p[tt] = s;
                    }
                }
            }
            const float sum = alt_transpose_reduce(p, lane);
            const int t = 64 * bt + lane;
            if (t < SS) st.grid[g * SP + t] = alt_scale(P, sum);
        }
    }
    __syncthreads();

    // the blends: each channel's run of queries together (queries fastest)
    for (int idx = tid; idx < KK * ALT_QB; idx += ALT_NT) {
        const int g = idx % ALT_QB, k = idx / ALT_QB;
        const int md = st.org[g][0];
        if (md == 2) continue;
        const int a = k / K, bb = k - a * K;
        const float xa = st.fx[g][a], yb = st.fy[g][bb];
        const float wa = st.wx[g][a], nb = st.wy[g][bb];
        float v;
        if (md == 0) {
            const float* c = st.grid + g * SP + ((int)yb - st.org[g][2]) * S + ((int)xa - st.org[g][1]);
            v = blend(c[0], c[1], c[S], c[S + 1], wa, nb);
        } else {
            v = alt_sample(P, b, q0 + g, lv, xa, yb, wa, nb);
        }
        alt_store(P.out, fmt, ((int64_t)b * P.C + lv * KK + k) * Q + q0 + g, v);
    }
}

template <typename T>
void alt_transpose(const void* src, float* dst, int B, int D, int Dp, int Q, hipStream_t stream) {
    const dim3 grid((unsigned)((Q + 31) / 32), (unsigned)((Dp + 31) / 32), (unsigned)B);
    hipLaunchKernelGGL(alt_transpose_kernel<T>, grid, dim3(ALT_NT), 0, stream, static_cast<const T*>(src), dst, D, Dp, Q);
}

unsigned alt_grid(int64_t threads) {
    return (unsigned)std::min<int64_t>((threads + ALT_NT - 1) / ALT_NT, 8192);
}

}  // namespace

int launch_alt_pack(const void* f1, const void* f2, int fmap_format, int B, int D, int H, int W, const AltGeom& g,
                    float* feat, hipStream_t stream) {
    const int Q = H * W;
    float* l0 = feat + g.off[0];
    if (fmap_format == ECORR_ELEM_F16) {
        alt_transpose<InElem<ECORR_ELEM_F16>::type>(f1, feat, B, D, g.Dp, Q, stream);
        alt_transpose<InElem<ECORR_ELEM_F16>::type>(f2, l0, B, D, g.Dp, Q, stream);
    } else if (fmap_format == ECORR_ELEM_BF16) {
        alt_transpose<InElem<ECORR_ELEM_BF16>::type>(f1, feat, B, D, g.Dp, Q, stream);
        alt_transpose<InElem<ECORR_ELEM_BF16>::type>(f2, l0, B, D, g.Dp, Q, stream);
    } else {
        alt_transpose<float>(f1, feat, B, D, g.Dp, Q, stream);
        alt_transpose<float>(f2, l0, B, D, g.Dp, Q, stream);
    }
    for (int i = 1; i < g.levels; ++i) {
        const int64_t n = (int64_t)B * g.h[i] * g.w[i] * (g.Dp / 4);
        hipLaunchKernelGGL(alt_pool_kernel, dim3(alt_grid(n)), dim3(ALT_NT), 0, stream, feat + g.off[i - 1],
                           feat + g.off[i], B, g.h[i - 1], g.w[i - 1], g.Dp);
    }
    return hip_status();
}

int launch_alt_lookup(const AltParams& P, int out_format, hipStream_t stream) {
    const int64_t nblk = (int64_t)P.B * P.levels * ((P.Q + ALT_QB - 1) / ALT_QB);
    if (P.radius <= 4 && nblk <= 0x7fffffff) {
        const dim3 grid((unsigned)nblk), block(ALT_NT);
        switch (P.radius) {
            case 0: hipLaunchKernelGGL(alt_window_kernel<0>, grid, block, 0, stream, P, out_format); break;
            case 1: hipLaunchKernelGGL(alt_window_kernel<1>, grid, block, 0, stream, P, out_format); break;
            case 2: hipLaunchKernelGGL(alt_window_kernel<2>, grid, block, 0, stream, P, out_format); break;
            case 3: hipLaunchKernelGGL(alt_window_kernel<3>, grid, block, 0, stream, P, out_format); break;
            default: hipLaunchKernelGGL(alt_window_kernel<4>, grid, block, 0, stream, P, out_format); break;
        }
    } else {
        const int64_t n = (int64_t)P.B * P.C * P.Q;
        hipLaunchKernelGGL(alt_generic_kernel, dim3(alt_grid(n)), dim3(ALT_NT), 0, stream, P, out_format);
    }
    return hip_status();
}

}  // namespace ecorr
