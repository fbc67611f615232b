// grad.hip -- backward of the CorrBlock on gfx950 (ecorr_lookup_backward, ecorr_build_backward).
//
// The gradient pyramid G has the pyramid's own storage (ecorr_device.h pix_off), so a query row's
// level images belong to that row alone:
//   lookup_backward_kernel  one workgroup = QB consecutive queries x 1 level (the forward lookup's
//     grid).  The K^2 upstream values of a query are folded into its (2r+3)^2 window in LDS by two
//     separable passes, each LDS cell owned by one thread and summed in a fixed tap order; the window
//     is then added to G with plain loads and stores.  No atomics anywhere: the launches of one
//     block are ordered by the stream, so G is bitwise reproducible.
//   fold_kernel             T_0 = G_0 + 1/4 (G_1 + 1/4 (G_2 + ...)) per level-0 pixel, in place: the
//     chain of avg_pool2d backwards (floor pooling: the dropped last row / column gets no term).
//   build_backward_kernel   grad_fmap = (1/sqrt(D)) fmap x T on v_mfma_f32_32x32x2_f32; a workgroup
//     owns 64 output pixels x all of D and loops over the whole reduction axis (no split-K).
// Stores are plain global stores (DESIGN §3.1 store rule: nothing rides in an SGPR soffset).
#include <math.h>

#include "ecorr_device.h"
#include "ecorr_internal.h"
#include "lookup_grad_window.h"
#include "mfma_f32_frame.h"

namespace ecorr {

namespace {

constexpr int NT = 256;

// ---------------------------------------------------------------------------------------------
// lookup backward
// ---------------------------------------------------------------------------------------------
// Phases 0 - 2 (the tap chains, the window fit, the two separable passes into the LDS window) are
// lookup_grad_window.h grad_window_phases, shared with the volume-free block's backward
// (alt_grad.hip); its header describes the LDS carve.
// RT >= 0: compile-time radius (the tuned r = 4), RT < 0: P.radius.
template <int RT>
__global__ __launch_bounds__(NT) void lookup_backward_kernel(LookupGradParams P, int QB) {
    extern __shared__ float lds[];
    const int r = RT >= 0 ? RT : P.radius;
    const int K = 2 * r + 1, S = K + 2, KK = K * K;
    const int QP = QB + 1;
    const GradWindowLds L = grad_window_carve(lds, K, S, QB);
    const int* org = L.org;
    const float* win = L.win;

    const int tid = threadIdx.x;
    const int lv = blockIdx.y, b = blockIdx.z;
    const int q0 = blockIdx.x * QB;
    const int h = P.lh[lv], w = P.lw[lv];
    const float wm1 = (float)(w - 1), hm1 = (float)(h - 1);
    const float inv = 1.0f / (float)(1 << lv);
    const int64_t Q = P.q_count;
    const float* __restrict__ cxp = P.coords + ((int64_t)b * 2 + 0) * Q;
    const float* __restrict__ cyp = P.coords + ((int64_t)b * 2 + 1) * Q;
    const float* __restrict__ gout = P.grad_out + ((int64_t)b * P.C + (int64_t)lv * KK) * Q;

    grad_window_phases<NT>(L, cxp, cyp, gout, Q, P.q_count, q0, h, w, inv, r, QB);

    // ---- phase 3: G += window.  Each (query, pixel) has one thread; tiled / compact levels walk a
    // query's window row by row (lanes along x), interleaved levels put lanes on adjacent queries
    // (their blocks of one pixel are neighbours in memory).
    float* __restrict__ G = P.lvl[lv];
    const int ntx = P.lntx[lv];
    const int64_t sz = P.lsz[lv];
    const int64_t R0 = (int64_t)b * P.q_count + q0;
    const int nwin = S * S * QB;
    for (int it = tid; it < nwin; it += NT) {
        int g, j, i;
        if (ntx < 0) {
            g = it % QB;
            const int ji = it / QB;
            j = ji / S;
            i = ji - j * S;
        } else {
            i = it % S;
            const int gj = it / S;
            j = gj % S;
            g = gj / S;
        }
        if (org[2 * QB + g] != 0) continue;
        const float v = win[(j * S + i) * QP + g];
        if (v == 0.0f) continue;   // cells no in-range corner touched (and exact zeros: adding them changes nothing)
        const int x = org[g] + i, y = org[QB + g] + j;
        if (x < 0 || x >= w || y < 0 || y >= h) continue;
        float* dst = G + pix_off(R0 + g, y, x, lv, ntx, w, sz);
        *dst = __fadd_rn(*dst, v);
    }

    // ---- serial path: a window the end taps do not bound (NaN, +-inf, huge coordinates: nothing
    // is in range).  One thread walks its query's taps in order, straight on G.
    for (int g = tid; g < QB; g += NT) {
        if (org[2 * QB + g] != 1) continue;
        const float cx = __fmul_rn(cxp[q0 + g], inv), cy = __fmul_rn(cyp[q0 + g], inv);
        for (int a = 0; a < K; ++a) {
            float fx, wx;
            coord_chain(cx, a - r, wm1, fx, wx);
            for (int bb = 0; bb < K; ++bb) {
                float fy, wy;
                coord_chain(cy, bb - r, hm1, fy, wy);
                const float go = gout[(int64_t)(a * K + bb) * Q + q0 + g];
                const float ex = __fsub_rn(1.0f, wx), sy = __fsub_rn(1.0f, wy);
                const float xs[2] = {fx, __fadd_rn(fx, 1.0f)}, ys[2] = {fy, __fadd_rn(fy, 1.0f)};
                const float wxs[2] = {ex, wx}, wys[2] = {sy, wy};
                for (int cy2 = 0; cy2 < 2; ++cy2)
                    for (int cx2 = 0; cx2 < 2; ++cx2) {
                        if (!axis_in(xs[cx2], w) || !axis_in(ys[cy2], h)) continue;
                        float* dst = G + pix_off(R0 + g, (int)ys[cy2], (int)xs[cx2], lv, ntx, w, sz);
                        *dst = __fadd_rn(*dst, __fmul_rn(wys[cy2], __fmul_rn(wxs[cx2], go)));
                    }
            }
        }
    }
}

// ---------------------------------------------------------------------------------------------
// fold: one thread per stored level-0 cell (tile order: coalesced read-modify-write)
// ---------------------------------------------------------------------------------------------
__global__ __launch_bounds__(NT) void fold_kernel(LookupGradParams P, int64_t rows) {
    const int H = P.lh[0], W = P.lw[0], ntx = P.lntx[0];
    const int64_t sz = P.lsz[0];
    const int64_t n = rows * sz;
    for (int64_t idx = blockIdx.x * (int64_t)NT + threadIdx.x; idx < n; idx += (int64_t)gridDim.x * NT) {
        const int64_t R = idx / sz;
        int y, x;
        tiled_cell_yx((int)(idx - R * sz), ntx, y, x);
        if (y >= H || x >= W) continue;
        // coarsest first; a pixel outside level l (floor pooling dropped it) is outside every coarser one
        float t = 0.0f;
        for (int l = P.levels - 1; l >= 1; --l) {
            const int yy = y >> l, xx = x >> l;
            if (yy >= P.lh[l] || xx >= P.lw[l]) continue;
            t = __fadd_rn(P.lvl[l][pix_off(R, yy, xx, l, P.lntx[l], P.lw[l], P.lsz[l])], __fmul_rn(0.25f, t));
        }
        P.lvl[0][idx] = __fadd_rn(P.lvl[0][idx], __fmul_rn(0.25f, t));
    }
}

// ---------------------------------------------------------------------------------------------
// build backward: out[d][n] = (1/sqrt(D)) sum_k op[d][k] T(n, k)
//   F2 = false (grad_fmap1): n = query p of the slab, k = stored level-0 cell c of row b q + p (the
//     padding cells carry zeros), op = fmap2[b][d][pixel of c], T(n, k) = T[b q + n][c]
//   F2 = true  (grad_fmap2): n = stored cell c (outputs of padding cells are dropped), k = query p,
//     op = fmap1[b][d][p], T(n, k) = T[b q + k][n]
// Workgroup = 64 n x all of D, 256 d at a time, on the frame of mfma_f32_frame.h (tile, staging, K loop
// and fragments: A = op, B = T; shared with conv_grad.hip's grad_weight_kernel); the addressing and the
// epilogue are this kernel's.  A chunk of T is whole 128-byte lines either way: 32 consecutive cells of
// one row (one 4 x 8 tile).
// ---------------------------------------------------------------------------------------------
constexpr int GD = kFrameM;   // d rows per pass
constexpr int GN = kFrameN;   // output pixels per workgroup
constexpr int GK = kFrameK;   // reduction chunk

template <bool F2>
__global__ __launch_bounds__(NT) void build_backward_kernel(BuildGradParams P) {
    constexpr int OLD = kFrameLd, TLD = kFrameBLd<F2>;   // T tile: F2 [k][n], else [n][k]
    __shared__ float ol[GD * OLD];
    __shared__ float tl[(F2 ? GK : GN) * TLD];
    const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
    const int b = blockIdx.y;
    const int n0 = blockIdx.x * GN;
    const int H = P.H, W = P.W, D = P.D, ntx = P.ntx;
    const int64_t HW = (int64_t)H * W;
    const int sz = P.sz;                        // stored cells per level-0 image
    const int q = P.q_count;
    const int Kdim = F2 ? q : sz;
    const int Ndim = F2 ? sz : q;
    const float* __restrict__ op = F2 ? P.f1 + (int64_t)b * D * q : P.f2 + (int64_t)b * D * HW;
    const int64_t opld = F2 ? q : HW;
    const float* __restrict__ T = P.T + (int64_t)b * q * sz;
    float* __restrict__ out = F2 ? P.g2 + (int64_t)b * D * HW : P.g1 + (int64_t)b * D * q;
    const int64_t outld = F2 ? HW : q;

    // pixel of a stored cell, or -1 for a padding cell
    auto cell_pixel = [&](int c) -> int {
        if (c >= sz) return -1;
        int y, x;
        tiled_cell_yx(c, ntx, y, x);
        return (y < H && x < W) ? y * W + x : -1;
    };

    const float rs = sqrtf((float)D);
    const int kl = tid & 31, dr = tid >> 5;     // op tile: lane = k, 8 d rows per step
    const int nchunks = (Kdim + GK - 1) / GK;

    for (int d0 = 0; d0 < D; d0 += GD) {
        floatx16 acc[2][2];
        ECORR_FRAME_CLEAR(acc)

        float ro[GD / 8], rt[8];
        auto load_chunk = [&](int kc) {
            const int k = kc * GK + kl;
            int ko;   // element offset of reduction index k in an op row, -1 = zero
            if (F2) ko = k < q ? k : -1;
            else ko = cell_pixel(k);
#pragma unroll
            for (int i = 0; i < GD / 8; ++i) {
                const int d = d0 + dr + 8 * i;
                ro[i] = (ko >= 0 && d < D) ? op[(int64_t)d * opld + ko] : 0.0f;
            }
            if (F2) {   // rows k = kr + 4 i of the chunk, 64 consecutive cells n
                const int nl = tid & 63, kr = tid >> 6;
                const bool nv = cell_pixel(n0 + nl) >= 0;
#pragma unroll
                for (int i = 0; i < 8; ++i) {
                    const int p = kc * GK + kr + 4 * i;
                    rt[i] = (nv && p < q) ? T[(int64_t)p * sz + n0 + nl] : 0.0f;
                }
            } else {    // rows n = nr + 8 i of the block, the chunk's 32 consecutive cells
                const bool kv = ko >= 0;
#pragma unroll
                for (int i = 0; i < 8; ++i) {
                    const int n = n0 + dr + 8 * i;
                    rt[i] = (kv && n < q) ? T[(int64_t)n * sz + k] : 0.0f;
                }
            }
        };
        auto store_chunk = [&]() {
#pragma unroll
            for (int i = 0; i < GD / 8; ++i) ol[(dr + 8 * i) * OLD + kl] = ro[i];
            if (F2) {
                const int nl = tid & 63, kr = tid >> 6;
#pragma unroll
                for (int i = 0; i < 8; ++i) tl[(kr + 4 * i) * TLD + nl] = rt[i];
            } else {
#pragma unroll
                for (int i = 0; i < 8; ++i) tl[(dr + 8 * i) * TLD + kl] = rt[i];
            }
        };

        ECORR_FRAME_K_LOOP(F2, nchunks, ol, tl, lane, wave, acc, load_chunk, store_chunk)

        // epilogue: lane (n, kh) holds column n, rows mfma_c_row(r, kh) of each 32 x 32 tile
        const int kh = lane >> 5;
#pragma unroll
        for (int j = 0; j < 2; ++j) {
            const int n = n0 + 32 * j + (lane & 31);
            int64_t col;
            if (F2) {
                const int pix = n < Ndim ? cell_pixel(n) : -1;
                col = pix;
            } else {
                col = n < Ndim ? n : -1;
            }
            if (col < 0) continue;
#pragma unroll
            for (int i = 0; i < 2; ++i)
#pragma unroll
                for (int r = 0; r < 16; ++r) {
                    const int d = mfma_c_row(r, kh, d0 + 64 * wave + 32 * i);
                    if (d < D) out[(int64_t)d * outld + col] = acc[i][j][r] / rs;
                }
        }
        __syncthreads();   // the next d pass restages LDS
    }
}

}  // namespace

int launch_lookup_backward(const LookupGradParams& P, int B, hipStream_t stream) {
    const int QB = grad_window_queries(P.radius);
    const size_t lds = grad_window_lds_bytes(P.radius, QB);
    const dim3 grid((unsigned)((P.q_count + QB - 1) / QB), (unsigned)P.levels, (unsigned)B);
    if (P.radius == 4) hipLaunchKernelGGL((lookup_backward_kernel<4>), grid, dim3(NT), lds, stream, P, QB);
    else hipLaunchKernelGGL((lookup_backward_kernel<-1>), grid, dim3(NT), lds, stream, P, QB);
    return hip_status();
}

int launch_build_backward(const LookupGradParams& L, const BuildGradParams& P, int B, hipStream_t stream) {
    if (L.levels > 1) {
        const int64_t n = (int64_t)B * P.q_count * P.sz;
        const int64_t g = (n + NT - 1) / NT;
        hipLaunchKernelGGL(fold_kernel, dim3((unsigned)(g < 65536 ? g : 65536)), dim3(NT), 0, stream, L,
                           (int64_t)B * P.q_count);
        const int st = hip_status();
        if (st != ECORR_OK) return st;
    }
    if (P.g1) {
        const dim3 grid((unsigned)((P.q_count + GN - 1) / GN), (unsigned)B);
        hipLaunchKernelGGL((build_backward_kernel<false>), grid, dim3(NT), 0, stream, P);
        const int st = hip_status();
        if (st != ECORR_OK) return st;
    }
    if (P.g2) {
        const dim3 grid((unsigned)((P.sz + GN - 1) / GN), (unsigned)B);
        hipLaunchKernelGGL((build_backward_kernel<true>), grid, dim3(NT), 0, stream, P);
    }
    return hip_status();
}

}  // namespace ecorr
