// lookup_grad_window.h -- the window gradient of a lookup's backward: the one definition that both
// backward kernels call (grad.hip lookup_backward_kernel, which adds the window to the gradient
// pyramid, and alt_grad.hip alt_window_grad_kernel, which writes it to the workspace).
//
// A workgroup of NT threads serves QB consecutive queries of one batch item on one level.  The K^2
// upstream values of a query are folded into its (2r+3)^2 window in LDS by two separable passes, each
// LDS cell owned by one thread and summed in a fixed tap order.  The tap chains, the window fit and the
// in-range test are the forward's own (ecorr_device.h coord_chain, window_fit, axis_in): the
// backward's support is the forward's by construction.
//
// LDS (floats), g = query of the block innermost so that lanes = queries never share a bank:
//   cf / cw [K][QB]      floor (as float) and fraction of the current axis' K taps
//   org     [3][QB]      window origin x, y and mode (0 window, 1 serial, 2 no query) as ints
//   tmp     [K][S][QB]   x pass: row bb of the upstream summed into the S window columns
//   win     [S][S][QB+1] the window gradient
#pragma once
#include "ecorr_device.h"

namespace ecorr {

struct GradWindowLds {
    float* cf;
    float* cw;
    int* org;
    float* tmp;
    float* win;
};

__device__ __forceinline__ GradWindowLds grad_window_carve(float* lds, int K, int S, int QB) {
    GradWindowLds L;
    L.cf = lds;
    L.cw = L.cf + K * QB;
    L.org = reinterpret_cast<int*>(L.cw + K * QB);
    L.tmp = reinterpret_cast<float*>(L.org + 3 * QB);
    L.win = L.tmp + K * S * QB;
    return L;
}

// LDS bytes of the carve for QB queries at radius r
inline size_t grad_window_lds_bytes(int r, int QB) {
    const size_t K = 2 * r + 1, S = K + 2;
    return (2 * K * QB + 3 * QB + K * S * QB + S * S * (QB + 1)) * sizeof(float);
}
// as many queries per workgroup as fit 64 KB of LDS (64 at r <= 4, 1 at r = 32)
inline int grad_window_queries(int r) {
    int QB = 64;
    while (QB > 1 && grad_window_lds_bytes(r, QB) > 64 * 1024) QB >>= 1;
    return QB;
}

// Phases 0 - 2 for queries q0 .. q0 + QB - 1 (those below q_count) of the level h x w, inv = 2^-level:
// cxp / cyp the batch item's coordinate rows, gout its upstream rows of this level ([K^2][Q], row
// stride Q).  On return (after a barrier) L.win holds the windows and L.org the origins and modes;
// L.cf / L.cw hold the y chains.
template <int NT>
__device__ __forceinline__ void grad_window_phases(const GradWindowLds& L, const float* __restrict__ cxp,
                                                   const float* __restrict__ cyp, const float* __restrict__ gout,
                                                   int64_t Q, int q_count, int q0, int h, int w, float inv, int r,
                                                   int QB) {
    const int K = 2 * r + 1, S = K + 2;
    const int QP = QB + 1;
    float* cf = L.cf;
    float* cw = L.cw;
    int* org = L.org;
    float* tmp = L.tmp;
    float* win = L.win;
    const int tid = threadIdx.x;
    const float wm1 = (float)(w - 1), hm1 = (float)(h - 1);

    // ---- phase 0: the x chains, the window origin from the end taps of both axes, zeroed LDS
    for (int i = tid; i < K * QB; i += NT) {
        const int g = i % QB, o = i / QB;
        float f = 0.0f, wg = 0.0f;
        if (q0 + g < q_count) coord_chain(__fmul_rn(cxp[q0 + g], inv), o - r, wm1, f, wg);
        cf[o * QB + g] = f;
        cw[o * QB + g] = wg;
    }
    for (int g = tid; g < QB; g += NT) {
        int md = 2, X0 = 0, Y0 = 0;
        if (q0 + g < q_count) {
            const float cx = __fmul_rn(cxp[q0 + g], inv), cy = __fmul_rn(cyp[q0 + g], inv);
            float x0, xl, y0, yl, d;
            coord_chain(cx, -r, wm1, x0, d);
            coord_chain(cx, r, wm1, xl, d);
            coord_chain(cy, -r, hm1, y0, d);
            coord_chain(cy, r, hm1, yl, d);
            const WindowFit f = window_fit(x0, xl, y0, yl, S - 2);
            md = f.md, X0 = f.x0, Y0 = f.y0;   // md 1: the serial path
        }
        org[0 * QB + g] = X0;
        org[1 * QB + g] = Y0;
        org[2 * QB + g] = md;
    }
    for (int i = tid; i < K * S * QB; i += NT) tmp[i] = 0.0f;
    for (int i = tid; i < S * S * QP; i += NT) win[i] = 0.0f;
    __syncthreads();

    // ---- phase 1 (x pass): thread = (query g, tap row bb); taps a = 0 .. K-1 in order:
    //   tmp[bb][fx_a - X0] += (1 - wx_a) g[a][bb],  tmp[bb][fx_a + 1 - X0] += wx_a g[a][bb]
    // for the corners whose x is inside the level.  Upstream reads: lanes = consecutive queries.
    for (int i = tid; i < K * QB; i += NT) {
        const int g = i % QB, bb = i / QB;
        if (org[2 * QB + g] != 0) continue;
        const int X0 = org[g];
        float* row = tmp + (bb * S) * QB + g;
        const float* gp = gout + q0 + g;
#pragma unroll 3
        for (int a = 0; a < K; ++a) {
            const float go = gp[(int64_t)(a * K + bb) * Q];
            const float f = cf[a * QB + g], wx = cw[a * QB + g];
            const int ci = (int)f - X0;
            if ((unsigned)ci > (unsigned)(S - 2)) continue;   // never: the end taps bound the window
            if (axis_in(f, w)) row[ci * QB] = __fadd_rn(row[ci * QB], __fmul_rn(__fsub_rn(1.0f, wx), go));
            if (axis_in(__fadd_rn(f, 1.0f), w))
                row[(ci + 1) * QB] = __fadd_rn(row[(ci + 1) * QB], __fmul_rn(wx, go));
        }
    }
    __syncthreads();
    // ---- the y chains replace the x chains
    for (int i = tid; i < K * QB; i += NT) {
        const int g = i % QB, o = i / QB;
        float f = 0.0f, wg = 0.0f;
        if (q0 + g < q_count) coord_chain(__fmul_rn(cyp[q0 + g], inv), o - r, hm1, f, wg);
        cf[o * QB + g] = f;
        cw[o * QB + g] = wg;
    }
    __syncthreads();
    // ---- phase 2 (y pass): thread = (query g, window column i); taps bb = 0 .. K-1 in order
    for (int it = tid; it < S * QB; it += NT) {
        const int g = it % QB, i = it / QB;
        if (org[2 * QB + g] != 0) continue;
        const int Y0 = org[QB + g];
        float* col = win + i * QP + g;
        for (int bb = 0; bb < K; ++bb) {
            const float t = tmp[(bb * S + i) * QB + g];
            const float f = cf[bb * QB + g], wy = cw[bb * QB + g];
            const int ri = (int)f - Y0;
            if ((unsigned)ri > (unsigned)(S - 2)) continue;
            if (axis_in(f, h)) col[ri * S * QP] = __fadd_rn(col[ri * S * QP], __fmul_rn(__fsub_rn(1.0f, wy), t));
            if (axis_in(__fadd_rn(f, 1.0f), h))
                col[(ri + 1) * S * QP] = __fadd_rn(col[(ri + 1) * S * QP], __fmul_rn(wy, t));
        }
    }
    __syncthreads();
}

}  // namespace ecorr
