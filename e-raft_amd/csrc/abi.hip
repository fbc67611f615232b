// abi.hip -- extern "C" entry points of libecorr.so (declared in include/ecorr.h).
//
// Validation mirrors the reference's failure behaviour where it has one (a pyramid level of zero
// pixels raises in avg_pool2d, corr.py:26) and rejects what the C ABI cannot express; nothing
// throws across the boundary.
#include <math.h>

#include "ecorr_device.h"
#include "ecorr_internal.h"

#define ECORR_EXPORT extern "C" __attribute__((visibility("default")))

using namespace ecorr;

namespace ecorr {

int pyramid_geometry(int64_t rows, int H, int W, int levels, PyrGeom* g) {
    if (rows <= 0 || H <= 0 || W <= 0) return ECORR_EINVAL;
    if (levels < 1 || levels > ECORR_MAX_LEVELS) return ECORR_ELEVELS;
    int hh = H, ww = W;
    int64_t o = 0;
    g->levels = levels;
    for (int i = 0; i < levels; ++i) {
        if (i > 0) { hh /= 2; ww /= 2; }
        if (hh == 0 || ww == 0) return ECORR_ESHAPE;
        g->h[i] = hh;
        g->w[i] = ww;
        int64_t nrows = rows;
        if (level_ilv(i)) {   // ecorr_device.h: 2 x 4 / 2 x 4 / 1 x 2 blocks
            const int bh = 1 << ilv_sy(i), bw = 1 << ilv_sx(i);
            const int nby = (hh + bh - 1) / bh, nbx = (ww + bw - 1) / bw;
            g->ntx[i] = -nbx;
            g->nty[i] = nby;
            g->sz[i] = (int64_t)nby * nbx * ilv_bsz(i);
            nrows = (rows + kGroup - 1) / kGroup * kGroup;
        } else if (level_compact(i, hh, ww)) {
            g->ntx[i] = 0;
            g->nty[i] = hh;
            g->sz[i] = (int64_t)hh * ww;
        } else {
            g->ntx[i] = pad_w(ww) / kTileW;
            g->nty[i] = pad_h(hh) / kTileH;
            g->sz[i] = (int64_t)pad_h(hh) * pad_w(ww);
        }
        g->off[i] = o;
        o += nrows * g->sz[i];
        o = (o + kTile - 1) & ~(int64_t)(kTile - 1);   // every level starts on a 128-byte line
    }
    g->off[levels] = o;
    return ECORR_OK;
}

}  // namespace ecorr

namespace {

bool q_count_ok(int H, int W, int q_count) {
    const int64_t Q = (int64_t)H * W;
    return H > 0 && W > 0 && Q <= 0x7fffffff && q_count > 0 && q_count <= Q;
}

}  // namespace

ECORR_EXPORT int ecorr_abi_version(void) { return ECORR_ABI_VERSION; }

ECORR_EXPORT int ecorr_pyramid_tile(int* tile_h, int* tile_w) {
    if (!tile_h || !tile_w) return ECORR_EINVAL;
    *tile_h = kTileH;
    *tile_w = kTileW;
    return ECORR_OK;
}

ECORR_EXPORT const char* ecorr_strerror(int status) {
    switch (status) {
        case ECORR_OK: return "ok";
        case ECORR_EINVAL: return "invalid argument (null pointer, non-positive size or q_count outside [1, H*W])";
        case ECORR_ESHAPE: return "Output size is too small (a pyramid level would be 0 pixels tall or wide)";
        case ECORR_ERADIUS: return "radius out of range [0, 32]";
        case ECORR_ELEVELS: return "num_levels out of range [1, 16]";
        default: break;
    }
    if (status <= ECORR_EHIP) return hipGetErrorString((hipError_t)(ECORR_EHIP - status));
    return "unknown ecorr status";
}

ECORR_EXPORT int ecorr_pyramid_layout(int64_t rows, int H, int W, int levels, int* h, int* w, int64_t* off) {
    PyrGeom g;
    const int st = pyramid_geometry(rows, H, W, levels, &g);
    if (st != ECORR_OK) return st;
    for (int i = 0; i < levels; ++i) {
        if (h) h[i] = g.h[i];
        if (w) w[i] = g.w[i];
        if (off) off[i] = g.off[i];
    }
    if (off) off[levels] = g.off[levels];
    return ECORR_OK;
}

ECORR_EXPORT int ecorr_pyramid_formats(int H, int W, int levels, int* ntx) {
    if (!ntx) return ECORR_EINVAL;
    PyrGeom g;
    const int st = pyramid_geometry(1, H, W, levels, &g);
    if (st != ECORR_OK) return st;
    for (int i = 0; i < levels; ++i) ntx[i] = g.ntx[i];
    return ECORR_OK;
}

namespace {

// The scale step of the build and of the volume-free lookup: corr.py:60 divides by
// torch.sqrt(torch.tensor(dim).float()) (IEEE sqrtf).  When that is a power of two the division is an
// exact scaling and is done as a multiply (*is_mul, *scale = 1 / s, returns shift: s = 2^shift); else *scale = s.
int scale_step_of(int D, float* scale, int* is_mul) {
    const float s = sqrtf((float)D);
    int e = 0;
    *is_mul = frexpf(s, &e) == 0.5f ? 1 : 0;
    *scale = *is_mul ? 1.0f / s : s;
    return *is_mul ? e - 1 : 0;   // s = 0.5 * 2^e
}

// fmap_format (split build): ECORR_ELEM_* of the elements fmap1 / fmap2 point at; hi: workspace is a
// hi workspace (the flag block, then the split workspace)
int build_common(const float* fmap1, const float* fmap2, int B, int D, int H, int W, int q_count, int levels,
                 float* pyramid, void* workspace, void* stream, int stages = 3, int fmap_format = ECORR_ELEM_F32,
                 bool hi = false) {
    if ((stages & 1) && (!fmap1 || !fmap2)) return ECORR_EINVAL;
    if ((stages & 2) && !pyramid) return ECORR_EINVAL;
    if (B <= 0 || D <= 0) return ECORR_EINVAL;
    if (!q_count_ok(H, W, q_count)) return ECORR_EINVAL;
    PyrGeom g;
    const int st = pyramid_geometry((int64_t)B * q_count, H, W, levels, &g);
    if (st != ECORR_OK) return st;

    BuildParams P{};
    P.f1 = fmap1;
    P.f2 = fmap2;
    P.D = D;
    P.H = H;
    P.W = W;
    P.q_count = q_count;
    P.scale_shift = scale_step_of(D, &P.scale, &P.scale_is_mul);
    if (workspace) {
        if (B > 65535 || ((uintptr_t)workspace & 255)) return ECORR_EINVAL;
        P.ws = static_cast<char*>(workspace) + (hi ? kHiFlagBytes : 0);
    }
    return launch_build(P, B, g, pyramid, (hipStream_t)stream, stages, fmap_format, hi);
}

}  // namespace

ECORR_EXPORT int ecorr_build(const float* fmap1, const float* fmap2, int B, int D, int H, int W, int q_count,
                             int levels, float* pyramid, void* stream) {
    return build_common(fmap1, fmap2, B, D, H, W, q_count, levels, pyramid, nullptr, stream);
}

ECORR_EXPORT int ecorr_build_split_workspace_size(int B, int D, int H, int W, int q_count, int64_t* bytes) {
    if (!bytes || B <= 0 || B > 65535 || D <= 0 || !q_count_ok(H, W, q_count)) return ECORR_EINVAL;
    *bytes = build_split_workspace_bytes(B, D, H, W, q_count);
    return ECORR_OK;
}

ECORR_EXPORT int ecorr_build_split(const float* fmap1, const float* fmap2, int B, int D, int H, int W, int q_count,
                                   int levels, float* pyramid, void* workspace, void* stream) {
    if (!workspace) return ECORR_EINVAL;
    return build_common(fmap1, fmap2, B, D, H, W, q_count, levels, pyramid, workspace, stream);
}

ECORR_EXPORT int ecorr_build_split_pack(const float* fmap1, const float* fmap2, int B, int D, int H, int W,
                                        int q_count, void* workspace, void* stream) {
    if (!workspace) return ECORR_EINVAL;
    return build_common(fmap1, fmap2, B, D, H, W, q_count, 1, nullptr, workspace, stream, 1);
}

ECORR_EXPORT int ecorr_build_split_pack_as(const void* fmap1, const void* fmap2, int fmap_format, int B, int D, int H,
                                           int W, int q_count, void* workspace, void* stream) {
    if (!workspace) return ECORR_EINVAL;
    return build_common((const float*)fmap1, (const float*)fmap2, B, D, H, W, q_count, 1, nullptr, workspace, stream, 1,
                        fmap_format);
}

ECORR_EXPORT int ecorr_build_split_as(const void* fmap1, const void* fmap2, int fmap_format, int B, int D, int H, int W,
                                      int q_count, int levels, float* pyramid, void* workspace, void* stream) {
    if (!workspace) return ECORR_EINVAL;
    return build_common((const float*)fmap1, (const float*)fmap2, B, D, H, W, q_count, levels, pyramid, workspace,
                        stream, 3, fmap_format);
}

ECORR_EXPORT int ecorr_build_split_gemm(int B, int D, int H, int W, int q_count, int levels, float* pyramid,
                                        void* workspace, void* stream) {
    if (!workspace) return ECORR_EINVAL;
    return build_common(nullptr, nullptr, B, D, H, W, q_count, levels, pyramid, workspace, stream, 2);
}

ECORR_EXPORT int ecorr_build_split_hi_workspace_size(int B, int D, int H, int W, int q_count, int64_t* bytes) {
    const int st = ecorr_build_split_workspace_size(B, D, H, W, q_count, bytes);
    if (st == ECORR_OK) *bytes += kHiFlagBytes;
    return st;
}

ECORR_EXPORT int ecorr_build_split_pack_hi_as(const void* fmap1, const void* fmap2, int fmap_format, int B, int D,
                                              int H, int W, int q_count, void* workspace, void* stream) {
    if (!workspace) return ECORR_EINVAL;
    return build_common((const float*)fmap1, (const float*)fmap2, B, D, H, W, q_count, 1, nullptr, workspace, stream, 1,
                        fmap_format, true);
}

ECORR_EXPORT int ecorr_build_split_gemm_hi(int B, int D, int H, int W, int q_count, int levels, float* pyramid,
                                           void* workspace, void* stream) {
    if (!workspace) return ECORR_EINVAL;
    return build_common(nullptr, nullptr, B, D, H, W, q_count, levels, pyramid, workspace, stream, 2, ECORR_ELEM_F32,
                        true);
}

ECORR_EXPORT int ecorr_build_split_hi_as(const void* fmap1, const void* fmap2, int fmap_format, int B, int D, int H,
                                         int W, int q_count, int levels, float* pyramid, void* workspace,
                                         void* stream) {
    if (!workspace) return ECORR_EINVAL;
    return build_common((const float*)fmap1, (const float*)fmap2, B, D, H, W, q_count, levels, pyramid, workspace,
                        stream, 3, fmap_format, true);
}

namespace {

int lookup_params(const float* pyramid, const float* coords, int B, int H, int W, int q_count, int levels,
                  int radius, float* out, LookupParams* P) {
    if (!pyramid || !coords || !out || B <= 0) return ECORR_EINVAL;
    if (!q_count_ok(H, W, q_count)) return ECORR_EINVAL;
    if (radius < 0 || radius > 32) return ECORR_ERADIUS;
    PyrGeom g;
    const int st = pyramid_geometry((int64_t)B * q_count, H, W, levels, &g);
    if (st != ECORR_OK) return st;
    if (g.sz[0] > 0x7fffffff) return ECORR_EINVAL;   // the lookup kernels' offsets inside a query image are 32-bit
    level_table<const float>(g, pyramid, P);
    P->coords = coords;
    P->out = out;
    P->H = H;
    P->W = W;
    P->q_count = q_count;
    P->levels = levels;
    P->radius = radius;
    P->C = levels * (2 * radius + 1) * (2 * radius + 1);
    if ((int64_t)B * P->C > 0xffff * 64) return ECORR_EINVAL;
    return ECORR_OK;
}

}  // namespace

ECORR_EXPORT int ecorr_lookup(const float* pyramid, const float* coords, int B, int H, int W, int q_count,
                              int levels, int radius, float* out, void* stream) {
    LookupParams P{};
    const int st = lookup_params(pyramid, coords, B, H, W, q_count, levels, radius, out, &P);
    if (st != ECORR_OK) return st;
    return launch_lookup(P, B, (hipStream_t)stream);
}

ECORR_EXPORT int ecorr_lookup_as(const float* pyramid, const float* coords, int B, int H, int W, int q_count,
                                 int levels, int radius, int out_format, void* out, void* stream) {
    LookupParams P{};
    const int st = lookup_params(pyramid, coords, B, H, W, q_count, levels, radius, (float*)out, &P);
    if (st != ECORR_OK) return st;
    if (out_format != ECORR_OUT_F32 && out_format != ECORR_OUT_F16 && out_format != ECORR_OUT_BF16)
        return ECORR_EINVAL;
    return launch_lookup(P, B, (hipStream_t)stream, out_format);
}

ECORR_EXPORT int ecorr_lookup_qmax(const float* pyramid, const float* coords, int B, int H, int W, int q_count,
                                   int levels, int radius, float* out, float* qmax, void* stream) {
    if (!qmax) return ECORR_EINVAL;
    LookupParams P{};
    const int st = lookup_params(pyramid, coords, B, H, W, q_count, levels, radius, out, &P);
    if (st != ECORR_OK) return st;
    P.qmax = qmax;
    return launch_lookup(P, B, (hipStream_t)stream);
}

namespace {

// radius: the lookup's (the build backward has none: 0)
int grad_params(float* grad_pyramid, int B, int H, int W, int q_count, int levels, int radius, PyrGeom* g,
                LookupGradParams* P) {
    if (!grad_pyramid || B <= 0) return ECORR_EINVAL;
    if (!q_count_ok(H, W, q_count)) return ECORR_EINVAL;
    if (radius < 0 || radius > 32) return ECORR_ERADIUS;
    if (B > 65535) return ECORR_EINVAL;
    const int st = pyramid_geometry((int64_t)B * q_count, H, W, levels, g);
    if (st != ECORR_OK) return st;
    level_table<float>(*g, grad_pyramid, P);
    P->q_count = q_count;
    P->levels = levels;
    return ECORR_OK;
}

}  // namespace

ECORR_EXPORT int ecorr_lookup_backward(const float* grad_out, const float* coords, int B, int H, int W, int q_count,
                                       int levels, int radius, float* grad_pyramid, void* stream) {
    if (!grad_out || !coords) return ECORR_EINVAL;
    PyrGeom g;
    LookupGradParams P{};
    const int st = grad_params(grad_pyramid, B, H, W, q_count, levels, radius, &g, &P);
    if (st != ECORR_OK) return st;
    P.grad_out = grad_out;
    P.coords = coords;
    P.radius = radius;
    P.C = levels * (2 * radius + 1) * (2 * radius + 1);
    return launch_lookup_backward(P, B, (hipStream_t)stream);
}

ECORR_EXPORT int ecorr_build_backward(float* grad_pyramid, const float* fmap1, const float* fmap2, int B, int D, int H,
                                      int W, int q_count, int levels, float* grad_fmap1, float* grad_fmap2,
                                      void* stream) {
    if (!grad_pyramid || !fmap1 || !fmap2 || B <= 0 || D <= 0) return ECORR_EINVAL;
    PyrGeom g;
    LookupGradParams L{};
    const int st = grad_params(grad_pyramid, B, H, W, q_count, levels, 0, &g, &L);
    if (st != ECORR_OK) return st;
    if (g.sz[0] > 0x7fffffff) return ECORR_EINVAL;
    BuildGradParams P{};
    P.T = grad_pyramid + g.off[0];
    P.f1 = fmap1;
    P.f2 = fmap2;
    P.g1 = grad_fmap1;
    P.g2 = grad_fmap2;
    P.D = D;
    P.H = H;
    P.W = W;
    P.q_count = q_count;
    P.ntx = g.ntx[0];
    P.sz = (int)g.sz[0];
    return launch_build_backward(L, P, B, (hipStream_t)stream);
}

ECORR_EXPORT int ecorr_lookup_conv1x1_relu(const float* pyramid, const float* coords, int B, int H, int W,
                                           int q_count, int levels, int radius, const float* weight,
                                           const float* bias, int O, float* out, void* stream) {
    if (!weight) return ECORR_EINVAL;
    LookupParams P{};
    const int st = lookup_params(pyramid, coords, B, H, W, q_count, levels, radius, out, &P);
    if (st != ECORR_OK) return st;
    return launch_lookup_conv(P, B, weight, bias, O, out, (hipStream_t)stream, false);
}

ECORR_EXPORT int ecorr_conv1x1_packed_size(int O, int C, int64_t* floats) {
    if (!floats || O <= 0 || O % 64 != 0 || C <= 0) return ECORR_EINVAL;
    *floats = conv1x1_packed_floats(O, C);
    return ECORR_OK;
}

ECORR_EXPORT int ecorr_conv1x1_pack(const float* weight, int O, int C, float* packed, void* stream) {
    if (!weight || !packed) return ECORR_EINVAL;
    return launch_conv1x1_pack(weight, O, C, packed, (hipStream_t)stream);
}

ECORR_EXPORT int ecorr_lookup_conv1x1_relu_packed(const float* pyramid, const float* coords, int B, int H, int W,
                                                  int q_count, int levels, int radius, const float* packed,
                                                  const float* bias, int O, float* out, void* stream) {
    if (!packed) return ECORR_EINVAL;
    LookupParams P{};
    const int st = lookup_params(pyramid, coords, B, H, W, q_count, levels, radius, out, &P);
    if (st != ECORR_OK) return st;
    return launch_lookup_conv(P, B, packed, bias, O, out, (hipStream_t)stream, true);
}

ECORR_EXPORT int ecorr_lookup_conv1x1_relu_packed_as(const float* pyramid, const float* coords, int B, int H, int W,
                                                     int q_count, int levels, int radius, const float* packed,
                                                     const float* bias, int O, int out_format, void* out,
                                                     void* stream) {
    if (!packed) return ECORR_EINVAL;
    LookupParams P{};
    const int st = lookup_params(pyramid, coords, B, H, W, q_count, levels, radius, (float*)out, &P);
    if (st != ECORR_OK) return st;
    return launch_lookup_conv(P, B, packed, bias, O, (float*)out, (hipStream_t)stream, true, out_format);
}

ECORR_EXPORT int ecorr_conv1x1_split_size(int O, int C, int64_t* bytes) {
    if (!bytes || O <= 0 || C <= 0) return ECORR_EINVAL;
    *bytes = conv1x1_split_bytes(O, C);
    return ECORR_OK;
}

ECORR_EXPORT int ecorr_conv1x1_split_pack(const float* weight, int O, int C, void* packed, void* stream) {
    if (!weight || !packed) return ECORR_EINVAL;
    return launch_conv1x1_split_pack(weight, O, C, packed, (hipStream_t)stream);
}

ECORR_EXPORT int ecorr_conv1x1_relu_split(const float* in, int B, int C, int Q, const float* qmax, int G,
                                          const void* packed, const float* bias, int O, float* out, void* stream) {
    if (!in || !packed || !out) return ECORR_EINVAL;
    return launch_conv1x1_relu_split(in, B, C, Q, qmax, G, packed, bias, O, out, (hipStream_t)stream);
}

ECORR_EXPORT int ecorr_conv1x1_relu_split_as(const float* in, int B, int C, int Q, const float* qmax, int G,
                                             const void* packed, const float* bias, int O, int out_format, void* out,
                                             void* stream) {
    if (!in || !packed || !out) return ECORR_EINVAL;
    return launch_conv1x1_relu_split(in, B, C, Q, qmax, G, packed, bias, O, (float*)out, (hipStream_t)stream,
                                     out_format);
}

ECORR_EXPORT int ecorr_conv1x1_relu_backward_workspace_size(int B, int C, int Q, int O, int64_t* bytes) {
    if (!bytes) return ECORR_EINVAL;
    return conv1x1_relu_backward_workspace_bytes(B, C, Q, O, bytes);
}

ECORR_EXPORT int ecorr_conv1x1_relu_backward(const float* grad_out, const float* out, const float* in,
                                             const void* packed_t, int B, int C, int Q, int O, float* grad_in,
                                             float* grad_weight, float* grad_bias, void* workspace, void* stream) {
    if (!grad_out || !out || !workspace || (!grad_in && !grad_weight && !grad_bias)) return ECORR_EINVAL;
    if ((grad_in && !packed_t) || (grad_weight && !in)) return ECORR_EINVAL;
    if (grad_in && (grad_in == grad_out || grad_in == out || grad_in == in)) return ECORR_EINVAL;
    return launch_conv1x1_relu_backward(grad_out, out, in, packed_t, B, C, Q, O, grad_in, grad_weight, grad_bias,
                                        workspace, (hipStream_t)stream);
}

ECORR_EXPORT int ecorr_split_column_scale(const float* fmap1, const float* fmap2, int B, int D, int H, int W,
                                          int* scale, void* stream) {
    if (!fmap1 || !fmap2 || !scale) return ECORR_EINVAL;
    return launch_split_column_scale(fmap1, fmap2, B, D, H, W, scale, (hipStream_t)stream);
}

ECORR_EXPORT int ecorr_presplit_size(int B, int levels, int q_count, int64_t* bytes) {
    if (!bytes || B <= 0 || q_count <= 0) return ECORR_EINVAL;
    if (levels < 1 || levels > 4) return ECORR_ELEVELS;
    *bytes = (int64_t)B * presplit_bytes_per_item(presplit_positions(levels), q_count);
    return ECORR_OK;
}

ECORR_EXPORT int ecorr_lookup_presplit(const float* pyramid, const float* coords, int B, int H, int W, int q_count,
                                       int levels, int radius, const int* scale, void* out, void* stream) {
    if (!scale || !out) return ECORR_EINVAL;
    if (radius != 4) return ECORR_ERADIUS;
    if (levels < 1 || levels > 4) return ECORR_ELEVELS;
    LookupParams P{};
    const int st = lookup_params(pyramid, coords, B, H, W, q_count, levels, radius, (float*)out, &P);
    if (st != ECORR_OK) return st;
    if (presplit_bytes_per_item(presplit_positions(levels), q_count) >= 0x7fffffffLL)
        return ECORR_EINVAL;   // 32-bit store offsets
    P.scale = scale;
    return launch_lookup(P, B, (hipStream_t)stream);
}

ECORR_EXPORT int ecorr_conv1x1_presplit_size(int O, int levels, int64_t* bytes) {
    if (!bytes || O <= 0) return ECORR_EINVAL;
    if (levels < 1 || levels > 4) return ECORR_ELEVELS;
    *bytes = conv1x1_presplit_bytes(O, levels);
    return ECORR_OK;
}

ECORR_EXPORT int ecorr_conv1x1_split_pack_presplit(const float* weight, int O, int levels, void* packed,
                                                   void* stream) {
    if (!weight || !packed) return ECORR_EINVAL;
    if (levels < 1 || levels > 4) return ECORR_ELEVELS;
    return launch_conv1x1_split_pack(weight, O, 81 * levels, packed, (hipStream_t)stream, levels);
}

ECORR_EXPORT int ecorr_conv1x1_relu_presplit(const void* in, int B, int levels, int Q, const int* scale,
                                             const void* packed, const float* bias, int O, float* out, void* stream) {
    if (!in || !packed || !out || !scale) return ECORR_EINVAL;
    if (levels < 1 || levels > 4) return ECORR_ELEVELS;
    return launch_conv1x1_relu_presplit(in, B, levels, Q, scale, packed, bias, O, out, (hipStream_t)stream);
}

// ---- volume-free correlation (alt.hip) ----
namespace ecorr {

int alt_geometry(int B, int D, int H, int W, int levels, AltGeom* g) {
    if (B < 1 || B > 65535 || D < 1 || H < 1 || W < 1 || (int64_t)H * W > 0x7fffffff) return ECORR_EINVAL;
    if (levels < 1 || levels > ECORR_MAX_LEVELS) return ECORR_EINVAL;
    if (D > 0x7fffffff - 3) return ECORR_EINVAL;
    g->levels = levels;
    g->Dp = (D + 3) & ~3;
    int64_t o = (int64_t)B * H * W * g->Dp;   // fmap1 first
    for (int i = 0; i < levels; ++i) {
        const int hh = H >> i, ww = W >> i;
        if (hh == 0 || ww == 0) return ECORR_EINVAL;
        // the kernels' offsets inside one batch item's level are 32-bit byte offsets
        if ((int64_t)hh * ww * g->Dp * 4 > 0x7fffffff) return ECORR_EINVAL;
        g->h[i] = hh;
        g->w[i] = ww;
        g->off[i] = o;
        o += (int64_t)B * hh * ww * g->Dp;
    }
    g->off[levels] = o;
    return ECORR_OK;
}

}  // namespace ecorr

namespace {

bool elem_format_ok(int f) { return f == ECORR_ELEM_F32 || f == ECORR_ELEM_F16 || f == ECORR_ELEM_BF16; }

// what AltParams and AltGradParams share: the features' level table, the geometry, the scale step
template <class Params>
void alt_fill(Params& P, const float* feat, const float* coords, const AltGeom& g, int B, int D, int H, int W,
              int levels, int radius) {
    P.f1 = feat;
    for (int i = 0; i < levels; ++i) {
        P.lvl[i] = feat + g.off[i];
        P.lh[i] = g.h[i];
        P.lw[i] = g.w[i];
    }
    P.coords = coords;
    P.B = B;
    P.Dp = g.Dp;
    P.Q = H * W;
    P.levels = levels;
    P.radius = radius;
    P.C = levels * (2 * radius + 1) * (2 * radius + 1);
    scale_step_of(D, &P.scale, &P.scale_is_mul);
}

}  // namespace

ECORR_EXPORT int ecorr_alt_size(int B, int D, int H, int W, int levels, int64_t* floats) {
    if (!floats) return ECORR_EINVAL;
    AltGeom g;
    const int st = alt_geometry(B, D, H, W, levels, &g);
    if (st != ECORR_OK) return st;
    *floats = g.off[levels];
    return ECORR_OK;
}

ECORR_EXPORT int ecorr_alt_pack_as(const void* fmap1, const void* fmap2, int fmap_format, int B, int D, int H, int W,
                                   int levels, float* feat, void* stream) {
    if (!fmap1 || !fmap2 || !feat || ((uintptr_t)feat & 15) || !elem_format_ok(fmap_format)) return ECORR_EINVAL;
    AltGeom g;
    const int st = alt_geometry(B, D, H, W, levels, &g);
    if (st != ECORR_OK) return st;
    return launch_alt_pack(fmap1, fmap2, fmap_format, B, D, H, W, g, feat, (hipStream_t)stream);
}

ECORR_EXPORT int ecorr_alt_lookup_as(const float* feat, const float* coords, int B, int D, int H, int W, int levels,
                                     int radius, void* out, int out_format, void* stream) {
    if (!feat || !coords || !out || ((uintptr_t)feat & 15) || !elem_format_ok(out_format)) return ECORR_EINVAL;
    if (radius < 0 || radius > 32) return ECORR_EINVAL;
    AltGeom g;
    const int st = alt_geometry(B, D, H, W, levels, &g);
    if (st != ECORR_OK) return st;
    AltParams P{};
    alt_fill(P, feat, coords, g, B, D, H, W, levels, radius);
    P.out = out;
    return launch_alt_lookup(P, out_format, (hipStream_t)stream);
}

ECORR_EXPORT int ecorr_alt_backward_workspace_size(int B, int H, int W, int levels, int radius, int64_t* bytes) {
    if (!bytes || radius < 0 || radius > 32) return ECORR_EINVAL;
    AltGeom g;
    const int st = alt_geometry(B, 1, H, W, levels, &g);   // the workspace does not depend on D
    if (st != ECORR_OK) return st;
    *bytes = alt_backward_workspace_bytes(B, (int64_t)H * W, levels, radius);
    return ECORR_OK;
}

ECORR_EXPORT int ecorr_alt_lookup_backward(const float* feat, const float* coords, const float* grad_out, int B, int D,
                                           int H, int W, int levels, int radius, float* grad_feat, void* workspace,
                                           void* stream) {
    if (!feat || !coords || !grad_out || !grad_feat || !workspace) return ECORR_EINVAL;
    if (((uintptr_t)feat & 15) || ((uintptr_t)grad_feat & 15) || ((uintptr_t)workspace & 15)) return ECORR_EINVAL;
    if (radius < 0 || radius > 32) return ECORR_EINVAL;
    AltGeom g;
    const int st = alt_geometry(B, D, H, W, levels, &g);
    if (st != ECORR_OK) return st;
    AltGradParams P{};
    alt_fill(P, feat, coords, g, B, D, H, W, levels, radius);
    P.g1 = grad_feat;
    for (int i = 0; i < levels; ++i) {
        P.glvl[i] = grad_feat + g.off[i];
        P.lt0[i + 1] = P.lt0[i] + g.h[i] * g.w[i];
    }
    P.grad_out = grad_out;
    P.org = static_cast<int2*>(workspace);
    P.win = reinterpret_cast<float*>(P.org + (int64_t)B * levels * P.Q);
    return launch_alt_lookup_backward(P, (hipStream_t)stream);
}

ECORR_EXPORT int ecorr_alt_pack_backward(float* grad_feat, int B, int D, int H, int W, int levels, float* grad_fmap1,
                                         float* grad_fmap2, void* stream) {
    if (!grad_feat || ((uintptr_t)grad_feat & 15)) return ECORR_EINVAL;
    AltGeom g;
    const int st = alt_geometry(B, D, H, W, levels, &g);
    if (st != ECORR_OK) return st;
    return launch_alt_pack_backward(grad_feat, B, D, H, W, g, grad_fmap1, grad_fmap2, (hipStream_t)stream);
}

ECORR_EXPORT int ecorr_sepconv_gru_packed_size(int hidden, int input, int64_t* bytes) {
    if (!bytes || !gru_sizes_ok(hidden, input)) return ECORR_EINVAL;
    *bytes = gru_packed_bytes();
    return ECORR_OK;
}

ECORR_EXPORT int ecorr_sepconv_gru_pack(const float* const weight[6], const float* const bias[6], int hidden,
                                        int input, void* packed, void* stream) {
    if (!weight || !bias || !packed || ((uintptr_t)packed & 15) || !gru_sizes_ok(hidden, input)) return ECORR_EINVAL;
    for (int i = 0; i < 6; ++i)
        if (!weight[i] || !bias[i]) return ECORR_EINVAL;
    return launch_gru_pack(weight, bias, packed, (hipStream_t)stream);
}

ECORR_EXPORT int ecorr_sepconv_gru_workspace_size(int B, int hidden, int input, int H, int W, int64_t* bytes) {
    if (!bytes || !gru_sizes_ok(hidden, input) || !gru_geometry_ok(B, H, W)) return ECORR_EINVAL;
    *bytes = gru_workspace_bytes(B, H, W);
    return ECORR_OK;
}

ECORR_EXPORT int ecorr_sepconv_gru(const float* h, const float* x, int B, int hidden, int input, int H, int W,
                                   const void* packed, float* h_out, void* workspace, void* stream) {
    if (!h || !x || !packed || !h_out || !workspace || !gru_sizes_ok(hidden, input) || !gru_geometry_ok(B, H, W))
        return ECORR_EINVAL;
    if (((uintptr_t)packed & 15) || ((uintptr_t)workspace & 15)) return ECORR_EINVAL;
    // h_out overlapping h or x: the second half-step's taps would read what it is writing; the workspace
    // overlapping any of the three: a launch would write h1, z or r*h over what it (or the next) reads
    const uintptr_t n = (uintptr_t)B * H * W * 4;
    auto overlap = [](const void* a, uintptr_t na, const void* b, uintptr_t nb) {
        return (uintptr_t)a < (uintptr_t)b + nb && (uintptr_t)b < (uintptr_t)a + na;
    };
    const uintptr_t nws = (uintptr_t)gru_workspace_bytes(B, H, W);
    if (overlap(h_out, n * hidden, h, n * hidden) || overlap(h_out, n * hidden, x, n * input) ||
        overlap(workspace, nws, h, n * hidden) || overlap(workspace, nws, x, n * input) ||
        overlap(workspace, nws, h_out, n * hidden) || overlap(packed, (uintptr_t)gru_packed_bytes(), workspace, nws) ||
        overlap(packed, (uintptr_t)gru_packed_bytes(), h_out, n * hidden))
        return ECORR_EINVAL;
    return launch_gru(h, x, B, H, W, packed, h_out, workspace, (hipStream_t)stream);
}

ECORR_EXPORT int ecorr_sepconv_gru_backward_packed_size(int hidden, int input, int64_t* bytes) {
    if (!bytes || !gru_sizes_ok(hidden, input)) return ECORR_EINVAL;
    *bytes = gru_packed_t_bytes();
    return ECORR_OK;
}

ECORR_EXPORT int ecorr_sepconv_gru_backward_pack(const float* const weight[6], int hidden, int input, void* packed_t,
                                                 void* stream) {
    if (!weight || !packed_t || ((uintptr_t)packed_t & 15) || !gru_sizes_ok(hidden, input)) return ECORR_EINVAL;
    for (int i = 0; i < 6; ++i)
        if (!weight[i]) return ECORR_EINVAL;
    return launch_gru_pack_t(weight, packed_t, (hipStream_t)stream);
}

ECORR_EXPORT int ecorr_sepconv_gru_backward_workspace_size(int B, int hidden, int input, int H, int W,
                                                           int64_t* bytes) {
    if (!bytes || !gru_sizes_ok(hidden, input) || !gru_geometry_ok(B, H, W)) return ECORR_EINVAL;
    *bytes = gru_backward_workspace_bytes(B, H, W);
    return ECORR_OK;
}

ECORR_EXPORT int ecorr_sepconv_gru_backward(const float* h, const float* x, const float* grad_out, int B, int hidden,
                                            int input, int H, int W, const void* packed, const void* packed_t,
                                            float* grad_h, float* grad_x, float* const grad_weight[6],
                                            float* const grad_bias[6], void* workspace, void* stream) {
    if (!h || !x || !grad_out || !packed || !packed_t || !workspace || !gru_sizes_ok(hidden, input) ||
        !gru_geometry_ok(B, H, W))
        return ECORR_EINVAL;
    if (((uintptr_t)packed & 15) || ((uintptr_t)packed_t & 15) || ((uintptr_t)workspace & 15)) return ECORR_EINVAL;
    if (!grad_weight != !grad_bias) return ECORR_EINVAL;
    if (!grad_h && !grad_x && !grad_weight) return ECORR_EINVAL;   // nothing wanted
    if (grad_weight)
        for (int i = 0; i < 6; ++i)
            if (!grad_weight[i] || !grad_bias[i]) return ECORR_EINVAL;
    // every output disjoint from every input, both packs, the workspace and every other output: the kernels
    // read h, x and the workspace while they write the outputs, and the outputs one after another
    struct Region { const void* p; uintptr_t n; };
    const uintptr_t n = (uintptr_t)B * H * W * 4, nw = (uintptr_t)hidden * (hidden + input) * 5 * 4;
    Region in[6] = {{h, n * hidden}, {x, n * input}, {grad_out, n * hidden}, {packed, (uintptr_t)gru_packed_bytes()},
                    {packed_t, (uintptr_t)gru_packed_t_bytes()},
                    {workspace, (uintptr_t)gru_backward_workspace_bytes(B, H, W)}};
    Region out[14];
    int no = 0;
    if (grad_h) out[no++] = {grad_h, n * hidden};
    if (grad_x) out[no++] = {grad_x, n * input};
    if (grad_weight)
        for (int i = 0; i < 6; ++i) {
            out[no++] = {grad_weight[i], nw};
            out[no++] = {grad_bias[i], (uintptr_t)hidden * 4};
        }
    auto overlap = [](const Region& a, const Region& b) {
        return (uintptr_t)a.p < (uintptr_t)b.p + b.n && (uintptr_t)b.p < (uintptr_t)a.p + a.n;
    };
    for (int i = 0; i < no; ++i) {
        for (int k = 0; k < 6; ++k)
            if (overlap(out[i], in[k])) return ECORR_EINVAL;
        for (int k = 0; k < i; ++k)
            if (overlap(out[i], out[k])) return ECORR_EINVAL;
    }
    // the workspace is written while h, x, grad_out and the packs are read
    for (int k = 0; k < 5; ++k)
        if (overlap(in[5], in[k])) return ECORR_EINVAL;
    return launch_gru_backward(h, x, grad_out, B, H, W, packed, packed_t, grad_h, grad_x, grad_weight, grad_bias,
                               workspace, (hipStream_t)stream);
}

ECORR_EXPORT int ecorr_motion_encoder_packed_size(int64_t* bytes) {
    if (!bytes) return ECORR_EINVAL;
    *bytes = menc_packed_bytes();
    return ECORR_OK;
}

ECORR_EXPORT int ecorr_motion_encoder_pack(const float* const weight[4], const float* const bias[4], void* packed,
                                           void* stream) {
    if (!weight || !bias || !packed || ((uintptr_t)packed & 15)) return ECORR_EINVAL;
    for (int i = 0; i < 4; ++i)
        if (!weight[i] || !bias[i]) return ECORR_EINVAL;
    return launch_menc_pack(weight, bias, packed, (hipStream_t)stream);
}

ECORR_EXPORT int ecorr_motion_encoder_workspace_size(int B, int H, int W, int64_t* bytes) {
    if (!bytes || !menc_geometry_ok(B, H, W)) return ECORR_EINVAL;
    *bytes = menc_workspace_bytes(B, H, W);
    return ECORR_OK;
}

ECORR_EXPORT int ecorr_motion_encoder(const float* c1, const float* flow, int B, int H, int W, const void* packed,
                                      float* out, int64_t out_batch_stride, void* workspace, void* stream) {
    if (!c1 || !flow || !packed || !out || !workspace || !menc_geometry_ok(B, H, W)) return ECORR_EINVAL;
    if (((uintptr_t)packed & 15) || ((uintptr_t)workspace & 15)) return ECORR_EINVAL;
    const int64_t hw = (int64_t)H * W;
    if (out_batch_stride < 128 * hw || out_batch_stride > (int64_t)1 << 40) return ECORR_EINVAL;
    // out's whole strided extent (the gaps between its batch items included) disjoint from everything the
    // launches read, and the workspace (cor, f1, flo: written and read back) from the inputs and the pack
    auto overlap = [](const void* a, uintptr_t na, const void* b, uintptr_t nb) {
        return (uintptr_t)a < (uintptr_t)b + nb && (uintptr_t)b < (uintptr_t)a + na;
    };
    const uintptr_t n = (uintptr_t)B * hw * 4, nc1 = n * 256, nfl = n * 2;
    const uintptr_t nout = ((uintptr_t)(B - 1) * out_batch_stride + 128 * hw) * 4;
    const uintptr_t nws = (uintptr_t)menc_workspace_bytes(B, H, W), npk = (uintptr_t)menc_packed_bytes();
    if (overlap(out, nout, c1, nc1) || overlap(out, nout, flow, nfl) || overlap(out, nout, packed, npk) ||
        overlap(out, nout, workspace, nws) || overlap(workspace, nws, c1, nc1) || overlap(workspace, nws, flow, nfl) ||
        overlap(workspace, nws, packed, npk))
        return ECORR_EINVAL;
    return launch_menc(c1, flow, B, H, W, packed, out, out_batch_stride, workspace, (hipStream_t)stream);
}

ECORR_EXPORT int ecorr_motion_encoder_backward_packed_size(int64_t* bytes) {
    if (!bytes) return ECORR_EINVAL;
    *bytes = menc_packed_t_bytes();
    return ECORR_OK;
}

ECORR_EXPORT int ecorr_motion_encoder_backward_pack(const float* const weight[4], void* packed_t, void* stream) {
    if (!weight || !packed_t || ((uintptr_t)packed_t & 15)) return ECORR_EINVAL;
    for (int i = 0; i < 4; ++i)
        if (!weight[i]) return ECORR_EINVAL;
    return launch_menc_pack_t(weight, packed_t, (hipStream_t)stream);
}

ECORR_EXPORT int ecorr_motion_encoder_backward_workspace_size(int B, int H, int W, int64_t* bytes) {
    if (!bytes || !menc_geometry_ok(B, H, W)) return ECORR_EINVAL;
    *bytes = menc_backward_workspace_bytes(B, H, W);
    return ECORR_OK;
}

ECORR_EXPORT int ecorr_motion_encoder_backward(const float* c1, const float* flow, const float* grad_out,
                                               int64_t grad_out_batch_stride, int B, int H, int W, const void* packed,
                                               const void* packed_t, float* grad_c1, float* grad_flow,
                                               float* const grad_weight[4], float* const grad_bias[4], void* workspace,
                                               void* stream) {
    if (!c1 || !flow || !grad_out || !packed || !packed_t || !workspace || !menc_geometry_ok(B, H, W))
        return ECORR_EINVAL;
    if (((uintptr_t)packed & 15) || ((uintptr_t)packed_t & 15) || ((uintptr_t)workspace & 15)) return ECORR_EINVAL;
    const int64_t hw = (int64_t)H * W;
    if (grad_out_batch_stride < 128 * hw || grad_out_batch_stride > (int64_t)1 << 40) return ECORR_EINVAL;
    if (!grad_weight != !grad_bias) return ECORR_EINVAL;
    if (!grad_c1 && !grad_flow && !grad_weight) return ECORR_EINVAL;   // nothing wanted
    if (grad_weight)
        for (int i = 0; i < 4; ++i)
            if (!grad_weight[i] || !grad_bias[i]) return ECORR_EINVAL;
    // every output disjoint from every input (grad_out's whole strided extent, the gaps between its batch items
    // included), both packs, the workspace and every other output; the workspace from what is read while it is written
    struct Region { const void* p; uintptr_t n; };
    const uintptr_t n = (uintptr_t)B * hw * 4;
    static const uintptr_t wn[4] = {192 * 256 * 9, 128 * 2 * 49, 64 * 128 * 9, 126 * 256 * 9}, bn[4] = {192, 128, 64, 126};
    Region in[6] = {{c1, n * 256}, {flow, n * 2},
                    {grad_out, ((uintptr_t)(B - 1) * grad_out_batch_stride + 128 * hw) * 4},
                    {packed, (uintptr_t)menc_packed_bytes()}, {packed_t, (uintptr_t)menc_packed_t_bytes()},
                    {workspace, (uintptr_t)menc_backward_workspace_bytes(B, H, W)}};
    Region out[10];
    int no = 0;
    if (grad_c1) out[no++] = {grad_c1, n * 256};
    if (grad_flow) out[no++] = {grad_flow, n * 2};
    if (grad_weight)
        for (int i = 0; i < 4; ++i) {
            out[no++] = {grad_weight[i], wn[i] * 4};
            out[no++] = {grad_bias[i], bn[i] * 4};
        }
    auto overlap = [](const Region& a, const Region& b) {
        return (uintptr_t)a.p < (uintptr_t)b.p + b.n && (uintptr_t)b.p < (uintptr_t)a.p + a.n;
    };
    for (int i = 0; i < no; ++i) {
        for (int k = 0; k < 6; ++k)
            if (overlap(out[i], in[k])) return ECORR_EINVAL;
        for (int k = 0; k < i; ++k)
            if (overlap(out[i], out[k])) return ECORR_EINVAL;
    }
    for (int k = 0; k < 5; ++k)
        if (overlap(in[5], in[k])) return ECORR_EINVAL;
    return launch_menc_backward(c1, flow, grad_out, grad_out_batch_stride, B, H, W, packed, packed_t, grad_c1, grad_flow,
                                grad_weight, grad_bias, workspace, (hipStream_t)stream);
}

ECORR_EXPORT int ecorr_bilinear_sampler(const float* img, int N, int C, int h, int w, const float* coords,
                                        int Hg, int Wg, float* out, float* mask, void* stream) {
    if (!img || !coords || !out || N <= 0 || C < 0 || h <= 0 || w <= 0 || Hg <= 0 || Wg <= 0)
        return ECORR_EINVAL;
    return launch_bilinear_sampler(img, N, C, h, w, coords, Hg, Wg, out, mask, (hipStream_t)stream);
}

ECORR_EXPORT int ecorr_coords_grid(int B, int H, int W, float* out, void* stream) {
    if (!out || B <= 0 || H <= 0 || W <= 0) return ECORR_EINVAL;
    return launch_coords_grid(B, H, W, out, (hipStream_t)stream);
}

ECORR_EXPORT int ecorr_rows_assemble(const float* chunks, int64_t chunk, int world, int B, int C, int H, int W,
                                     float* out, void* stream) {
    if (!chunks || !out || world < 1 || B <= 0 || C <= 0 || H < world || W <= 0) return ECORR_EINVAL;
    const int64_t rows_max = H / world + (H % world ? 1 : 0);
    if (chunk < (int64_t)B * C * rows_max * W || (int64_t)B * C > 0x7fffffff) return ECORR_EINVAL;
    return launch_rows_assemble(chunks, chunk, world, B, C, H, W, out, (hipStream_t)stream);
}

namespace {

bool splat_dims_ok(int B, int64_t n, int h, int w) {
    return B > 0 && n >= 0 && n < (1 << 24) && h > 0 && w > 0 && (int64_t)h * w <= 0x7fffffff;
}

}  // namespace

ECORR_EXPORT int ecorr_splat_workspace_size(int B, int64_t n, int h, int w, int64_t* bytes) {
    if (!bytes || !splat_dims_ok(B, n, h, w)) return ECORR_EINVAL;
    *bytes = splat_workspace_bytes(B, n, h, w);
    return ECORR_OK;
}

ECORR_EXPORT int ecorr_forward_interpolate(const float* flow, int B, int h, int w, float* out, void* workspace,
                                           void* stream) {
    const int64_t n = (int64_t)h * w;
    if (!flow || !out || !splat_dims_ok(B, n, h, w)) return ECORR_EINVAL;
    if (!workspace && splat_workspace_bytes(B, n, h, w) > 0) return ECORR_EINVAL;
    return launch_splat(true, flow, B, n, h, w, out, nullptr, workspace, (hipStream_t)stream);
}

ECORR_EXPORT int ecorr_grid_sample_values(const float* pts, int64_t n, int h, int w, float* values, uint8_t* valid,
                                          void* workspace, void* stream) {
    if (!values || (!pts && n > 0) || !splat_dims_ok(1, n, h, w)) return ECORR_EINVAL;
    if (!workspace && splat_workspace_bytes(1, n, h, w) > 0) return ECORR_EINVAL;
    return launch_splat(false, pts, 1, n, h, w, values, valid, workspace, (hipStream_t)stream);
}

namespace {

// the upsampling kernels' limits: N rides a 16-bit grid axis, and 8 * H * W stays an int
bool upsample_dims_ok(int N, int H, int W) {
    return N > 0 && N <= 65535 && H > 0 && W > 0 && (int64_t)H * W <= (1 << 26);
}

}  // namespace

ECORR_EXPORT int ecorr_upsample_flow(const float* flow, const float* mask, int N, int H, int W, float* out,
                                     void* stream) {
    if (!flow || !mask || !out || !upsample_dims_ok(N, H, W)) return ECORR_EINVAL;
    if ((uintptr_t)out & 15) return ECORR_EINVAL;   // upsample_kernel stores out as 16-byte vectors
    return launch_upsample_flow(flow, mask, N, H, W, out, (hipStream_t)stream);
}

ECORR_EXPORT int ecorr_upsample_backward_workspace_size(int N, int H, int W, int64_t* bytes) {
    if (!bytes || !upsample_dims_ok(N, H, W)) return ECORR_EINVAL;
    *bytes = upsample_backward_workspace_bytes(N, H, W);
    return ECORR_OK;
}

ECORR_EXPORT int ecorr_upsample_flow_backward(const float* grad_out, const float* flow, const float* mask, int N,
                                              int H, int W, float* grad_flow, float* grad_mask, void* workspace,
                                              void* stream) {
    if (!grad_out || !flow || !mask || (!grad_flow && !grad_mask) || !upsample_dims_ok(N, H, W)) return ECORR_EINVAL;
    if (!workspace && upsample_backward_workspace_bytes(N, H, W) > 0) return ECORR_EINVAL;
    if ((uintptr_t)grad_out & 15) return ECORR_EINVAL;   // upsample_backward_kernel loads grad_out as 16-byte vectors
    return launch_upsample_flow_backward(grad_out, flow, mask, N, H, W, grad_flow, grad_mask, workspace,
                                         (hipStream_t)stream);
}

ECORR_EXPORT int ecorr_flow_to_png16(const float* flow, int B, int h, int w, uint16_t* out, void* stream) {
    if (!flow || !out || B <= 0 || h <= 0 || w <= 0) return ECORR_EINVAL;
    return launch_png16_encode(flow, B, h, w, out, (hipStream_t)stream);
}

ECORR_EXPORT int ecorr_png16_to_flow(const uint16_t* in, int B, int h, int w, float* flow, uint8_t* valid, int* bad,
                                     void* stream) {
    if (!in || !flow || !valid || !bad || B <= 0 || h <= 0 || w <= 0) return ECORR_EINVAL;
    return launch_png16_decode(in, B, h, w, flow, valid, bad, (hipStream_t)stream);
}

namespace {

bool voxel_dims_ok(int64_t n, int C, int H, int W) {
    // keys (extended grid for DSEC) must stay below 2^32 - 1; event indices are int32
    return n >= 1 && n <= 0x7fffffff && C > 0 && H > 0 && W > 0 &&
           (int64_t)(C + 1) * (H + 1) * (W + 1) < 0xffffffffLL;
}

}  // namespace

ECORR_EXPORT int ecorr_voxel_workspace_size(int dsec, int64_t n, int C, int H, int W, int64_t* bytes) {
    if (!bytes || !voxel_dims_ok(n, C, H, W)) return ECORR_EINVAL;
    return voxel_workspace_bytes(dsec != 0, n, C, H, W, bytes);
}

ECORR_EXPORT int ecorr_voxel_grid_dsec(const float* p, const float* t, const float* x, const float* y, int64_t n,
                                       int C, int H, int W, int normalize, float* voxel, void* workspace,
                                       void* stream) {
    if (!p || !t || !x || !y || !voxel || !workspace || !voxel_dims_ok(n, C, H, W)) return ECORR_EINVAL;
    return launch_voxel(true, p, t, x, y, nullptr, n, C, H, W, normalize, voxel, nullptr, workspace,
                        (hipStream_t)stream);
}

ECORR_EXPORT int ecorr_voxel_grid_mvsec(const double* events, int64_t n, int C, int H, int W, int normalize,
                                        float* voxel, int* bad_index, void* workspace, void* stream) {
    if (!events || !voxel || !bad_index || !workspace || !voxel_dims_ok(n, C, H, W)) return ECORR_EINVAL;
    return launch_voxel(false, nullptr, nullptr, nullptr, nullptr, events, n, C, H, W, normalize, voxel, bad_index,
                        workspace, (hipStream_t)stream);
}
