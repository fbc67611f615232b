"""Cases, inputs and a plain fp64 reference of the convex upsampling's forward (upsample_kernel,
csrc/upsample.hip): test infrastructure, numpy only.  Shared by tests/test_flow_ref.py (on the CPU: the
reference against the committed goldens and against ERAFT.upsample_flow in fp64) and
tests/test_flow_edges_gpu.py.

The kernel's thread is (n, sub-row i, pixel p = h * W + w) in 256-thread blocks over p; it leaves early
for p >= H * W, gathers the zero-padded 3 x 3 window of 8 * flow, and stores 8 sub-pixels j as two
16-byte vectors per channel.  Each shape below reaches one thing that can go wrong there.
"""
import numpy as np

import prng

NTU = 256   # csrc/upsample.hip: pixels per block of upsample_kernel
UPSAMPLE_TOL = 2e-6   # the project's bar for the kernel: max|got - ref| / rms(ref) (tests/test_flow_gpu.py)

# (N, H, W): what it reaches
SHAPES = {
    (1, 1, 1): "every off-centre tap is padding",
    (1, 1, 7): "one row: two of three tap rows are padding everywhere",
    (1, 6, 1): "one column: two of three tap columns are padding everywhere",
    (2, 1, 300): "one row with a block boundary inside the map and a batch offset",
    (2, 300, 1): "one column with a block boundary inside the map and a batch offset",
    (3, 5, 53): "HW = 265: the block boundary falls mid-row, a 9-thread tail, three items",
    (2, 16, 16): "exactly one full block, no tail",
    (1, 17, 31): "odd sides, HW = 527: two full blocks and a 15-thread tail",
}
SCALES = (1.0, 20.0)   # the mask's: ordinary logits, and near one-hot
CASES = [(N, H, W, ms) for (N, H, W) in SHAPES for ms in SCALES]

_cache = {}


def _frozen(key, make):
    if key not in _cache:
        arrs = make()
        for a in arrs:
            a.setflags(write=False)
        _cache[key] = arrs
    return _cache[key]


def inputs(N, H, W, ms):
    """(flow [N, 2, H, W], mask [N, 576, H, W]) float32, read-only, made once."""
    seed = 9000 + 1000 * N + 13 * H + W + (500 if ms > 1.0 else 0)
    return _frozen(("in", N, H, W, ms), lambda: (prng.normal(seed, (N, 2, H, W), 3.0),
                                                 prng.normal(seed + 1, (N, 576, H, W), ms)))


def reference(flow, mask, with_scale=False):
    """ERAFT.upsample_flow in fp64 from explicit indices -> float64 [N, 2, 8H, 8W]:

        out[n, c, 8h + i, 8w + j] = sum_k softmax_k(mask[n, k*64 + i*8 + j, h, w]) * P[n, c, h + ky, w + kx]

    with k = 3 ky + kx ascending and P = 8 * flow inside a one-pixel border of zeros.  The loops run over
    (c, i, j, k); each statement is an array over (n, h, w).  with_scale: also A [N, 2, 8H, 8W] =
    sum_k s_k (20 + d_k) |P_k| with d_k = max - logit_k, the element's error scale: a floating-point
    evaluation with unit roundoff u in any order is within u * A of the exact value to first order (per
    weight d_k u from rounding logit - max ahead of exp, 2 u for exp, 8 u for the sum of 9 weights, u for
    the division, u for the product, 8 u for the sum of 9 products).  The test's own arithmetic; nothing
    of the view / unfold / permute expression."""
    flow = np.asarray(flow, dtype=np.float64)
    mask = np.asarray(mask, dtype=np.float64)
    N, _, H, W = flow.shape
    assert flow.shape == (N, 2, H, W) and mask.shape == (N, 576, H, W)
    P = np.zeros((N, 2, H + 2, W + 2), dtype=np.float64)
    P[:, :, 1:H + 1, 1:W + 1] = 8.0 * flow
    out = np.empty((N, 2, 8 * H, 8 * W), dtype=np.float64)
    A = np.empty_like(out) if with_scale else None
    with np.errstate(invalid="ignore"):   # non-finite logits give NaN, as the softmax does
        for i in range(8):
            for j in range(8):
                logit = [mask[:, k * 64 + i * 8 + j] for k in range(9)]
                mx = logit[0]
                for k in range(1, 9):
                    mx = np.maximum(mx, logit[k])   # propagates a NaN, as ATen's max
                e = [np.exp(logit[k] - mx) for k in range(9)]
                s = e[0]
                for k in range(1, 9):
                    s = s + e[k]
                for c in range(2):
                    acc = np.zeros((N, H, W), dtype=np.float64)
                    a = np.zeros((N, H, W), dtype=np.float64)
                    for k in range(9):
                        ky, kx = k // 3, k % 3
                        tap = P[:, c, ky:ky + H, kx:kx + W]
                        acc = acc + (e[k] / s) * tap
                        if with_scale:
                            a = a + (e[k] / s) * (20.0 + (mx - logit[k])) * np.abs(tap)
                    out[:, c, i::8, j::8] = acc
                    if with_scale:
                        A[:, c, i::8, j::8] = a
    return (out, A) if with_scale else out


def case(N, H, W, ms):
    """(flow, mask, out64), read-only, the reference computed once."""
    def make():
        flow, mask = inputs(N, H, W, ms)
        return flow, mask, reference(flow, mask)
    return _frozen(("case", N, H, W, ms), make)


def onehot(N, H, W, low):
    """(flow, mask, want): per (n, h, w, i, j) one tap drawn from prng.uniform has logit 0 and the other
    eight `low` (-inf, or -120: exp is exactly 0 in fp32 either way), so the softmax is exactly one-hot
    and want [N, 2, 8H, 8W] float32 is 8 * flow of the selected neighbour, +0.0 where it is padding
    (an in-order sum that starts at +0 and adds +-0 products and one value)."""
    def make():
        flow = inputs(N, H, W, 1.0)[0]
        pick = np.minimum((prng.uniform(9900 + 13 * H + W, (N, 8, 8, H, W)) * 9.0).astype(np.int64), 8)
        mask = np.full((N, 9, 8, 8, H, W), low, dtype=np.float32)
        np.put_along_axis(mask, pick[:, None], np.float32(0.0), axis=1)
        want = np.zeros((N, 2, 8 * H, 8 * W), dtype=np.float32)
        f8 = np.float32(8.0) * flow
        for n in range(N):
            for h in range(H):
                for w in range(W):
                    for i in range(8):
                        for j in range(8):
                            k = int(pick[n, i, j, h, w])
                            y, x = h + k // 3 - 1, w + k % 3 - 1
                            if 0 <= y < H and 0 <= x < W:
                                want[n, :, 8 * h + i, 8 * w + j] = f8[n, :, y, x]
        return flow, np.ascontiguousarray(mask.reshape(N, 576, H, W)), want, pick
    return _frozen(("onehot", N, H, W, low), make)


# ---- the codec ----------------------------------------------------------------------------------------

CODEC_PASS = 16384 * NTU   # grid_for() (csrc/upsample.hip): at most 16384 blocks of NTU threads, so one
                           # pass of the codec's grid-stride loops covers 4,194,304 pixels
CODEC_LARGE_W = 2048
CODEC_LARGE_H = CODEC_PASS // CODEC_LARGE_W + 1   # the first whole row past one pass
# tests/golden/make_golden_next.py's special values of the encoder
ENC_SPECIAL = np.array([0.5 / 128, 1.5 / 128, -0.5 / 128, 2.5 / 128, 255.99, 256.0, -256.0, -300.0, 600.0, 1e9, -1e9,
                        np.nan, np.inf, -np.inf, 1e-30, -0.0], dtype=np.float32)


def codec_flow_large():
    """flow [1, 2, h, w] float32 past one pass of the encoder's loop: an arithmetic pattern (multiples of
    1/512 in [-320, 320): every rounding case of rint(128 f + 2^15), and both ends outside the uint16
    range), with ENC_SPECIAL in the last 100 pixels of both channels."""
    def make():
        h, w = CODEC_LARGE_H, CODEC_LARGE_W
        assert (h - 1) * w == CODEC_PASS and h * w > CODEC_PASS
        q = np.arange(2 * h * w, dtype=np.int64)
        f = (((q * 2654435761) >> 7) % 327680 - 163840).astype(np.float32) / np.float32(512.0)
        f = f.reshape(1, 2, h * w)
        f[0, 0, -100:-100 + ENC_SPECIAL.size] = ENC_SPECIAL
        f[0, 1, -ENC_SPECIAL.size:] = ENC_SPECIAL[::-1]
        return (np.ascontiguousarray(f.reshape(1, 2, h, w)),)
    return _frozen(("codec_flow_large",), make)[0]


def codec_png(B, h, w, bad_at):
    """uint16 [B, h, w, 3] for the decoder: channels 0 and 1 an arithmetic pattern over the whole uint16
    range, channel 2 in {0, 1}, and at the flat pixel indices bad_at the values 2, 3, 65535, 256, ... in
    turn (above 1: the reference's assertion)."""
    def make():
        n = B * h * w
        q = np.arange(n, dtype=np.int64)
        png = np.empty((n, 3), dtype=np.uint16)
        png[:, 0] = (q * 40503 + 17) % 65536
        png[:, 1] = (q * 30011 + 65535) % 65536
        png[:, 2] = ((q * 2654435761) >> 11) % 3 != 0
        png[list(bad_at), 2] = [(2, 3, 65535, 256, 2, 1000)[t % 6] for t in range(len(bad_at))]
        return (png.reshape(B, h, w, 3),)
    return _frozen(("codec_png", B, h, w, tuple(bad_at)), make)[0]
