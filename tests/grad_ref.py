"""Plain references of the CorrBlock backward (test infrastructure: numpy / torch-CPU, no GPU).

lookup_backward_ref  the gradient pyramid of one lookup.  The coordinate chain is the forward's, step
    by step in float32 (the fp32 rounding of the coordinates decides which pixels a tap touches and is
    part of the operation: a pure-fp64 chain is a different function); the weight products and the
    accumulation are float64.
build_backward_ref   the two fmap gradients from a gradient pyramid, all in float64.
aten_*               the same two steps as fp32 ATen autograd of the reference's op sequence
    (oracle/torch_ref.py) on independent leaf levels: the yardstick `e_aten` of the GPU tests' bar and
    what tests/test_grad_ref.py validates the plain references against.
"""
import numpy as np
import torch
import torch.nn.functional as F

from torch_ref import TorchCpuCorrBlock


def level_sizes(H, W, levels):
    """(hs, ws) of the floor-pooled pyramid."""
    return [H >> i for i in range(levels)], [W >> i for i in range(levels)]


def _tap_chain(c, i, r, n):
    """Floor (float32), in-range masks and float64 weights of the K taps of one axis at level i.
    c: float32 [B, Q] -> each [K, B, Q] for the two corners (floor, floor + 1)."""
    f32 = np.float32
    with np.errstate(all="ignore"):
        cs = c * f32(2.0 ** -i)                                              # 1. c * 2^-i
        t = cs[None] + np.arange(-r, r + 1, dtype=np.float32)[:, None, None]  # 2. + (o - r)
        g = (f32(2.0) * t) / f32(n - 1) - f32(1.0)                           # 3. g = 2c / (n - 1) - 1
        v = (g + f32(1.0)) * f32((n - 1) / 2)                                # 4. v = (g + 1) (n - 1) / 2
        f0 = np.floor(v)                                                     # 5. floor and fraction
        frac = v - f0
        f1 = f0 + f32(1.0)
        w0 = f32(1.0) - frac
        assert t.dtype == g.dtype == v.dtype == frac.dtype == w0.dtype == np.float32
        in0 = (f0 >= f32(0.0)) & (f0 < f32(n))                               # axis_in: the float test
        in1 = (f1 >= f32(0.0)) & (f1 < f32(n))
        i0 = np.where(in0, f0, f32(0.0)).astype(np.int64)
        i1 = np.where(in1, f1, f32(0.0)).astype(np.int64)
    return (i0, in0, w0.astype(np.float64)), (i1, in1, frac.astype(np.float64))


def lookup_backward_ref(grad_out, coords, hs, ws, radius):
    """grad_out [B][L K^2][Q] (channel K^2 i + K a + b = x-offset a, y-offset b), coords [B][2][Q]
    -> per level [B Q, h_i, w_i] float64: what the lookup's backward adds to the gradient pyramid."""
    go = np.asarray(grad_out, dtype=np.float32)
    c = np.asarray(coords, dtype=np.float32)
    B, C, Q = go.shape
    K = 2 * radius + 1
    L = len(hs)
    assert C == L * K * K and c.shape == (B, 2, Q)
    rows = (np.arange(B)[:, None] * Q + np.arange(Q)[None, :])[None, None]    # [1, 1, B, Q]
    out = []
    for i, (h, w) in enumerate(zip(hs, ws)):
        g = go[:, i * K * K:(i + 1) * K * K].reshape(B, K, K, Q).transpose(1, 2, 0, 3).astype(np.float64)  # [a][b][B][Q]
        xc = _tap_chain(c[:, 0], i, radius, w)
        yc = _tap_chain(c[:, 1], i, radius, h)
        acc = np.zeros(B * Q * h * w, dtype=np.float64)
        for (xi, xin, xw) in xc:
            for (yi, yin, yw) in yc:
                m = xin[:, None] & yin[None, :]                               # [a][b][B][Q]
                val = (yw[None, :] * xw[:, None]) * g
                idx = (rows * h + yi[None, :]) * w + xi[:, None]
                acc += np.bincount(idx[m], weights=val[m], minlength=acc.size)
        out.append(acc.reshape(B * Q, h, w))
    return out


def up2(x, h, w):
    """Adjoint of the floor-mode 2 x 2 sum pool onto an h x w image: every fine pixel takes its coarse
    parent's value, a dropped odd last row / column gets nothing."""
    n, ch, cw = x.shape
    assert ch == h // 2 and cw == w // 2
    out = np.zeros((n, h, w), dtype=np.float64)
    out[:, :2 * ch, :2 * cw] = np.repeat(np.repeat(x, 2, axis=1), 2, axis=2)
    return out


def fold_ref(G_levels):
    """T_0 = G_0 + 1/4 up(G_1 + 1/4 up(G_2 + ...)) in float64."""
    t = np.asarray(G_levels[-1], dtype=np.float64)
    for lv in reversed(G_levels[:-1]):
        lv = np.asarray(lv, dtype=np.float64)
        t = lv + 0.25 * up2(t, lv.shape[1], lv.shape[2])
    return t


def build_backward_ref(G_levels, fmap1_slab, fmap2):
    """G_levels: [B q, h_i, w_i] each; fmap1_slab [B][D][q]; fmap2 [B][D][H][W]
    -> (grad_fmap1 [B][D][q], grad_fmap2 [B][D][H][W]) float64."""
    f1 = np.asarray(fmap1_slab, dtype=np.float64)
    f2 = np.asarray(fmap2, dtype=np.float64)
    B, D, H, W = f2.shape
    q = f1.shape[2]
    T = fold_ref(G_levels).reshape(B, q, H * W)
    s = np.sqrt(np.float64(D))
    g1 = np.einsum("bdn,bpn->bdp", f2.reshape(B, D, H * W), T) / s
    g2 = np.einsum("bdp,bpn->bdn", f1, T) / s
    return g1, g2.reshape(B, D, H, W)


# ---- special coordinates ----

def specials(H, W):
    """NaN, +-inf, huge and overflowing values (3e38 * 2 = inf; 1.1e7 and 3e7 are past the kernels' 1e7
    window guard, 9.9e6 just inside it; 2^23 and 2^24 + 1 sit where float32 loses the fraction / the
    unit), signed zero, the values around both image borders and a denormal-scale positive."""
    return np.array([np.nan, np.inf, -np.inf, 1e6, -1e6, 3e38, 1e9, -7e5, 3e7, 9.9e6, 1.1e7, 8388608.0,
                     16777217.0, -0.0, -0.5, -1.0, W - 1, W, H - 1, H, 1e-30], dtype=np.float32)


# the specials whose level-0 window the end taps do not bound (NaN, or a floor of 1e7 and more): the
# lookup backward's serial path
SERIAL = np.array([np.nan, np.inf, -np.inf, 3e38, 1e9, 3e7, 1.1e7, 16777217.0], dtype=np.float32)


def special_coords(seed, B, H, W, block=64):
    """[B, 2, H, W] coordinates: sigma = 3 flow, with (per batch item, shifted by one block per item)
      block 0: every query special in both channels, x from SERIAL (a whole workgroup of the lookup
               backward on its serial path);
      block 1: every other query special, the rest normal;
      block 2: one axis special and the other normal (x special on even queries, y on odd ones);
    and, as tests/golden/make_golden.py special_coords, specials scattered singly through the rest."""
    import prng
    c = prng.coords_with_flow(seed, B, H, W, 3.0).reshape(B, 2, H * W)
    sp = specials(H, W)
    n = sp.size
    Q = H * W
    assert Q >= 4 * block
    for b in range(B):
        q0 = (b * block) % (Q - 3 * block + 1)
        k = np.arange(block)
        c[b, 0, q0 + k] = SERIAL[k % SERIAL.size]           # at level 0 the whole block leaves the window path
        c[b, 1, q0 + k] = sp[(5 * k + 3 + b) % n]
        k2 = q0 + block + np.arange(0, block, 2)
        c[b, 0, k2] = sp[(np.arange(k2.size) + 7) % n]
        c[b, 1, k2] = sp[(np.arange(k2.size) * 2 + b) % n]
        k3 = q0 + 2 * block + np.arange(block)
        ev, od = k3[0::2], k3[1::2]
        c[b, 0, ev] = sp[np.arange(ev.size) % n]
        c[b, 1, od] = sp[np.arange(od.size) % n]
        rest = np.arange(q0 + 3 * block, Q)
        if rest.size:
            idx = rest[(np.arange(n) * 37 + 5) % rest.size]
            c[b, (np.arange(n) + b) % 2, idx] = sp
    return np.ascontiguousarray(c.reshape(B, 2, H, W))


def edge_coords(B, H, W):
    """The integer grid with windows hanging over all four image edges (the `edge` set of
    tests/test_corr_gpu.py test_lookup_adversarial_coords)."""
    ys, xs = np.meshgrid(np.arange(H, dtype=np.float32), np.arange(W, dtype=np.float32), indexing="ij")
    edge = np.broadcast_to(np.stack([xs, ys])[None], (B, 2, H, W)).astype(np.float32).copy()
    edge[:, 0, :, :4] = np.float32(-4.5) - edge[:, 0, :, :4]              # left of the image
    edge[:, 0, :, -4:] += np.float32(3.7)                                  # right of it
    edge[:, 1, :2] = np.float32(-0.999)                                    # just above
    edge[:, 1, -2:] = np.float32(H - 1) + np.float32(2.25)                 # below
    return edge


def special_rows(coords):
    """Queries [B, Q] (bool) with a non-finite or huge (|c| >= 7e5) coordinate in either channel: every
    tap of theirs is outside every level."""
    B = coords.shape[0]
    c = coords.reshape(B, 2, -1)
    with np.errstate(invalid="ignore"):
        return (~(np.abs(c) < 7e5)).any(axis=1)


# ---- ATen fp32 autograd of the reference's op sequence ----

def aten_lookup_backward(grad_out, coords, hs, ws, radius, dtype=torch.float32):
    """Per-level gradients [B Q, h_i, w_i] of sum(lookup * grad_out) with respect to independent leaf
    levels: F.grid_sample(align_corners=True) backward, the op sequence of oracle/torch_ref.py."""
    go = torch.from_numpy(np.ascontiguousarray(grad_out)).to(dtype)
    c = torch.from_numpy(np.ascontiguousarray(coords)).to(dtype)
    B, C, Q = go.shape
    blk = TorchCpuCorrBlock.__new__(TorchCpuCorrBlock)
    blk.num_levels, blk.radius = len(hs), radius
    blk.corr_pyramid = [torch.zeros(B * Q, 1, h, w, dtype=dtype, requires_grad=True) for h, w in zip(hs, ws)]
    out = TorchCpuCorrBlock.__call__(blk, c.view(B, 2, 1, Q))
    if dtype != torch.float32:   # __call__ ends in .float(); differentiable, exact for the zero leaves
        out = out.to(dtype)
    (out * go.view(B, C, 1, Q)).sum().backward()
    return [lv.grad[:, 0].numpy() for lv in blk.corr_pyramid]


def aten_build_backward(G_levels, fmap1_slab, fmap2, dtype=torch.float32):
    """(grad_fmap1, grad_fmap2) by autograd of bmm / sqrt(D) followed by the avg_pool2d chain, with the
    G_levels as the levels' upstream gradients."""
    f1 = torch.from_numpy(np.ascontiguousarray(fmap1_slab)).to(dtype).requires_grad_(True)
    f2 = torch.from_numpy(np.ascontiguousarray(fmap2)).to(dtype).requires_grad_(True)
    B, D, H, W = f2.shape
    q = f1.shape[2]
    vol = torch.bmm(f1.transpose(1, 2), f2.reshape(B, D, H * W))
    vol = vol / torch.sqrt(torch.tensor(D, dtype=dtype))
    lvl = vol.reshape(B * q, 1, H, W)
    loss = 0.0
    for i, g in enumerate(G_levels):
        if i > 0:
            lvl = F.avg_pool2d(lvl, 2, stride=2)
        loss = loss + (lvl[:, 0] * torch.from_numpy(np.ascontiguousarray(g)).to(dtype)).sum()
    loss.backward()
    return f1.grad.numpy(), f2.grad.numpy()
