"""The motion encoder's integer-exact input set and its exactness certificate (test infrastructure; CPU only, torch
and numpy, every value from tests/prng.py).

On this set every pre-activation, every ReLU mask and every gradient of BasicMotionEncoder (corr_is_convc1=True) is
an integer that fp32 holds exactly under any summation order, so a correct fp32 implementation -- ATen on the CPU,
the HIP kernels with their tiles, slabs and chains -- must return the fp64 reference cast to fp32, bit for bit.  A
tolerance cannot be trusted on this op at large shapes: a ReLU unit whose pre-activation lies within fp32 rounding of
zero takes the other branch and its whole gradient term appears or vanishes (fp32 ATen is 0.1 normwise from fp64 in
grad_c1 at (22, 33, 63) on the normal set).  Here a pre-activation is an exact integer, zero included:
relu'(0) = 0 in the kernels (y <= 0 ? 0 : v) and in ATen alike.

Values
  weights   {-1, 0, 1}, nonzero with probability 1/8 (convf1, whose fan-in is 98: 1/4); biases dense in {-1, 0, 1};
  c1        {0, 1}, half of it zero;  flow  integers in [-2, 2];  grad_out  {-1, 0, 1} on all 128 channels.

Certificate
  For each of the 16 stages -- the four forward convolutions, the four data gradients (grad_flow with the two
  pass-through channels of grad_out added), the four weight gradients and the four bias gradients -- the sum of the
  absolute values of the terms of every output element: the same operation on |input| and |weight| (plus |bias|).
  It bounds every partial sum of that element in any order; with all of them below 2^24 every partial sum is an
  integer fp32 represents, by induction over the stages.  reference() asserts worst < 2^24 for the inputs it builds.
"""
import copy
import functools
import types

import numpy as np
import torch
import torch.nn.functional as F

import prng

C1, OUT, CONV = 256, 128, 126
CONVS = ("convc2", "convf1", "convf2", "conv")   # the order of ecorr_motion_encoder_pack
NAMES = ["grad_flow", "grad_c1"] + [f"{c}.weight" for c in CONVS] + [f"{c}.bias" for c in CONVS]
ONE_IN = {"convc2": 8, "convf1": 4, "convf2": 8, "conv": 8}   # a weight is nonzero with probability 1 / ONE_IN
PAD = {"convc2": 1, "convf1": 3, "convf2": 1, "conv": 1}
LIMIT = 2 ** 24


def _ints(seed, shape):
    """Independent 32-bit draws as int64."""
    n = int(np.prod(shape))
    return (prng.splitmix64(seed, n) >> np.uint64(32)).astype(np.int64).reshape(shape)


def sparse_ternary(seed, shape, one_in):
    v = _ints(seed, shape)
    return np.where(v % one_in == 0, 2 * ((v >> 8) & 1) - 1, 0).astype(np.float32)


def dense_ternary(seed, shape):
    return (_ints(seed, shape) % 3 - 1).astype(np.float32)


def inputs(shape):
    """(flow, c1, grad_out): fp32 CPU tensors of integers."""
    B, H, W = shape
    seed = 4000 + 7 * H + W
    c1 = (_ints(seed, (B, C1, H, W)) & 1).astype(np.float32)
    flow = (_ints(seed + 1, (B, 2, H, W)) % 5 - 2).astype(np.float32)
    go = dense_ternary(seed + 2, (B, OUT, H, W))
    return torch.from_numpy(flow), torch.from_numpy(c1), torch.from_numpy(go)


def exact_module(base):
    """A copy of the BasicMotionEncoder `base` (its device and dtype) with the ternary weights and biases written into
    convc2, convf1, convf2 and conv; convc1 is not part of the op (corr_is_convc1=True)."""
    mod = copy.deepcopy(base)
    with torch.no_grad():
        for k, name in enumerate(CONVS):
            conv = getattr(mod, name)
            w = sparse_ternary(5000 + 2 * k, tuple(conv.weight.shape), ONE_IN[name])
            b = dense_ternary(5001 + 2 * k, tuple(conv.bias.shape))
            conv.weight.copy_(torch.from_numpy(w))
            conv.bias.copy_(torch.from_numpy(b))
    return mod


def autograd(mod, flow, c1, go, dtype, keep=None):
    """The forward output and the 10 gradients (NAMES order) of sum(mod(flow, c1) * go) by autograd on the CPU in
    `dtype` -> numpy float64.  keep: a dict that receives, per convolution, (its input, the gradient at its output)
    as detached tensors of `dtype`, and the fraction of its outputs that are > 0."""
    m = copy.deepcopy(mod).to(dtype).requires_grad_(True)
    ff, cc = flow.clone().to(dtype).requires_grad_(True), c1.clone().to(dtype).requires_grad_(True)
    seen, hooks = {}, []
    if keep is not None:
        for name in CONVS:
            def hook(_, args, out, name=name):
                out.retain_grad()
                seen[name] = (args[0], out)
            hooks.append(getattr(m, name).register_forward_hook(hook))
    out = m(ff, cc, corr_is_convc1=True)
    (out * go.to(dtype)).sum().backward()
    for h in hooks:
        h.remove()
    if keep is not None:
        for name, (x, y) in seen.items():
            keep[name] = (x.detach(), y.grad.detach(), float((y > 0).double().mean()))
    gs = [ff.grad, cc.grad] + [getattr(m, c).weight.grad for c in CONVS] + [getattr(m, c).bias.grad for c in CONVS]
    assert m.convc1.weight.grad is None
    return out.detach().double().numpy(), [g.double().numpy() for g in gs]


def certificate(mod, go, kept):
    """Stage -> the largest sum of absolute values of the terms of one output element, from the fp64 intermediates
    `kept` of autograd(): the 16 stages of the module docstring."""
    cert = {}
    m = copy.deepcopy(mod).double()
    for name in CONVS:
        conv = getattr(m, name)
        x, g = (t.abs() for t in kept[name][:2])
        w, b, pad = conv.weight.detach().abs(), conv.bias.detach().abs(), PAD[name]
        cert[f"{name} forward"] = float(F.conv2d(x, w, b, padding=pad).max())
        dx = F.conv_transpose2d(g, w, padding=pad)
        if name == "convf1":   # grad_flow = the transposed convolution + channels 126-127 of grad_out
            dx = dx + go[:, CONV:].double().abs()
        cert[f"{name} data gradient"] = float(dx.max())
        cert[f"{name} weight gradient"] = float(torch.nn.grad.conv2d_weight(x, tuple(w.shape), g, padding=pad).max())
        cert[f"{name} bias gradient"] = float(g.sum((0, 2, 3)).max())
    return cert


def drop_last_pixel(conv_w, kept):
    """conv.weight's gradient with the last pixel of every item left out of its sum: what a reduction that loses its
    final element would return."""
    x, g = kept["conv"][:2]
    B, _, H, W = x.shape
    wrong = torch.from_numpy(conv_w).clone()
    for ky in range(3):
        for kx in range(3):
            y0, x0 = H - 1 + ky - 1, W - 1 + kx - 1
            if 0 <= y0 < H and 0 <= x0 < W:
                wrong[:, :, ky, kx] -= torch.einsum("bo,bc->oc", g[:, :, H - 1, W - 1], x[:, :, y0, x0])
    return wrong.numpy()


@functools.lru_cache(maxsize=None)
def reference(shape):
    """Once per shape, never changed: flow, c1, go (fp32 CPU tensors); out and grads (NAMES order), the fp64 autograd
    reference as numpy float64; cert and worst, the certificate, asserted < 2^24 here; alive, the fraction of each
    ReLU layer with a positive pre-activation; dropped, conv.weight's gradient without every item's last pixel."""
    from eraft_amd import network
    flow, c1, go = inputs(shape)
    mod = exact_module(network.BasicMotionEncoder())
    kept = {}
    out, grads = autograd(mod, flow, c1, go, torch.float64, keep=kept)
    cert = certificate(mod, go, kept)
    worst = max(cert.values())
    assert worst < LIMIT, f"exact set at {shape}: {max(cert, key=cert.get)} reaches {worst:.4g} >= 2^24"
    for a in [out] + grads:
        assert np.array_equal(a, np.rint(a)) and np.abs(a).max() < LIMIT   # integers fp32 holds
    dropped = drop_last_pixel(grads[NAMES.index("conv.weight")], kept)
    return types.SimpleNamespace(shape=shape, flow=flow, c1=c1, go=go, mod=mod, out=out, grads=grads, cert=cert,
                                 worst=worst, alive={n: kept[n][2] for n in CONVS}, dropped=dropped)
