"""eraft_amd.motion_encoder_train / ecorr_motion_encoder_backward (csrc/motion_enc_grad.hip) against autograd of an
fp64 BasicMotionEncoder on the CPU.

Inputs: tests/test_motion_enc_gpu.py's recipe (make_inputs: c1 = relu(normal) with its exact zeros, flow = 3 * normal;
the PRNG weights), grad_out PRNG normal; loss sum(out * grad_out).  Reference: network.BasicMotionEncoder.double()
autograd on the CPU (corr_is_convc1=True).  fp32 ATen autograd on the CPU runs on the same inputs as the yardstick.
Bars:
  grad_c1, grad_flow                          max |got - ref| / rms(ref) <= 1e-5, the project's bar;
  the four weight and four bias gradients     fp32 ATen itself misses 1e-5 in that metric on the weights (1.5e-5 at
      (2, 40, 50)), so both must hold: the worst of the eight max / rms <= max(1e-5, 4 x ATen's worst of eight), and
      the relative Frobenius error pooled over the eight <= 4 x ATen's -- tests/test_gru_grad_gpu.py's bar and margin
      for two independent fp32 roundings of the same sums; a wrong tap, border or slab is off by orders of magnitude.
Shapes: test_motion_enc_gpu.SHAPES (H or W of 1, sizes shorter than every tap reach, 65 and 129 pixels, three batch
items crossing row ends) and (2, 40, 50): 2000 pixels per item are two weight-gradient slabs of 1024 and 976 pixels,
four in all with ragged last ones.  None of these doubles the slab cap or runs a second chain in menc_wgrad_kernel;
grad_slab_rule.SLAB_SHAPES do, and there the normal set is not used: with 17-23 million ReLU units per case a unit
whose pre-activation lies within fp32 rounding of zero flips its mask (fp32 ATen on the CPU is itself 0.1 normwise from
fp64 in grad_c1 and 0.028 in the weights at (22, 33, 63)), so a tolerance would flake or prove nothing.  They run on
the integer-exact set of tests/menc_exact.py instead, where the forward and all ten gradients must equal the fp64
reference cast to fp32 bit for bit (tests/test_menc_exact_ref.py shows fp32 ATen doing so on the CPU).
"""
import copy
import ctypes
import functools

import numpy as np
import pytest
import torch

import menc_exact
import prng
from gpu_guard import Workspace, check_guarded, guarded, mismatch
from grad_slab_rule import SLAB_GEOMETRY, SLAB_SHAPES, assert_single_chain, assert_slab_shapes, slab_rule, slabs_of
from graph_capture import replay_matches_eager
from test_motion_enc_gpu import SHAPES, cpu_module, gpu_module, make_inputs

pytestmark = pytest.mark.gpu

BAR = 1e-5
C1, OUT, CONV = 256, 128, 126
GRAD_SHAPES = SHAPES + [(2, 40, 50)]
CONVS = ("convc2", "convf1", "convf2", "conv")   # the order of ecorr_motion_encoder_pack
NAMES = ["grad_flow", "grad_c1"] + [f"{c}.weight" for c in CONVS] + [f"{c}.bias" for c in CONVS]


@pytest.fixture(autouse=True)
def _device():
    if not torch.cuda.is_available():
        pytest.fail("no HIP device visible")


def inputs(shape):
    B, H, W = shape
    flow, c1 = make_inputs(300 + 7 * H + W, B, H, W)
    go = torch.from_numpy(prng.normal(700 + 7 * H + W, (B, OUT, H, W)))
    return flow, c1, go


def cpu_grads(flow, c1, go, dtype):
    """The 10 gradients of sum(enc(flow, c1) * go) by autograd on the CPU in `dtype` -> numpy float64, NAMES order."""
    m = copy.deepcopy(cpu_module()).to(dtype).requires_grad_(True)
    ff, cc = flow.clone().to(dtype).requires_grad_(True), c1.clone().to(dtype).requires_grad_(True)
    (m(ff, cc, corr_is_convc1=True) * go.to(dtype)).sum().backward()
    gs = [ff.grad, cc.grad] + [getattr(m, c).weight.grad for c in CONVS] + [getattr(m, c).bias.grad for c in CONVS]
    assert m.convc1.weight.grad is None
    return [g.double().numpy() for g in gs]


@functools.lru_cache(maxsize=None)
def case(shape):
    """(flow, c1, grad_out) on the CPU, the fp64 reference and ATen's fp32 gradients: once per shape, never changed."""
    flow, c1, go = inputs(shape)
    return flow, c1, go, cpu_grads(flow, c1, go, torch.float64), cpu_grads(flow, c1, go, torch.float32)


def train_mod():
    """A trainable copy of the module on the GPU (gpu_module's own is shared with test_motion_enc_gpu)."""
    return copy.deepcopy(gpu_module()).requires_grad_(True)


def ours(flow, c1, go, mod, need_flow=True, need_c1=True):
    """The gradients through motion_encoder_train, NAMES order, numpy float32 (None where nothing was asked for), and
    the forward's output."""
    import eraft_amd
    fd, cd = flow.cuda().requires_grad_(need_flow), c1.cuda().requires_grad_(need_c1)
    mod.zero_grad(set_to_none=True)
    out = eraft_amd.motion_encoder_train(fd, cd, mod)
    (out * go.cuda()).sum().backward()
    torch.cuda.synchronize()
    gs = [fd.grad, cd.grad] + [getattr(mod, c).weight.grad for c in CONVS] + [getattr(mod, c).bias.grad for c in CONVS]
    return [None if g is None else g.cpu().numpy() for g in gs], out.detach()


def normwise(got, ref):
    return float(np.abs(np.asarray(got, np.float64) - ref).max() / np.sqrt(np.mean(ref * ref)))


def pooled(gots, refs):
    num = sum(float(np.sum((np.asarray(g, np.float64) - r) ** 2)) for g, r in zip(gots, refs))
    return (num / sum(float(np.sum(r * r)) for r in refs)) ** 0.5


def same(a, b, what):
    d = mismatch(a.reshape(1, 1, -1), b.reshape(1, 1, -1))
    assert d is None, f"{what}: {d}"


@pytest.mark.parametrize("shape", GRAD_SHAPES, ids=lambda s: "x".join(map(str, s)))
def test_accuracy(shape):
    flow, c1, go, ref, aten = case(shape)
    got, _ = ours(flow, c1, go, train_mod())
    for g, r in zip(got, ref):
        assert g.shape == r.shape and np.isfinite(g).all()
    for n, r in zip(NAMES, ref):
        assert np.any(r != 0), f"{n}: the reference gradient is identically zero"
    errs = [normwise(g, r) for g, r in zip(got, ref)]
    aerr = [normwise(a, r) for a, r in zip(aten, ref)]
    pworst, aworst = max(errs[2:]), max(aerr[2:])
    ppool, apool = pooled(got[2:], ref[2:]), pooled(aten[2:], ref[2:])
    print(f"motion_encoder backward {shape}: max|err|/rms(ref) grad_flow {errs[0]:.3g} (ATen fp32 {aerr[0]:.3g}), "
          f"grad_c1 {errs[1]:.3g} ({aerr[1]:.3g}), weight worst {max(errs[2:6]):.3g} ({max(aerr[2:6]):.3g}), bias "
          f"worst {max(errs[6:]):.3g} ({max(aerr[6:]):.3g}), parameters pooled Frobenius {ppool:.3g} ({apool:.3g})")
    assert errs[0] <= BAR and errs[1] <= BAR
    assert pworst <= max(BAR, 4 * aworst)
    assert ppool <= 4 * apool


def test_forward_unchanged():
    """With grad on, motion_encoder_train returns bitwise what motion_encoder returns under no_grad; a frozen module
    with inputs that do not require grad gives no node."""
    import eraft_amd
    flow, c1, go, _, _ = case((3, 9, 15))
    mod = train_mod()
    _, out = ours(flow, c1, go, mod)
    with torch.no_grad():
        plain = eraft_amd.motion_encoder(flow.cuda(), c1.cuda(), mod)
        again = eraft_amd.motion_encoder_train(flow.cuda(), c1.cuda(), mod)
    assert not again.requires_grad and again.is_contiguous()
    d = mismatch(out.cpu().numpy(), plain.cpu().numpy())
    assert d is None, d
    assert torch.equal(again, plain)
    frozen = copy.deepcopy(mod).requires_grad_(False)
    res = eraft_amd.motion_encoder_train(flow.cuda(), c1.cuda(), frozen)
    assert res.grad_fn is None and torch.equal(res, plain)
    live = eraft_amd.motion_encoder_train(flow.cuda(), c1.cuda(), mod)
    assert live.grad_fn is not None and live.is_contiguous() and live.shape == plain.shape


FOOT = (1, 15, 20)
SPOTS = {"interior": (7, 9), "top-left": (0, 0), "top-right": (0, 19), "bottom-left": (14, 0),
         "bottom-right": (14, 19), "row_end": (7, 19)}


def _block(y0, x0, reach):
    _, H, W = FOOT
    yy, xx = np.mgrid[0:H, 0:W]
    return np.maximum(np.abs(yy - y0), np.abs(xx - x0)) <= reach


@pytest.mark.parametrize("where", list(SPOTS))
def test_footprint(where):
    """grad_out nonzero at one pixel on channels 0-125: grad_c1 is == 0 outside the 5 x 5 block around it (two 3x3
    convolutions), grad_flow outside the 11 x 11 block (two 3x3, then 7x7), each clipped to the image.  A row wrap
    (the flattened neighbour of a row end is the next row's start) or a channel wrap (p - W of row 0 is the previous
    channel's last row) would land outside the clipped block.  One element of grad_out on channel 126 reaches
    grad_flow at its own element with its exact bits, and nothing else."""
    B, H, W = FOOT
    flow, c1, go = inputs(FOOT)
    y0, x0 = SPOTS[where]
    keep = torch.zeros(B, OUT, H, W)
    keep[0, :CONV, y0, x0] = 1
    got, _ = ours(flow, c1, go * keep, train_mod())
    for name, g, reach in (("grad_c1", got[1], 2), ("grad_flow", got[0], 5)):
        blk = _block(y0, x0, reach)
        assert not blk.all()
        assert np.isfinite(g).all()
        assert (g[0][:, ~blk] == 0).all(), f"{name}: outside the block"
        assert (g[0][:, blk] != 0).any(axis=0).all(), f"{name}: a pixel of the block got nothing"
    one = torch.zeros(B, OUT, H, W)
    one[0, CONV, y0, x0] = go[0, CONV, y0, x0]
    got, _ = ours(flow, c1, one, train_mod())
    want = np.zeros((B, 2, H, W), np.float32)
    want[0, 0, y0, x0] = go[0, CONV, y0, x0].item()
    assert want[0, 0, y0, x0] != 0
    assert (got[0] == want).all()
    assert got[0][0, 0, y0, x0].view(np.uint32) == want[0, 0, y0, x0].view(np.uint32)
    for name, g in zip(NAMES[1:], got[1:]):
        assert (g == 0).all(), name


def sizes():
    import eraft_amd
    L = eraft_amd.lib()
    n, m = ctypes.c_int64(), ctypes.c_int64()
    assert L.ecorr_motion_encoder_packed_size(ctypes.byref(n)) == 0
    assert L.ecorr_motion_encoder_backward_packed_size(ctypes.byref(m)) == 0
    return n.value, m.value


def workspace_bytes(B, H, W):
    import eraft_amd
    n = ctypes.c_int64()
    assert eraft_amd.lib().ecorr_motion_encoder_backward_workspace_size(B, H, W, ctypes.byref(n)) == 0
    return n.value


def raw_packs(mod):
    """(packed, packed_t) of mod's weights through the raw pack entries."""
    import eraft_amd
    from eraft_amd import _lib
    L = eraft_amd.lib()
    ws = [getattr(mod, c).weight.detach().contiguous() for c in CONVS]
    bs = [getattr(mod, c).bias.detach().contiguous() for c in CONVS]
    st = _lib.stream_of(ws[0])
    n, m = sizes()
    packed = torch.empty(n, dtype=torch.uint8, device="cuda")
    packed_t = torch.empty(m, dtype=torch.uint8, device="cuda")
    wp = (ctypes.c_void_p * 4)(*[t.data_ptr() for t in ws])
    bp = (ctypes.c_void_p * 4)(*[t.data_ptr() for t in bs])
    assert L.ecorr_motion_encoder_pack(wp, bp, packed.data_ptr(), st) == 0
    assert L.ecorr_motion_encoder_backward_pack(wp, packed_t.data_ptr(), st) == 0
    torch.cuda.synchronize()
    return packed, packed_t


def raw_backward(fd, cd, go_ptr, stride, packs, outs, ws_ptr):
    """ecorr_motion_encoder_backward on device tensors into the 10 device float tensors `outs` (NAMES order)."""
    import eraft_amd
    from eraft_amd import _lib
    B, _, H, W = cd.shape
    gw = (ctypes.c_void_p * 4)(*[t.data_ptr() for t in outs[2:6]])
    gb = (ctypes.c_void_p * 4)(*[t.data_ptr() for t in outs[6:]])
    assert eraft_amd.lib().ecorr_motion_encoder_backward(
        cd.data_ptr(), fd.data_ptr(), go_ptr, stride, B, H, W, packs[0].data_ptr(), packs[1].data_ptr(),
        outs[1].data_ptr(), outs[0].data_ptr(), gw, gb, ws_ptr, _lib.stream_of(cd)) == 0


def out_sizes(B, H, W):
    return [B * 2 * H * W, B * C1 * H * W, 192 * 256 * 9, 128 * 2 * 49, 64 * 128 * 9, 126 * 256 * 9, 192, 128, 64, 126]


@pytest.mark.parametrize("shape", [(3, 9, 15), (1, 1, 1), (2, 40, 50)], ids=lambda s: "x".join(map(str, s)))
def test_guards_and_raw_abi(shape):
    """All 10 outputs between guard bands and a workspace of exactly the reported size between guards, prefilled with
    0xff bytes (a read before a write is a NaN) and then with 0x00: the guards stay, every output element is written,
    the bits are those of the Python path either way.  Then grad_out as the upper half of a [B, 256, H, W] buffer
    through grad_out_batch_stride: the contiguous call's bits."""
    B, H, W = shape
    flow, c1, go, _, _ = case(shape)
    mod = train_mod()
    want, _ = ours(flow, c1, go, mod)
    fd, cd, god = flow.cuda(), c1.cuda(), go.cuda()
    packs = raw_packs(mod)
    gx = torch.full((B, 256, H, W), float("nan"), device="cuda")   # the lower half is never to be read
    gx[:, 128:] = god
    for fill, ptr, stride in ((0xff, god.data_ptr(), OUT * H * W), (0x00, god.data_ptr(), OUT * H * W),
                              (0xff, gx[:, 128:].data_ptr(), 256 * H * W)):
        bufs = [guarded(n) for n in out_sizes(B, H, W)]
        ws = Workspace(workspace_bytes(B, H, W), fill)
        raw_backward(fd, cd, ptr, stride, packs, [b[1] for b in bufs], ws.ptr)
        torch.cuda.synchronize()
        ws.check("motion_encoder backward workspace")
        for name, (buf, _), w in zip(NAMES, bufs, want):
            got = check_guarded(buf, f"motion_encoder backward {name}")
            assert np.isfinite(got).all(), name
            same(got, w, f"{name}: raw ABI (workspace of {fill:#x}, stride {stride}) against motion_encoder_train")


EXACT_SHAPES = SLAB_SHAPES + [(3, 9, 15), (2, 40, 50)]


def test_slab_geometry():
    """SLAB_SHAPES have the doubled cap and the second chain the table states, the library sizes its partials by
    that slab count, and no shape of GRAD_SHAPES reaches either branch."""
    assert_slab_shapes()
    assert_single_chain(GRAD_SHAPES)
    for B, H, W in SLAB_SHAPES:
        cap, nsl, slab, chains = slab_rule(B, H * W)
        assert (cap, nsl, slab, slabs_of(H * W, nsl, slab)) == SLAB_GEOMETRY[(B, H, W)] and chains == 2
        bias = (B * -(-H * W // 64) * 512 * 4 + 255) // 256 * 256
        assert workspace_bytes(B, H, W) == 896 * B * H * W * 4 + bias + B * nsl * 9 * 192 * 256 * 4


def exact_mod():
    """A trainable copy of the GPU module holding the exact set's ternary weights."""
    return menc_exact.exact_module(gpu_module()).requires_grad_(True)


def exact_want(ref):
    """The fp64 reference's ten gradients and forward output cast to fp32: every value is an integer below 2^24."""
    return [g.astype(np.float32) for g in ref.grads], ref.out.astype(np.float32)


@pytest.mark.parametrize("shape", EXACT_SHAPES, ids=lambda s: "x".join(map(str, s)))
def test_exact_set_bit_for_bit(shape):
    """On the integer-exact set motion_encoder_train's forward and ten gradients, and motion_encoder's forward, are
    the fp64 reference's bits: any tile, slab, chain or tap error changes an integer."""
    import eraft_amd
    ref = menc_exact.reference(shape)
    assert ref.worst < menc_exact.LIMIT
    want, fwd = exact_want(ref)
    mod = exact_mod()
    got, out = ours(ref.flow, ref.c1, ref.go, mod)
    d = mismatch(out.cpu().numpy(), fwd)
    assert d is None, f"motion_encoder_train forward: {d}"
    for name, g, w in zip(NAMES, got, want):
        assert g.shape == w.shape, name
        assert np.any(w != 0), f"{name}: the reference gradient is identically zero"
        same(g, w, f"{name} against the fp64 reference")
    with torch.no_grad():
        plain = eraft_amd.motion_encoder(ref.flow.cuda(), ref.c1.cuda(), mod)
    d = mismatch(plain.cpu().numpy(), fwd)
    assert d is None, f"motion_encoder forward: {d}"


def test_exact_set_raw_abi_doubled_cap():
    """(33, 25, 41) through the raw entry: all 10 outputs between guard bands and a workspace of exactly the reported
    size between guards, prefilled with 0xff bytes.  The guards stay, every element is written, and the bits are the
    fp64 reference's (so the Python path's)."""
    shape = SLAB_SHAPES[0]
    B, H, W = shape
    assert slab_rule(B, H * W)[3] == 2
    ref = menc_exact.reference(shape)
    want, _ = exact_want(ref)
    fd, cd, god = ref.flow.cuda(), ref.c1.cuda(), ref.go.cuda()
    packs = raw_packs(exact_mod())
    bufs = [guarded(n) for n in out_sizes(B, H, W)]
    ws = Workspace(workspace_bytes(B, H, W), 0xff)
    raw_backward(fd, cd, god.data_ptr(), OUT * H * W, packs, [b[1] for b in bufs], ws.ptr)
    torch.cuda.synchronize()
    ws.check("motion_encoder backward workspace")
    for name, (buf, _), w in zip(NAMES, bufs, want):
        got = check_guarded(buf, f"motion_encoder backward {name}")
        same(got, w, f"{name}: raw ABI on the exact set against the fp64 reference")


def test_strided_grad_out_from_cat():
    """x = cat([inp, m], 1) hands m's node the upper half of x's gradient as a view of batch stride 256 H W: at B > 1
    _MencFn.backward reads it in place.  The hook records that stride -- a contiguous tensor here would mean the
    in-place branch never runs under this torch -- and all ten gradients are the contiguous call's bits."""
    import eraft_amd
    shape = (3, 9, 15)
    B, H, W = shape
    flow, c1, _, _, _ = case(shape)
    gx = torch.from_numpy(prng.normal(811, (B, 2 * OUT, H, W)))
    inp = torch.from_numpy(prng.normal(812, (B, OUT, H, W))).cuda().requires_grad_(True)
    mod = train_mod()
    fd, cd = flow.cuda().requires_grad_(True), c1.cuda().requires_grad_(True)
    m = eraft_amd.motion_encoder_train(fd, cd, mod)
    seen = []
    m.register_hook(lambda g: seen.append((tuple(g.shape), tuple(g.stride()), g.dtype)))
    x = torch.cat([inp, m], 1)
    (x * gx.cuda()).sum().backward()
    torch.cuda.synchronize()
    assert seen == [((B, OUT, H, W), (2 * OUT * H * W, H * W, W, 1), torch.float32)], \
        f"autograd delivered {seen}: not the upper half of grad_x in place, the no-copy branch did not run"
    got = [fd.grad, cd.grad] + [getattr(mod, c).weight.grad for c in CONVS] + [getattr(mod, c).bias.grad for c in CONVS]
    same(inp.grad.cpu().numpy(), gx[:, :OUT].numpy(), "inp.grad")
    want, _ = ours(flow, c1, gx[:, OUT:].contiguous(), train_mod())
    for name, g, w in zip(NAMES, got, want):
        same(g.cpu().numpy(), w, f"{name}: strided grad_out against the contiguous call")


def test_two_calls_same_bits_and_batch_independence():
    flow, c1, go, _, _ = case((2, 40, 50))
    a, _ = ours(flow, c1, go, train_mod())
    b, _ = ours(flow, c1, go, train_mod())
    for name, p, q in zip(NAMES, a, b):
        same(p, q, name)
    flow, c1, go, _, _ = case((3, 9, 15))
    whole, _ = ours(flow, c1, go, train_mod())
    for i in range(3):
        part, _ = ours(flow[i:i + 1].contiguous(), c1[i:i + 1].contiguous(), go[i:i + 1].contiguous(), train_mod())
        for k in (0, 1):
            d = mismatch(part[k], whole[k][i:i + 1])
            assert d is None, f"item {i}, {NAMES[k]}: {d}"


def test_selective_outputs():
    flow, c1, go, _, _ = case((3, 9, 15))
    full, _ = ours(flow, c1, go, train_mod())
    frozen = copy.deepcopy(gpu_module()).requires_grad_(False)
    got, _ = ours(flow, c1, go, frozen)
    assert all(g is None for g in got[2:])
    for k in (0, 1):
        same(got[k], full[k], f"frozen encoder, {NAMES[k]}")
    got, _ = ours(flow, c1, go, train_mod(), need_flow=False, need_c1=False)
    assert got[0] is None and got[1] is None
    for name, p, q in zip(NAMES[2:], got[2:], full[2:]):
        same(p, q, f"detached flow and c1, {name}")
    for nf, nc in ((True, False), (False, True)):   # one of the two data gradients
        got, _ = ours(flow, c1, go, frozen, need_flow=nf, need_c1=nc)
        k = 0 if nf else 1
        assert got[1 - k] is None and all(g is None for g in got[2:])
        same(got[k], full[k], f"{NAMES[k]} alone")


def test_weight_cache_follows_updates():
    """After an in-place optimizer-style update the next forward + backward uses the new weights: both packs are
    repacked, the result is a fresh module's bit for bit."""
    from eraft_amd import motion_enc as M
    flow, c1, go, _, _ = case((1, 15, 20))
    mod = train_mod()
    before, _ = ours(flow, c1, go, mod)
    packs = (M._packs[mod][2], M._packs_t[mod][2])
    with torch.no_grad():
        for n, p in mod.named_parameters():
            if not n.startswith("convc1"):
                p.add_(p, alpha=0.25)
    after, _ = ours(flow, c1, go, mod)
    assert M._packs[mod][2] is not packs[0] and M._packs_t[mod][2] is not packs[1]
    want, _ = ours(flow, c1, go, copy.deepcopy(mod))
    for name, p, q, r in zip(NAMES, after, want, before):
        same(p, q, f"after the update, {name}")
        assert (p != r).any(), name


def test_autograd_contract():
    import eraft_amd
    flow, c1, go, _, _ = case((2, 3, 5))
    mod = train_mod()
    fd, cd = flow.cuda().requires_grad_(True), c1.cuda()
    out = eraft_amd.motion_encoder_train(fd, cd, mod)
    cd.add_(1.0)   # an in-place change of the saved c1 raises
    with pytest.raises(RuntimeError, match="modified by an inplace operation"):
        out.sum().backward()
    cd = c1.cuda()
    loss = (eraft_amd.motion_encoder_train(fd, cd, mod) * go.cuda()).sum()
    loss.backward()
    with pytest.raises(RuntimeError, match="second time"):
        loss.backward()
    with pytest.raises(TypeError):
        eraft_amd.motion_encoder_train(fd.half(), cd, mod)
    with pytest.raises(RuntimeError, match="HIP devices"):
        eraft_amd.motion_encoder_train(flow, cd, mod)
    with pytest.raises(RuntimeError):
        eraft_amd.motion_encoder_train(fd, cd[:, :128].contiguous(), mod)
    with pytest.raises(RuntimeError, match="forward-only"):   # the forward-only entry keeps its refusal
        eraft_amd.motion_encoder(fd, cd, mod)
    # a grad_out that is not (S, H W, W, 1): an expanded scalar
    fd.grad = None
    eraft_amd.motion_encoder_train(fd, cd, mod).sum().backward()
    assert torch.isfinite(fd.grad).all()


def _grads(fd, cd, god, mod):
    import eraft_amd
    ps = [getattr(mod, c).weight for c in CONVS] + [getattr(mod, c).bias for c in CONVS]
    out = eraft_amd.motion_encoder_train(fd, cd, mod)
    return [out.detach()] + list(torch.autograd.grad(out, [fd, cd] + ps, god))


def test_graph_capture():
    """Forward + backward through motion_encoder_train captured and replayed on changed inputs equals eager."""
    B, H, W = 3, 9, 15
    sets = [make_inputs(200 + 10 * i, B, H, W) + (torch.from_numpy(prng.normal(900 + i, (B, OUT, H, W))),)
            for i in range(2)]
    sets = [tuple(t.cuda() for t in s) for s in sets]
    fd, cd, god = (t.clone() for t in sets[0])
    fd.requires_grad_(True)
    cd.requires_grad_(True)
    mod = train_mod()
    _grads(fd, cd, god, mod)   # both packs, outside the capture
    outs = []

    def step():
        outs[:] = _grads(fd, cd, god, mod)

    def mutate(i):
        with torch.no_grad():
            for dst, src in zip((fd, cd, god), sets[i]):
                dst.copy_(src)

    replay_matches_eager(step, mutate, outs)


@pytest.mark.filterwarnings("ignore:The CUDA Graph is empty")   # the refused capture recorded nothing
def test_pack_under_capture_is_refused():
    flow, c1, go, _, _ = case((2, 3, 5))
    mod = train_mod()   # not packed yet
    fd, cd, god = flow.cuda().requires_grad_(True), c1.cuda(), go.cuda()
    torch.cuda.synchronize()
    g = torch.cuda.CUDAGraph()
    with pytest.raises(RuntimeError, match="outside the captured region"):
        with torch.cuda.graph(g):
            _grads(fd, cd, god, mod)
    want, _ = ours(flow, c1, go, train_mod())
    got, _ = ours(flow, c1, go, mod)   # the refusal left nothing behind: an eager call packs and runs
    for name, p, q in zip(NAMES, got, want):
        same(p, q, name)


def test_nan_in_c1_follows_torch():
    """One NaN in c1: isnan of grad_c1 and grad_flow equals isnan of fp32 CPU autograd's exactly.  relu' is
    y <= 0 ? 0 : g on the ReLU's output, so a NaN activation passes its gradient and no data gradient reads c1's
    values: autograd's two data gradients stay NaN-free (a mask applied as a product would put 0 * NaN there), while
    its convc2 and conv weight gradients are NaN."""
    B, H, W = 2, 13, 14
    flow, c1 = make_inputs(53, B, H, W)
    go = torch.from_numpy(prng.normal(54, (B, OUT, H, W)))
    c1 = c1.clone()
    c1[0, 17, 6, 7] = float("nan")
    ref = cpu_grads(flow, c1, go, torch.float32)
    got, _ = ours(flow, c1, go, train_mod())
    assert np.isnan(ref[2]).any() and np.isnan(ref[5]).any()   # the NaN did reach the reference's backward
    for k in (0, 1):
        diff = int((np.isnan(got[k]) != np.isnan(ref[k])).sum())
        assert diff == 0, f"{NAMES[k]}: {diff} elements differ in NaN-ness"
