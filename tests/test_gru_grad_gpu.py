"""eraft_amd.sepconv_gru_train / ecorr_sepconv_gru_backward (csrc/gru_grad.hip) against autograd of an fp64
SepConvGRU on the CPU.

Inputs: tests/test_gru_gpu.py's recipe (make_inputs, the PRNG weights * 1 and * 8), grad_out PRNG normal; loss
sum(h' * grad_out).  Reference: network.SepConvGRU.double() autograd on the CPU.  Bars:
  grad_h, grad_x, the six bias gradients   max |got - ref| / rms(ref) <= 1e-5, the project's bar;
  the six weight gradients                 fp32 ATen autograd on the CPU itself misses 1e-5 in that metric (the
      error scales with the element, and the flow channels' elements are 3x the rest), so it is run on the same
      inputs and both must hold: the worst of the six max / rms <= max(1e-5, 4 x ATen's worst of six), and the
      relative Frobenius error pooled over the six <= 4 x ATen's -- the margin tests/test_grad_gpu.py gives two
      independent fp32 roundings of the same sums; a wrong tap, border or slab is off by orders of magnitude.
Shapes: test_gru_gpu.SHAPES (ragged tiles across row ends with a batch offset, W = the tap count, H = 1, W = 1,
both axes shorter than the taps) and (2, 40, 50): 2000 pixels per item are two weight-gradient slabs of 1024
and 976 pixels each (the slab cap is 1024), four slabs in all with ragged last ones.  None of these doubles the slab
cap or runs a second chain in gru_wgrad_kernel; grad_slab_rule.SLAB_SHAPES do: (33, 25, 41), one slab of 33 chunks
whose second chain is one chunk holding one valid pixel, and (22, 33, 63), slabs of 1056 (a second chain of one full
chunk) and 1023 pixels, 44 in the launch.  There the six bias gradients take the weights' form of bar: over ~34 000
pixels fp32 ATen itself is at 5e-6 .. 7.4e-6 of the fixed 1e-5 (measured on these inputs on the CPU), so the worst of
six <= max(1e-5, 4 x ATen's worst of six); the existing shapes keep the fixed bar.  A dropped or misplaced chunk
changes a weight gradient by about sqrt(32 / 1025) of its norm, four orders of magnitude above the bars.
"""
import copy
import ctypes
import functools

import numpy as np
import pytest
import torch

import prng
from gpu_guard import Workspace, check_guarded, guarded, mismatch
from grad_slab_rule import SLAB_GEOMETRY, SLAB_SHAPES, assert_single_chain, assert_slab_shapes, slab_rule, slabs_of
from graph_capture import replay_matches_eager
from test_gru_gpu import HID, INP, SCALES, SHAPES, cpu_module, gpu_module, make_inputs

pytestmark = pytest.mark.gpu

BAR = 1e-5
GRAD_SHAPES = SHAPES + [(2, 40, 50)]
CONVS = ("convz1", "convr1", "convq1", "convz2", "convr2", "convq2")
NAMES = ["grad_h", "grad_x"] + [f"{c}.weight" for c in CONVS] + [f"{c}.bias" for c in CONVS]


@pytest.fixture(autouse=True)
def _device():
    if not torch.cuda.is_available():
        pytest.fail("no HIP device visible")


def inputs(shape):
    B, H, W = shape
    h, x = make_inputs(100 + 7 * H + W, B, H, W)
    go = torch.from_numpy(prng.normal(500 + 7 * H + W, (B, HID, H, W)))
    return h, x, go


def cpu_grads(mod, h, x, go, dtype):
    """The 14 gradients of sum(mod(h, x) * go) by autograd on the CPU in `dtype` -> numpy float64, in NAMES order."""
    m = copy.deepcopy(mod).to(dtype).requires_grad_(True)
    hh, xx = h.clone().to(dtype).requires_grad_(True), x.clone().to(dtype).requires_grad_(True)   # never h itself
    (m(hh, xx) * go.to(dtype)).sum().backward()
    gs = [hh.grad, xx.grad] + [getattr(m, c).weight.grad for c in CONVS] + [getattr(m, c).bias.grad for c in CONVS]
    return [g.double().numpy() for g in gs]


@functools.lru_cache(maxsize=None)
def case(shape, scale):
    """(h, x, grad_out) on the CPU, the fp64 reference and ATen's fp32 gradients: once per case, never changed."""
    h, x, go = inputs(shape)
    mod = cpu_module(scale)
    return h, x, go, cpu_grads(mod, h, x, go, torch.float64), cpu_grads(mod, h, x, go, torch.float32)


def train_mod(scale):
    """A trainable copy of the module on the GPU (gpu_module's own is shared with test_gru_gpu)."""
    return copy.deepcopy(gpu_module(scale)).requires_grad_(True)


def ours(h, x, go, mod, need_h=True, need_x=True):
    """The gradients through sepconv_gru_train, NAMES order, numpy float32 (None where nothing was asked for),
    and the forward's output."""
    import eraft_amd
    hd, xd = h.cuda().requires_grad_(need_h), x.cuda().requires_grad_(need_x)
    mod.zero_grad(set_to_none=True)
    out = eraft_amd.sepconv_gru_train(hd, xd, mod)
    (out * go.cuda()).sum().backward()
    torch.cuda.synchronize()
    gs = [hd.grad, xd.grad] + [getattr(mod, c).weight.grad for c in CONVS] + [getattr(mod, c).bias.grad for c in CONVS]
    return [None if g is None else g.cpu().numpy() for g in gs], out.detach()


def normwise(got, ref):
    return float(np.abs(np.asarray(got, np.float64) - ref).max() / np.sqrt(np.mean(ref * ref)))


def pooled(gots, refs):
    num = sum(float(np.sum((np.asarray(g, np.float64) - r) ** 2)) for g, r in zip(gots, refs))
    return (num / sum(float(np.sum(r * r)) for r in refs)) ** 0.5


@pytest.mark.parametrize("scale", SCALES, ids=lambda s: f"w{s}")
@pytest.mark.parametrize("shape", GRAD_SHAPES, ids=lambda s: "x".join(map(str, s)))
def test_accuracy(shape, scale):
    h, x, go, ref, aten = case(shape, scale)
    got, _ = ours(h, x, go, train_mod(scale))
    for g, r in zip(got, ref):
        assert g.shape == r.shape and np.isfinite(g).all()
    errs = [normwise(g, r) for g, r in zip(got, ref)]
    aerr = [normwise(a, r) for a, r in zip(aten, ref)]
    wworst, aworst = max(errs[2:8]), max(aerr[2:8])
    wpool, apool = pooled(got[2:8], ref[2:8]), pooled(aten[2:8], ref[2:8])
    print(f"sepconv_gru backward {shape} weights*{scale}: max|err|/rms(ref) grad_h {errs[0]:.3g} (ATen fp32 "
          f"{aerr[0]:.3g}), grad_x {errs[1]:.3g} ({aerr[1]:.3g}), bias worst {max(errs[8:]):.3g} "
          f"({max(aerr[8:]):.3g}), weight worst {wworst:.3g} ({aworst:.3g}), weight pooled Frobenius "
          f"{wpool:.3g} ({apool:.3g})")
    assert errs[0] <= BAR and errs[1] <= BAR
    for n, e in zip(NAMES[8:], errs[8:]):
        assert e <= BAR, n
    assert wworst <= max(BAR, 4 * aworst)
    assert wpool <= 4 * apool


def test_slab_geometry():
    """SLAB_SHAPES have the doubled cap and the second chain the table states, the library sizes its partials by
    that slab count, and no shape of GRAD_SHAPES reaches either branch."""
    assert_slab_shapes()
    assert_single_chain(GRAD_SHAPES)
    for B, H, W in SLAB_SHAPES:
        cap, nsl, slab, chains = slab_rule(B, H * W)
        assert (cap, nsl, slab, slabs_of(H * W, nsl, slab)) == SLAB_GEOMETRY[(B, H, W)] and chains == 2
        n = B * HID * H * W * 4
        bias = (B * -(-H * W // 64) * 3 * HID * 4 + 255) // 256 * 256
        assert workspace_bytes(B, H, W) == 13 * n + bias + B * nsl * 5 * 2 * HID * (HID + INP) * 4


@pytest.mark.parametrize("shape,scale", [(SLAB_SHAPES[0], 1), (SLAB_SHAPES[0], 8), (SLAB_SHAPES[1], 1)],
                         ids=lambda v: "x".join(map(str, v)) if isinstance(v, tuple) else f"w{v}")
def test_accuracy_doubled_cap(shape, scale):
    """test_accuracy's bars at SLAB_SHAPES, the bias gradients under the weights' form of bar (module docstring)."""
    assert slab_rule(shape[0], shape[1] * shape[2])[3] == 2
    h, x, go, ref, aten = case(shape, scale)
    got, _ = ours(h, x, go, train_mod(scale))
    for g, r in zip(got, ref):
        assert g.shape == r.shape and np.isfinite(g).all()
    errs = [normwise(g, r) for g, r in zip(got, ref)]
    aerr = [normwise(a, r) for a, r in zip(aten, ref)]
    wworst, aworst = max(errs[2:8]), max(aerr[2:8])
    bworst, abworst = max(errs[8:]), max(aerr[8:])
    wpool, apool = pooled(got[2:8], ref[2:8]), pooled(aten[2:8], ref[2:8])
    print(f"sepconv_gru backward {shape} weights*{scale}: max|err|/rms(ref) grad_h {errs[0]:.3g} (ATen fp32 "
          f"{aerr[0]:.3g}), grad_x {errs[1]:.3g} ({aerr[1]:.3g}), bias worst {bworst:.3g} ({abworst:.3g}), weight "
          f"worst {wworst:.3g} ({aworst:.3g}), weight pooled Frobenius {wpool:.3g} ({apool:.3g})")
    assert errs[0] <= BAR and errs[1] <= BAR
    assert bworst <= max(BAR, 4 * abworst), NAMES[8 + int(np.argmax(errs[8:]))]
    assert wworst <= max(BAR, 4 * aworst)
    assert wpool <= 4 * apool


def test_forward_unchanged():
    """With grad on, sepconv_gru_train returns bitwise what sepconv_gru returns under no_grad."""
    import eraft_amd
    h, x, go, _, _ = case((2, 7, 70), 1)
    mod = train_mod(1)
    _, out = ours(h, x, go, mod)
    with torch.no_grad():
        plain = eraft_amd.sepconv_gru(h.cuda(), x.cuda(), mod)
        again = eraft_amd.sepconv_gru_train(h.cuda(), x.cuda(), mod)
    assert not again.requires_grad
    d = mismatch(out.cpu().numpy(), plain.cpu().numpy())
    assert d is None, d
    assert torch.equal(again, plain)
    frozen = copy.deepcopy(mod).requires_grad_(False)   # nothing requires grad: the plain forward, no node
    res = eraft_amd.sepconv_gru_train(h.cuda(), x.cuda(), frozen)
    assert res.grad_fn is None and torch.equal(res, plain)


@pytest.mark.parametrize("where", ["interior", "row_end", "row_start", "first_row", "last_row"])
def test_footprint(where):
    """grad_out nonzero at one pixel of item 0 (all channels): grad_h and grad_x are == 0 outside the 9 x 9 block
    around it clipped to the image (two taps for q and two more for r, per half-step) and in item 1.  At a row
    end the flattened neighbours are the next row's first pixels (x axis) and on the first / last row the
    neighbouring channel's rows (y axis): a wrap would land outside the clipped block."""
    B, H, W = 2, 12, 14
    h, x, go = inputs((B, H, W))
    y0, x0 = {"interior": (5, 6), "row_end": (5, W - 1), "row_start": (6, 0), "first_row": (0, 6),
              "last_row": (H - 1, 7)}[where]
    keep = torch.zeros(B, 1, H, W)
    keep[0, 0, y0, x0] = 1
    got, _ = ours(h, x, go * keep, train_mod(1))
    block = np.zeros((H, W), dtype=bool)
    block[max(y0 - 4, 0):y0 + 5, max(x0 - 4, 0):x0 + 5] = True
    assert not block.all()
    for name, g in zip(NAMES[:2], got[:2]):
        assert np.isfinite(g).all()
        assert (g[1] == 0).all(), f"{name}: item 1"
        assert (g[0][:, ~block] == 0).all(), f"{name}: outside the block"
        assert (g[0][:, block] != 0).any(axis=0).all(), f"{name}: a pixel of the block got nothing"


def sizes():
    import eraft_amd
    n = ctypes.c_int64()
    assert eraft_amd.lib().ecorr_sepconv_gru_backward_packed_size(HID, INP, ctypes.byref(n)) == 0
    return n.value


def workspace_bytes(B, H, W):
    import eraft_amd
    n = ctypes.c_int64()
    assert eraft_amd.lib().ecorr_sepconv_gru_backward_workspace_size(B, HID, INP, H, W, ctypes.byref(n)) == 0
    return n.value


def raw_packs(mod):
    """(packed, packed_t) of mod's weights through the raw pack entries."""
    import eraft_amd
    from eraft_amd import _lib
    L = eraft_amd.lib()
    ws = [getattr(mod, c).weight.detach().contiguous() for c in CONVS]
    bs = [getattr(mod, c).bias.detach().contiguous() for c in CONVS]
    st = _lib.stream_of(ws[0])
    n = ctypes.c_int64()
    assert L.ecorr_sepconv_gru_packed_size(HID, INP, ctypes.byref(n)) == 0
    packed = torch.empty(n.value, dtype=torch.uint8, device="cuda")
    packed_t = torch.empty(sizes(), dtype=torch.uint8, device="cuda")
    wp = (ctypes.c_void_p * 6)(*[t.data_ptr() for t in ws])
    bp = (ctypes.c_void_p * 6)(*[t.data_ptr() for t in bs])
    assert L.ecorr_sepconv_gru_pack(wp, bp, HID, INP, packed.data_ptr(), st) == 0
    assert L.ecorr_sepconv_gru_backward_pack(wp, HID, INP, packed_t.data_ptr(), st) == 0
    torch.cuda.synchronize()
    return packed, packed_t


def raw_backward(hd, xd, god, packs, outs, ws_ptr):
    """ecorr_sepconv_gru_backward on device tensors into the 14 device float tensors `outs` (NAMES order)."""
    import eraft_amd
    from eraft_amd import _lib
    B, _, H, W = hd.shape
    gw = (ctypes.c_void_p * 6)(*[t.data_ptr() for t in outs[2:8]])
    gb = (ctypes.c_void_p * 6)(*[t.data_ptr() for t in outs[8:]])
    assert eraft_amd.lib().ecorr_sepconv_gru_backward(
        hd.data_ptr(), xd.data_ptr(), god.data_ptr(), B, HID, INP, H, W, packs[0].data_ptr(), packs[1].data_ptr(),
        outs[0].data_ptr(), outs[1].data_ptr(), gw, gb, ws_ptr, _lib.stream_of(hd)) == 0


def out_sizes(B, H, W):
    return [B * HID * H * W, B * INP * H * W] + [HID * (HID + INP) * 5] * 6 + [HID] * 6


@pytest.mark.parametrize("shape", [(2, 7, 70), (1, 2, 2), (2, 40, 50), SLAB_SHAPES[0]],
                         ids=lambda s: "x".join(map(str, s)))
def test_guards_and_raw_abi(shape):
    """All 14 outputs between guard bands and a workspace of exactly the reported size between guards, prefilled
    with 0xff bytes (a read before a write is a NaN): the guards stay, every output element is written, the bits
    are those of the Python path, and the recomputed h' in the workspace is bitwise the forward's."""
    import eraft_amd
    B, H, W = shape
    h, x, go, _, _ = case(shape, 1)
    mod = train_mod(1)
    want, fwd = ours(h, x, go, mod)
    hd, xd, god = h.cuda(), x.cuda(), go.cuda()
    packs = raw_packs(mod)
    bufs = [guarded(n) for n in out_sizes(B, H, W)]
    ws = Workspace(workspace_bytes(B, H, W), 0xff)
    raw_backward(hd, xd, god, packs, [b[1] for b in bufs], ws.ptr)
    torch.cuda.synchronize()
    ws.check("sepconv_gru backward workspace")
    for name, (buf, _), w in zip(NAMES, bufs, want):
        got = check_guarded(buf, f"sepconv_gru backward {name}")
        assert np.isfinite(got).all(), name
        d = mismatch(got.reshape(1, 1, -1), w.reshape(1, 1, -1))
        assert d is None, f"{name}: raw ABI against sepconv_gru_train: {d}"
    n = B * HID * H * W
    from gpu_guard import WS_GUARD
    redone = ws.buf[WS_GUARD + 7 * n * 4:WS_GUARD + 8 * n * 4].view(torch.float32).cpu().numpy()
    d = mismatch(redone.reshape(B, HID, -1), fwd.cpu().numpy().reshape(B, HID, -1))
    assert d is None, f"the recomputed h' against the forward's: {d}"
    with torch.no_grad():
        assert torch.equal(fwd, eraft_amd.sepconv_gru(hd, xd, mod))


def test_two_calls_same_bits():
    h, x, go, _, _ = case((2, 40, 50), 1)
    a, _ = ours(h, x, go, train_mod(1))
    b, _ = ours(h, x, go, train_mod(1))
    for name, p, q in zip(NAMES, a, b):
        d = mismatch(p.reshape(1, 1, -1), q.reshape(1, 1, -1))
        assert d is None, f"{name}: {d}"


def test_two_calls_same_bits_doubled_cap():
    """Two chains per slab and 44 slabs: the chain sum and the slab reduction have one order."""
    h, x, go, _, _ = case(SLAB_SHAPES[1], 1)
    a, _ = ours(h, x, go, train_mod(1))
    b, _ = ours(h, x, go, train_mod(1))
    for name, p, q in zip(NAMES, a, b):
        d = mismatch(p.reshape(1, 1, -1), q.reshape(1, 1, -1))
        assert d is None, f"{name}: {d}"


def test_selective_outputs():
    h, x, go, _, _ = case((2, 7, 70), 1)
    full, _ = ours(h, x, go, train_mod(1))
    frozen = copy.deepcopy(gpu_module(1)).requires_grad_(False)
    got, _ = ours(h, x, go, frozen)
    assert all(g is None for g in got[2:])
    for k in (0, 1):
        d = mismatch(got[k], full[k])
        assert d is None, f"frozen GRU, {NAMES[k]}: {d}"
    got, _ = ours(h, x, go, train_mod(1), need_h=False, need_x=False)
    assert got[0] is None and got[1] is None
    for name, p, q in zip(NAMES[2:], got[2:], full[2:]):
        d = mismatch(p.reshape(1, 1, -1), q.reshape(1, 1, -1))
        assert d is None, f"detached h and x, {name}: {d}"
    for nh, nx in ((True, False), (False, True)):   # one of the two data gradients
        got, _ = ours(h, x, go, frozen, need_h=nh, need_x=nx)
        k = 0 if nh else 1
        assert got[1 - k] is None
        d = mismatch(got[k], full[k])
        assert d is None, f"{NAMES[k]} alone: {d}"


def test_weight_cache_follows_updates():
    """After an in-place optimizer-style update and after load_state_dict the next forward + backward uses the new
    weights: both packs are repacked, the result is a fresh module's bit for bit."""
    from eraft_amd import gru as G
    h, x, go, _, _ = case((1, 15, 20), 1)
    mod = train_mod(1)
    before, _ = ours(h, x, go, mod)
    packs = (G._packs[mod][2], G._packs_t[mod][2])
    with torch.no_grad():
        for p in mod.parameters():
            p.add_(p, alpha=0.25)
    after, _ = ours(h, x, go, mod)
    assert G._packs[mod][2] is not packs[0] and G._packs_t[mod][2] is not packs[1]
    fresh = copy.deepcopy(mod)
    want, _ = ours(h, x, go, fresh)
    for name, p, q, r in zip(NAMES, after, want, before):
        d = mismatch(p.reshape(1, 1, -1), q.reshape(1, 1, -1))
        assert d is None, f"after the update, {name}: {d}"
        assert (p != r).any(), name
    mod.load_state_dict(gpu_module(1).state_dict())
    again, _ = ours(h, x, go, mod)
    for name, p, r in zip(NAMES, again, before):
        d = mismatch(p.reshape(1, 1, -1), r.reshape(1, 1, -1))
        assert d is None, f"after load_state_dict, {name}: {d}"


def test_graph_capture():
    """The raw ecorr_sepconv_gru_backward call captured and replayed on changed inputs equals eager."""
    B, H, W = 2, 7, 70
    sets = [make_inputs(200 + 10 * i, B, H, W) + (torch.from_numpy(prng.normal(900 + i, (B, HID, H, W))),)
            for i in range(2)]
    sets = [tuple(t.cuda() for t in s) for s in sets]
    hd, xd, god = (t.clone() for t in sets[0])
    packs = raw_packs(gpu_module(1))
    nbytes = workspace_bytes(B, H, W)
    outs = []

    def step():
        outs[:] = [torch.empty(n, dtype=torch.float32, device="cuda") for n in out_sizes(B, H, W)]
        ws = torch.empty(nbytes, dtype=torch.uint8, device="cuda")
        raw_backward(hd, xd, god, packs, outs, ws.data_ptr())

    def mutate(i):
        for dst, src in zip((hd, xd, god), sets[i]):
            dst.copy_(src)

    replay_matches_eager(step, mutate, outs)


def test_refusals():
    import eraft_amd
    h, x, go, _, _ = case((1, 2, 2), 1)
    mod = train_mod(1)
    hd, xd = h.cuda().requires_grad_(True), x.cuda()
    # a second backward without retain_graph behaves as autograd does
    loss = (eraft_amd.sepconv_gru_train(hd, xd, mod) * go.cuda()).sum()
    loss.backward()
    with pytest.raises(RuntimeError, match="second time"):
        loss.backward()
    loss = (eraft_amd.sepconv_gru_train(hd, xd, mod) * go.cuda()).sum()
    hd.grad = None
    loss.backward(retain_graph=True)
    first = hd.grad.clone()
    hd.grad = None
    loss.backward()
    assert torch.equal(hd.grad, first)
    # an in-place change of the saved h raises
    hc = h.cuda()
    out = eraft_amd.sepconv_gru_train(hc, xd, mod)
    hc.add_(1.0)
    with pytest.raises(RuntimeError, match="modified by an inplace operation"):
        out.sum().backward()
    # the checks of sepconv_gru; unsupported sizes raise ValueError before the weights are looked at
    fresh = train_mod(1)
    with pytest.raises(ValueError):
        eraft_amd.sepconv_gru_train(hd[:, :64].contiguous(), xd, fresh)
    with pytest.raises(ValueError):
        eraft_amd.sepconv_gru_train(hd, xd[:, :128].contiguous(), object())
    with pytest.raises(TypeError):
        eraft_amd.sepconv_gru_train(hd.half(), xd, mod)
    with pytest.raises(RuntimeError, match="HIP devices"):
        eraft_amd.sepconv_gru_train(h, xd, mod)
    with pytest.raises(RuntimeError):
        eraft_amd.sepconv_gru_train(hd, xd.transpose(2, 3), mod)
    with pytest.raises(RuntimeError, match="forward-only"):   # the forward-only entry keeps its refusal
        eraft_amd.sepconv_gru(hd, xd, mod)
