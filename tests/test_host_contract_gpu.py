"""The host layer's contract on a HIP device, as a table: every invalid call with its exception type
and full text (literals: a change of wording has to change this file), and the number of device
allocations that one call of each hot entry makes.  Each row prints `CONTRACT <id>: <type>: <text>`
(pytest -s), so two versions of the package can be compared line by line."""
import os
import socket
import types

import numpy as np
import pytest
import torch
import torch.distributed as dist

from conftest import ROOT  # noqa: F401  (puts the repo root on sys.path)

import eraft_amd
from eraft_amd import _lib
from eraft_amd.rowshard import RowShardedCorrBlock

pytestmark = pytest.mark.gpu

B, D, H, W, L, R = 1, 8, 8, 8, 2, 1
C = L * (2 * R + 1) ** 2   # 18 correlation channels

FORWARD_ONLY = ("eraft_amd CorrBlock is forward-only; call it under torch.no_grad() "
                "(as the reference harness does, test.py:80)")
COORDS_GRAD = ("differentiable CorrBlock: coords requires grad; detach it (as eraft.py:127 does), "
               "there is no gradient with respect to the coordinates")
CONSUMED = ("eraft_amd CorrBlock: backward through a block whose gradient was already "
            "consumed (one backward per differentiable block)")
BAD_SHAPES = "fmap shapes {} / {} differ or are not [B, D, H, W]"


@pytest.fixture(scope="module")
def s():
    """The valid inputs, a plain block, a live differentiable one and a one-process row-sharded one."""
    dev = torch.device("cuda", 0)
    g = torch.Generator(device="cpu").manual_seed(7)

    def randn(*shape):
        return torch.randn(*shape, generator=g).to(dev)

    ns = types.SimpleNamespace(dev=dev, randn=randn)
    ns.zeros = lambda *shape, **kw: torch.zeros(*shape, device=dev, **kw)
    ns.f1, ns.f2 = randn(B, D, H, W), randn(B, D, H, W)
    ns.coords = eraft_amd.coords_grid(B, H, W, device=dev) + 0.25
    ns.weight, ns.bias = randn(64, C, 1, 1), randn(64)
    ns.png_twos = torch.from_numpy(np.full((4, 4, 3), 2, dtype=np.uint16)).to(dev)   # channel 2 outside {0, 1}
    with torch.no_grad():
        ns.plain = eraft_amd.CorrBlock(ns.f1, ns.f2, num_levels=L, radius=R)
    ns.live_block = lambda: eraft_amd.CorrBlock(ns.f1.clone().requires_grad_(True), ns.f2, num_levels=L, radius=R,
                                                differentiable=True)
    ns.live = ns.live_block()
    started = not dist.is_initialized()
    if started:
        with socket.socket() as sock:
            sock.bind(("127.0.0.1", 0))
            port = sock.getsockname()[1]
        os.environ.update(MASTER_ADDR="127.0.0.1", MASTER_PORT=str(port))
        dist.init_process_group("gloo", rank=0, world_size=1)
    try:
        with torch.no_grad():
            ns.rows = RowShardedCorrBlock(ns.f1, ns.f2, num_levels=L, radius=R)
        yield ns
    finally:
        if started:
            dist.destroy_process_group()


def _block(s, f1, f2=None, **kw):
    with torch.no_grad():
        return eraft_amd.CorrBlock(f1, f1 if f2 is None else f2, num_levels=L, radius=R, **kw)


def _second_backward(s, conv):
    blk = s.live_block()
    out = blk.lookup_conv1x1_relu(s.coords, s.weight, s.bias) if conv else blk(s.coords)
    loss = out.sum()
    loss.backward(retain_graph=True)
    loss.backward()


def _events(s, n, **other):
    ev = {k: s.zeros(n) for k in "ptxy"}
    ev.update(other)
    return ev


VG = eraft_amd.VoxelGrid((3, 4, 4), normalize=True)

# (id, call(s), exception type, full message)
ROWS = [
    # the fmaps of CorrBlock
    ("fmap1-dtype", lambda s: _block(s, s.f1.half(), s.f2), TypeError, "fmap1 must be float32 (got torch.float16)"),
    ("fmap2-dtype", lambda s: _block(s, s.f1, s.f2.double()), TypeError, "fmap2 must be float32 (got torch.float64)"),
    ("fmap-rank", lambda s: _block(s, s.f1[0], s.f2[0]), RuntimeError, BAD_SHAPES.format((D, H, W), (D, H, W))),
    ("fmap-shapes", lambda s: _block(s, s.f1, s.zeros(B, D, H, W + 1)), RuntimeError,
     BAD_SHAPES.format((B, D, H, W), (B, D, H, W + 1))),
    ("fmap-strides", lambda s: _block(s, s.f1.transpose(2, 3)), RuntimeError,
     "fmap1/fmap2 must be contiguous (reference: view size is not compatible with input tensor's size and stride)"),
    ("fmap-empty-batch", lambda s: _block(s, s.zeros(0, D, H, W)), RuntimeError,
     f"cannot reshape tensor of 0 elements into shape [0, {H}, {W}, -1] "
     "(empty batch: the reference's CorrBlock.corr reshape)"),
    ("fmap-empty-map", lambda s: _block(s, s.zeros(B, D, 0, W)), RuntimeError,
     f"Expected 3D or 4D (batch mode) tensor with optional 0 dim batch size for input, but got:[0, 1, 0, {W}] "
     "(empty map: the reference's avg_pool2d)"),
    ("fmap-grad-plain", lambda s: eraft_amd.CorrBlock(s.f1.clone().requires_grad_(True), s.f2, L, R), RuntimeError,
     FORWARD_ONLY),
    ("rows-fmap-dtype", lambda s: RowShardedCorrBlock(s.f1.half(), s.f2, L, R), TypeError,
     "fmap1 must be float32 (got torch.float16)"),
    ("rows-fmap-shapes", lambda s: RowShardedCorrBlock(s.f1, s.zeros(B, D, H, W + 1), L, R), RuntimeError,
     BAD_SHAPES.format((B, D, H, W), (B, D, H, W + 1))),
    ("rows-fmap-grad", lambda s: RowShardedCorrBlock(s.f1.clone().requires_grad_(True), s.f2, L, R), RuntimeError,
     FORWARD_ONLY),
    ("rows-slabs-rows", lambda s: RowShardedCorrBlock.from_row_slabs(s.f1[:, :, :H - 1], s.f2[:, :, :H - 1], H, L, R),
     RuntimeError, f"rank 0: row slabs {(B, D, H - 1, W)} / {(B, D, H - 1, W)} do not match {H} rows"),
    # coords
    ("coords-list", lambda s: s.plain([0.0]), TypeError, "coords must be a torch.Tensor"),
    ("coords-cpu", lambda s: s.plain(s.coords.cpu()), RuntimeError,
     "coords is on cpu: eraft_amd runs only on HIP devices (no CPU path)"),
    ("coords-dtype", lambda s: s.plain(s.coords.half()), TypeError, "coords must be float32 (got torch.float16)"),
    ("coords-shape", lambda s: s.plain(s.zeros(B, 2, H, W + 1)), RuntimeError,
     f"coords shape {(B, 2, H, W + 1)} != {(B, 2, H, W)} of the pyramid"),
    ("coords-shape-conv", lambda s: s.plain.lookup_conv1x1_relu(s.zeros(B, 3, H, W), s.weight, s.bias), RuntimeError,
     f"coords shape {(B, 3, H, W)} != {(B, 2, H, W)} of the pyramid"),
    ("coords-shape-live", lambda s: s.live(s.zeros(B, 2, H, W + 1)), RuntimeError,
     f"coords shape {(B, 2, H, W + 1)} != {(B, 2, H, W)} of the pyramid"),
    ("coords-shape-rows", lambda s: s.rows(s.zeros(B, 2, H, W + 1)), RuntimeError,
     f"coords shape {(B, 2, H, W + 1)} != {(B, 2, H, W)}"),
    ("coords-grad-plain", lambda s: s.plain(s.coords.clone().requires_grad_(True)), RuntimeError, FORWARD_ONLY),
    ("coords-grad-plain-conv",
     lambda s: s.plain.lookup_conv1x1_relu(s.coords.clone().requires_grad_(True), s.weight, s.bias), RuntimeError,
     FORWARD_ONLY),
    ("coords-grad-rows", lambda s: s.rows(s.coords.clone().requires_grad_(True)), RuntimeError, FORWARD_ONLY),
    ("coords-grad-live", lambda s: s.live(s.coords.clone().requires_grad_(True)), RuntimeError, COORDS_GRAD),
    ("coords-grad-live-conv",
     lambda s: s.live.lookup_conv1x1_relu(s.coords.clone().requires_grad_(True), s.weight, s.bias), RuntimeError,
     COORDS_GRAD),
    # requires grad is looked at before the shape
    ("coords-grad-before-shape", lambda s: s.live(s.zeros(B, 2, H, W + 1).requires_grad_(True)), RuntimeError,
     COORDS_GRAD),
    ("coords-grad-before-shape-conv",
     lambda s: s.live.lookup_conv1x1_relu(s.zeros(B, 2, H, W + 1).requires_grad_(True), s.weight, s.bias),
     RuntimeError, COORDS_GRAD),
    # weight, bias and mode of lookup_conv1x1_relu
    ("weight-count", lambda s: s.plain.lookup_conv1x1_relu(s.coords, s.zeros(64, C - 1)), RuntimeError,
     f"weight (64, {C - 1}) does not map {C} correlation channels"),
    ("weight-count-live", lambda s: s.live.lookup_conv1x1_relu(s.coords, s.zeros(64, C - 1)), RuntimeError,
     f"weight (64, {C - 1}) does not map {C} correlation channels"),
    ("weight-list", lambda s: s.plain.lookup_conv1x1_relu(s.coords, [1.0]), TypeError, "weight must be a torch.Tensor"),
    ("weight-list-live", lambda s: s.live.lookup_conv1x1_relu(s.coords, [1.0]), TypeError,
     "weight must be a torch.Tensor"),
    ("weight-dtype", lambda s: s.plain.lookup_conv1x1_relu(s.coords, s.weight.half()), TypeError,
     "weight must be float32 (got torch.float16)"),
    ("weight-grad-plain", lambda s: s.plain.lookup_conv1x1_relu(s.coords, s.weight.clone().requires_grad_(True)),
     RuntimeError, FORWARD_ONLY),
    ("bias-length", lambda s: s.plain.lookup_conv1x1_relu(s.coords, s.weight, s.zeros(63)), RuntimeError,
     "bias has 63 elements, expected 64"),
    ("bias-dtype", lambda s: s.plain.lookup_conv1x1_relu(s.coords, s.weight, s.bias.half()), TypeError,
     "bias must be float32 (got torch.float16)"),
    ("fused-o8", lambda s: s.plain.lookup_conv1x1_relu(s.coords, s.zeros(8, C), mode="fused"), RuntimeError,
     "8 output channels: the fused kernel needs a positive multiple of 64"),
    ("mode-unknown", lambda s: s.plain.lookup_conv1x1_relu(s.coords, s.weight, s.bias, mode="bogus"), ValueError,
     "mode 'bogus': expected 'split', 'presplit' or 'fused'"),
    ("mode-presplit-rows", lambda s: s.rows.lookup_conv1x1_relu(s.coords, s.weight, s.bias, mode="presplit"),
     ValueError, "mode 'presplit': expected 'split' or 'fused'"),
    ("out-dtype", lambda s: s.plain(s.coords, out_dtype=torch.float64), TypeError,
     "out_dtype must be None, torch.float32, torch.float16 or torch.bfloat16 (got torch.float64)"),
    ("out-dtype-rows", lambda s: s.rows(s.coords, out_dtype=torch.float16), NotImplementedError,
     "RowShardedCorrBlock: out_dtype=torch.float16 is not supported, the row exchange "
     "carries fp32 lookups only; call it without out_dtype and cast the result"),
    # one backward per differentiable block
    ("second-backward", lambda s: _second_backward(s, conv=False), RuntimeError, CONSUMED),
    ("second-backward-conv", lambda s: _second_backward(s, conv=True), RuntimeError, CONSUMED),
    # the sampler, the flow side, the splat and the voxel grid
    ("sampler-shapes", lambda s: eraft_amd.bilinear_sampler(s.f1, s.zeros(B, H, W, 3)), RuntimeError,
     f"bilinear_sampler: img {(B, D, H, W)} / coords {(B, H, W, 3)}"),
    ("sampler-grad", lambda s: eraft_amd.bilinear_sampler(s.f1.clone().requires_grad_(True), s.zeros(B, H, W, 2)),
     RuntimeError, FORWARD_ONLY),
    ("sampler-dtype", lambda s: eraft_amd.bilinear_sampler(s.f1, s.zeros(B, H, W, 2).half()), TypeError,
     "coords must be float32 (got torch.float16)"),
    ("upsample-mask-size", lambda s: eraft_amd.upsample_flow(s.zeros(1, 2, 4, 4), s.zeros(1, 575, 4, 4)),
     RuntimeError, "shape '[1, 1, 9, 8, 8, 4, 4]' is invalid for input of size 9200"),
    ("upsample-flow-shape", lambda s: eraft_amd.upsample_flow(s.zeros(1, 3, 4, 4), s.zeros(1, 576, 4, 4)),
     RuntimeError, "flow must be [N, 2, H, W], got (1, 3, 4, 4)"),
    ("upsample-mask-dtype", lambda s: eraft_amd.upsample_flow(s.zeros(1, 2, 4, 4), s.zeros(1, 576, 4, 4).half()),
     TypeError, "mask must be float32 (got torch.float16)"),
    ("png16-dtype", lambda s: eraft_amd.flow_to_png16(s.zeros(2, 4, 4).double()), TypeError,
     "flow must be float32 (got torch.float64)"),
    ("png16-shape", lambda s: eraft_amd.flow_to_png16(s.zeros(3, 4, 4)), RuntimeError,
     "flow must be [2, h, w] or [B, 2, h, w], got (3, 4, 4)"),
    ("from16-invalid-pixel", lambda s: eraft_amd.flow_16bit_to_float(s.png_twos), AssertionError,
     "flow_16bit: invalid pixels must have channel 2 == 0"),
    ("splat-channels", lambda s: eraft_amd.forward_interpolate_pytorch(s.zeros(1, 3, 4, 4)), RuntimeError,
     "flow must be [B, 2, H, W], got (1, 3, 4, 4)"),
    ("splat-dtype", lambda s: eraft_amd.forward_interpolate_pytorch(s.zeros(1, 2, 4, 4).half()), TypeError,
     "flow_in must be float32 (got torch.float16)"),
    ("grid-sample-rows", lambda s: eraft_amd.grid_sample_values(s.zeros(2, 5), 4, 4), RuntimeError,
     "input must be [3, N] (x, y, z), got (2, 5)"),
    ("voxel-dtype", lambda s: VG.convert(_events(s, 5, t=s.zeros(5).double())), RuntimeError,
     "events['t'] must be a float32 HIP tensor (no CPU path)"),
    ("voxel-lengths", lambda s: VG.convert(_events(s, 5, y=s.zeros(4))), RuntimeError,
     "events p, t, x, y differ in length"),
    ("voxel-empty", lambda s: VG.convert(_events(s, 0)), IndexError,
     "index 0 is out of bounds for dimension 0 with size 0"),
]


@pytest.mark.parametrize("row", ROWS, ids=[r[0] for r in ROWS])
def test_invalid_call(s, row):
    name, call, exc, msg = row
    with pytest.raises(Exception) as e:
        call(s)
    print(f"\nCONTRACT {name}: {type(e.value).__name__}: {e.value}")
    assert type(e.value) is exc
    assert str(e.value) == msg


def test_blocks_still_serve_after_the_rejections(s):
    """No rejected call left a block unusable: the three blocks give the same lookup bits."""
    with torch.no_grad():
        a = s.plain(s.coords)
        b = s.rows(s.coords)
    c = s.live(s.coords)
    assert tuple(a.shape) == (B, C, H, W)
    assert torch.equal(a, b) and torch.equal(a, c.detach())


# device allocations of one call (after one warm-up call: the packed weight and the workspace sizes are cached)
ALLOCATIONS = {
    "lookup": 1,             # the output
    "lookup_conv split": 3,  # the output, the lookup and its per-query maxima
    "lookup_conv fused": 1,  # the output
    "build split": 2,        # the pyramid and the operand workspace
    "build fp32": 1,         # the pyramid
    "upsample forward": 1,   # the output
    "upsample backward": 3,  # the workspace and the two gradients
}


def _allocations(call):
    call()
    torch.cuda.synchronize()
    n0 = torch.cuda.memory_stats()["allocation.all.allocated"]
    keep = call()   # noqa: F841  (the result lives until the count is read)
    return torch.cuda.memory_stats()["allocation.all.allocated"] - n0


def test_device_allocations_per_call(s):
    sb, sd, sh, sw = 2, 64, 16, 24   # the smallest shape of tests/test_motion_gpu.py's dense case
    f1, f2 = s.randn(sb, sd, sh, sw), s.randn(sb, sd, sh, sw)
    coords = eraft_amd.coords_grid(sb, sh, sw, device=s.dev) + 0.25
    weight, bias = s.randn(256, 324, 1, 1), s.randn(256)
    flow, mask, go = s.randn(1, 2, 8, 8), s.randn(1, 576, 8, 8), s.randn(1, 2, 64, 64)
    flow_g, mask_g = flow.clone().requires_grad_(True), mask.clone().requires_grad_(True)
    prev = _lib.build_mode()
    got = {}
    try:
        with torch.no_grad():
            blk = eraft_amd.CorrBlock(f1, f2)
            got["lookup"] = _allocations(lambda: blk(coords))
            got["lookup_conv split"] = _allocations(lambda: blk.lookup_conv1x1_relu(coords, weight, bias, mode="split"))
            got["lookup_conv fused"] = _allocations(lambda: blk.lookup_conv1x1_relu(coords, weight, bias, mode="fused"))
            for mode in ("split", "fp32"):
                _lib.set_build_mode(mode)
                got[f"build {mode}"] = _allocations(lambda: eraft_amd.CorrBlock(f1, f2)._pyramid)
            got["upsample forward"] = _allocations(lambda: eraft_amd.upsample_flow(flow, mask))
        up = eraft_amd.upsample_flow(flow_g, mask_g)
        got["upsample backward"] = _allocations(
            lambda: torch.autograd.grad(up, (flow_g, mask_g), go, retain_graph=True))
    finally:
        _lib.set_build_mode(prev)
    for name, n in got.items():
        print(f"\nCONTRACT allocations {name}: {n}")
    assert got == ALLOCATIONS
