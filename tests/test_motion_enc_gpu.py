"""eraft_amd.motion_encoder / ecorr_motion_encoder (csrc/motion_enc.hip) against an fp64 BasicMotionEncoder on the CPU.

Reference: network.BasicMotionEncoder().double() on the CPU, fed the same fp32 inputs with corr_is_convc1=True
(the e2e goldens pin that module to the reference's update.py:63-81).  Inputs from tests/prng.py: c1 =
relu(normal), flow = 3 * normal; weights and biases at PyTorch's default scales as tests/e2e_weights.py draws them.

Accuracy bar: max |got - ref| / rms(ref) <= 1e-5 on channels 0-125, the project's normwise bar for every GEMM (the
fp32 ATen encoder on the CPU gives 3.3e-7 .. 2.2e-6 at these shapes and inputs); channels 126-127 are flow, bit
for bit.  ReLU networks are scale-homogeneous, so the GRU tests' weights * 8 case is not repeated.
Shapes: H or W (or both) shorter than every tap reach, 65 pixels (one past the 64-pixel tile of convf1 and
convc2), 129 pixels (one past the 128-pixel tile of convf2 and conv), 135 pixels over three batch items (ragged
tiles crossing row ends, batch offsets), exactly 128, a tile edge inside a row, and a pyramid-sized map.
"""
import copy
import ctypes
import functools

import numpy as np
import pytest
import torch

import prng
from e2e_weights import make_state_dict
from gpu_guard import FILL, GUARD, Workspace, guarded, mismatch
from graph_capture import replay_matches_eager

pytestmark = pytest.mark.gpu

C1, OUT, CONV = 256, 128, 126
BAR = 1e-5
SHAPES = [(1, 1, 1), (2, 1, 7), (1, 7, 1), (2, 3, 5), (1, 5, 13), (3, 9, 15), (2, 8, 16), (1, 2, 70), (1, 15, 20),
          (1, 3, 43)]


@pytest.fixture(autouse=True)
def _device():
    if not torch.cuda.is_available():
        pytest.fail("no HIP device visible")


def make_inputs(seed, B, H, W):
    c1 = np.maximum(prng.normal(seed, (B, C1, H, W)), 0).astype(np.float32)
    flow = prng.normal(seed + 1, (B, 2, H, W), 3.0).astype(np.float32)
    return torch.from_numpy(np.ascontiguousarray(flow)), torch.from_numpy(np.ascontiguousarray(c1))


@functools.lru_cache(maxsize=None)
def cpu_module():
    """The fp32 module on the CPU with the PRNG weights."""
    from eraft_amd import network
    mod = network.BasicMotionEncoder()
    mod.load_state_dict(make_state_dict(mod.state_dict()))
    return mod.eval().requires_grad_(False)


@functools.lru_cache(maxsize=None)
def gpu_module():
    return copy.deepcopy(cpu_module()).cuda()


@functools.lru_cache(maxsize=None)
def case(shape):
    """(flow, c1) on the CPU and the fp64 reference, computed once per shape and never changed."""
    B, H, W = shape
    flow, c1 = make_inputs(300 + 7 * H + W, B, H, W)
    with torch.no_grad():
        ref = copy.deepcopy(cpu_module()).double()(flow.double(), c1.double(), corr_is_convc1=True).numpy()
    return flow, c1, ref


def normwise(got, ref):
    d = np.abs(np.asarray(got, np.float64) - ref).max()
    return float(d / np.sqrt(np.mean(ref * ref)))


def run(flow, c1, mod=None, out=None):
    import eraft_amd
    with torch.no_grad():
        res = eraft_amd.motion_encoder(flow.cuda(), c1.cuda(), mod or gpu_module(), out=out)
    torch.cuda.synchronize()
    return res.cpu().numpy()


@pytest.mark.parametrize("shape", SHAPES, ids=lambda s: "x".join(map(str, s)))
def test_accuracy(shape):
    flow, c1, ref = case(shape)
    got = run(flow, c1)
    assert got.shape == ref.shape == (shape[0], OUT, shape[1], shape[2])
    err = normwise(got[:, :CONV], ref[:, :CONV])
    print(f"motion_encoder {shape}: max|err|/rms(ref) = {err:.3g} (rms {np.sqrt(np.mean(ref[:, :CONV] ** 2)):.3g})")
    assert np.isfinite(got).all()
    assert err <= BAR
    d = mismatch(got[:, CONV:], flow.numpy())
    assert d is None, f"channels 126-127 against flow: {d}"


def test_batch_independence_and_two_calls():
    """Item b of the B = 3 run is the B = 1 run of that item, and a second run of the same call the first, bit for
    bit."""
    flow, c1, _ = case((3, 9, 15))
    whole = run(flow, c1)
    d = mismatch(run(flow, c1), whole)
    assert d is None, f"two runs: {d}"
    for b in range(3):
        d = mismatch(run(flow[b:b + 1].contiguous(), c1[b:b + 1].contiguous()), whole[b:b + 1])
        assert d is None, f"item {b}: {d}"


@pytest.mark.parametrize("shape", [(3, 9, 15), (1, 2, 70)], ids=lambda s: "x".join(map(str, s)))
def test_strided_out_is_the_upper_half_of_x(shape):
    """out = x[:, 128:] of a guarded [B, 256, H, W] buffer: the bits of the contiguous call; x[:, :128] and the
    guard bands keep their fill."""
    B, H, W = shape
    flow, c1, _ = case(shape)
    plain = run(flow, c1)
    buf, mid = guarded(B * 256 * H * W)
    x = mid.view(B, 256, H, W)
    import eraft_amd
    with torch.no_grad():
        ret = eraft_amd.motion_encoder(flow.cuda(), c1.cuda(), gpu_module(), out=x[:, 128:])
    torch.cuda.synchronize()
    assert ret.data_ptr() == x[:, 128:].data_ptr() and ret.shape == (B, OUT, H, W)
    host = buf.cpu().numpy()
    assert (host[:GUARD] == FILL).all() and (host[-GUARD:] == FILL).all(), "a guard band was written"
    xs = host[GUARD:-GUARD].reshape(B, 256, H, W)
    assert (xs[:, :128] == FILL).all(), "x[:, :128] was written"
    d = mismatch(xs[:, 128:].view(np.float32), plain)
    assert d is None, d


def raw_encoder(flow, c1, mod, out_ptr, stride, ws_ptr, packed=None):
    """ecorr_motion_encoder through ctypes on device tensors, with its own pack of mod's weights unless one is
    given.  Returns the packed buffer."""
    import eraft_amd
    from eraft_amd import _lib
    L = eraft_amd.lib()
    B, _, H, W = c1.shape
    st = _lib.stream_of(c1)
    if packed is None:
        n = ctypes.c_int64()
        assert L.ecorr_motion_encoder_packed_size(ctypes.byref(n)) == 0
        packed = torch.empty(n.value, dtype=torch.uint8, device=c1.device)
        names = ("convc2", "convf1", "convf2", "conv")
        ws = [getattr(mod, k).weight.detach().contiguous() for k in names]
        bs = [getattr(mod, k).bias.detach().contiguous() for k in names]
        wp = (ctypes.c_void_p * 4)(*[t.data_ptr() for t in ws])
        bp = (ctypes.c_void_p * 4)(*[t.data_ptr() for t in bs])
        assert L.ecorr_motion_encoder_pack(wp, bp, packed.data_ptr(), st) == 0
        torch.cuda.synchronize()
    assert L.ecorr_motion_encoder(c1.data_ptr(), flow.data_ptr(), B, H, W, packed.data_ptr(), out_ptr, stride, ws_ptr,
                                  st) == 0
    torch.cuda.synchronize()
    return packed


@pytest.mark.parametrize("shape", [(3, 9, 15), (1, 1, 1)], ids=lambda s: "x".join(map(str, s)))
def test_guards_and_raw_abi(shape):
    """Through ctypes: out with a batch stride of 128 H W + 96 floats between guard bands, a workspace of exactly the
    reported size between guards, prefilled with 0xff bytes (a read before a write is a NaN) and then with 0x00:
    every output element is written, the gaps between the items and the guards keep their fill, and the bits are
    those of motion_encoder either way."""
    import eraft_amd
    B, H, W = shape
    flow, c1, ref = case(shape)
    mod = gpu_module()
    fd, cd = flow.cuda(), c1.cuda()
    item, S = OUT * H * W, OUT * H * W + 96
    nbytes = ctypes.c_int64()
    assert eraft_amd.lib().ecorr_motion_encoder_workspace_size(B, H, W, ctypes.byref(nbytes)) == 0
    assert nbytes.value == 384 * B * H * W * 4
    want = run(flow, c1)
    packed = None
    for fill in (0xff, 0x00):
        buf, out = guarded((B - 1) * S + item)
        ws = Workspace(nbytes.value, fill)
        packed = raw_encoder(fd, cd, mod, out.data_ptr(), S, ws.ptr, packed)
        ws.check("motion_encoder workspace")
        host = buf.cpu().numpy()
        assert (host[:GUARD] == FILL).all() and (host[-GUARD:] == FILL).all(), "a guard band was written"
        mid = host[GUARD:-GUARD]
        got = np.stack([mid[b * S:b * S + item] for b in range(B)])
        assert not (got == FILL).any(), f"{int((got == FILL).sum())} output elements were never written"
        for b in range(B - 1):
            assert (mid[b * S + item:(b + 1) * S] == FILL).all(), f"the gap behind item {b} was written"
        got = got.view(np.float32).reshape(B, OUT, H, W)
        assert np.isfinite(got).all()
        d = mismatch(got, want)
        assert d is None, f"raw ABI (workspace of {fill:#x}) against motion_encoder: {d}"
    assert normwise(want[:, :CONV], ref[:, :CONV]) <= BAR


def _corner(shape, corner):
    _, H, W = shape
    return ((0, H - 1)[corner >> 1], (0, W - 1)[corner & 1])


def _far(shape, y0, x0, reach):
    """[H, W] mask of the pixels farther than `reach` (Chebyshev) from (y0, x0)."""
    _, H, W = shape
    yy, xx = np.mgrid[0:H, 0:W]
    return np.maximum(np.abs(yy - y0), np.abs(xx - x0)) > reach


@pytest.mark.parametrize("corner", range(4), ids=["top-left", "top-right", "bottom-left", "bottom-right"])
@pytest.mark.parametrize("shape", [(2, 9, 15), (1, 3, 70)], ids=lambda s: "x".join(map(str, s)))
def test_border_isolation(shape, corner):
    """c1 nonzero only at one corner pixel (flow zero): two 3x3 convolutions reach 2 pixels, so every output farther
    than that is the all-zero input's, bit for bit; flow nonzero only there (c1 zero): 7x7 then two 3x3 reach 5.
    A row wrap (the flattened neighbour of a row end is the next row's start) or a channel wrap (p - W of row 0 is
    the previous channel's last row) would carry the corner into pixels far from it."""
    B, H, W = shape
    flow, c1 = make_inputs(61 + corner, B, H, W)
    y0, x0 = _corner(shape, corner)
    keep = torch.zeros(H, W, dtype=torch.bool)
    keep[y0, x0] = True
    c1 = c1 + 0.5   # relu(normal) is 0 for half the channels: every channel of the corner pixel nonzero
    zf, zc = torch.zeros_like(flow), torch.zeros_like(c1)
    zero = run(zf, zc)
    # (where, not a product: -x * 0 is -0.0, which the flow channels would copy bit for bit)
    for name, f, c, reach in (("c1", zf, torch.where(keep, c1, zc), 2), ("flow", torch.where(keep, flow, zf), zc, 5)):
        got = run(f, c)
        far = _far(shape, y0, x0, reach)
        if far.any():
            d = mismatch(got[:, :, far], zero[:, :, far])
            assert d is None, f"{name} at {(y0, x0)}: {d}"
        assert (got[:, :CONV, y0, x0] != zero[:, :CONV, y0, x0]).any()
        near = ~_far(shape, y0, x0, reach)
        moved = (got != zero).any(axis=(0, 1))
        assert not (moved & ~near).any()


def _nan_case(what, at):
    B, H, W = 2, 13, 14
    flow, c1 = make_inputs(53, B, H, W)
    y0, x0 = (6, 7) if at == "interior" else (0, W - 1)
    if what == "c1":
        c1 = c1.clone()
        c1[0, 17, y0, x0] = float("nan")
    else:
        flow = flow.clone()
        flow[0, 1, y0, x0] = float("nan")
    return flow, c1, (y0, x0)


@pytest.mark.parametrize("at", ["interior", "corner"])
@pytest.mark.parametrize("what", ["c1", "flow"])
def test_nan_stays_on_its_footprint(what, at):
    """One NaN in item 0's c1 (flow): isnan of the result is isnan of the fp32 CPU module's output, exactly -- the
    5 x 5 (11 x 11) block around the pixel clipped to the image on channels 0-125, plus flow's own element, and
    nothing in item 1; never a whole tile.  Outside it the NaN-free run's bits."""
    flow, c1, (y0, x0) = _nan_case(what, at)
    got = run(flow, c1)
    with torch.no_grad():
        ref_nan = np.isnan(cpu_module()(flow, c1, corr_is_convc1=True).numpy())
    reach = 2 if what == "c1" else 5
    block = ~_far((2, 13, 14), y0, x0, reach)
    want = np.zeros_like(ref_nan)
    want[0, :CONV] = block[None]
    if what == "flow":
        want[0, CONV + 1, y0, x0] = True
    assert (ref_nan == want).all()   # the reference's own footprint
    assert not block.all()
    assert (np.isnan(got) == ref_nan).all(), f"{int((np.isnan(got) != ref_nan).sum())} elements differ in NaN-ness"
    clean = run(*make_inputs(53, 2, 13, 14))
    d = mismatch(np.where(ref_nan, 0, got), np.where(ref_nan, 0, clean))
    assert d is None, f"outside the footprint: {d}"


def test_weight_cache_follows_in_place_update():
    flow, c1, _ = case((1, 15, 20))
    cpu = copy.deepcopy(cpu_module())
    mod = copy.deepcopy(cpu).cuda()
    before = run(flow, c1, mod)
    with torch.no_grad():
        cpu.convf2.weight.mul_(2)
        mod.convf2.weight.mul_(2)
        ref = copy.deepcopy(cpu).double()(flow.double(), c1.double(), corr_is_convc1=True).numpy()
    after = run(flow, c1, mod)
    err = normwise(after[:, :CONV], ref[:, :CONV])
    print(f"after convf2.weight.mul_(2): max|err|/rms(ref) = {err:.3g}")
    assert err <= BAR
    assert (after != before).any()


def test_python_refusals():
    import eraft_amd
    flow, c1, _ = case((2, 3, 5))
    fd, cd = flow.cuda(), c1.cuda()
    mod = gpu_module()
    live = copy.deepcopy(mod).requires_grad_(True)
    with pytest.raises(RuntimeError, match="forward-only"):   # the weights require grad, grad mode is on
        eraft_amd.motion_encoder(fd, cd, live)
    assert eraft_amd.motion_encoder(fd, cd, mod).shape == (2, OUT, 3, 5)   # nothing requires grad: allowed
    with pytest.raises(RuntimeError, match="forward-only"):
        eraft_amd.motion_encoder(fd.clone().requires_grad_(True), cd, mod)
    with pytest.raises(RuntimeError, match="forward-only"):
        eraft_amd.motion_encoder(fd, cd.clone().requires_grad_(True), mod)
    with torch.no_grad():
        with pytest.raises(TypeError):
            eraft_amd.motion_encoder(fd.half(), cd, mod)
        with pytest.raises(RuntimeError, match="HIP devices"):
            eraft_amd.motion_encoder(flow, cd, mod)
        with pytest.raises(RuntimeError):
            eraft_amd.motion_encoder(fd, cd[:, :128].contiguous(), mod)
        with pytest.raises(RuntimeError):
            eraft_amd.motion_encoder(fd, cd[:, :, :, :4], mod)
        B, H, W = 2, 3, 5
        x = torch.empty(B, 256, H, W, device="cuda")
        for bad in (torch.empty(B, OUT, W, H, device="cuda").transpose(2, 3),            # H and W swapped in memory
                    torch.empty(B, H, W, OUT, device="cuda").permute(0, 3, 1, 2),        # channels last
                    torch.empty(B, 2 * OUT, H, W, device="cuda")[:, ::2],                # every other channel
                    torch.empty(B, OUT, H, 2 * W, device="cuda")[..., ::2],              # every other column
                    torch.empty(OUT, B, H, W, device="cuda").transpose(0, 1),            # batch stride < 128 H W
                    torch.empty(1, OUT, H, W, device="cuda").expand(B, OUT, H, W)):      # batch stride 0
            assert tuple(bad.shape) == (B, OUT, H, W)
            with pytest.raises(ValueError, match="strides"):
                eraft_amd.motion_encoder(fd, cd, mod, out=bad)
        with pytest.raises(ValueError):
            eraft_amd.motion_encoder(fd, cd, mod, out=x[:, 100:])   # 156 channels
        with pytest.raises(TypeError):
            eraft_amd.motion_encoder(fd, cd, mod, out=x[:, 128:].half())
        both = torch.empty(B, 256 + 128, H, W, device="cuda")   # out overlapping c1: refused by the library
        cin = both[:, :256]
        with pytest.raises(RuntimeError):   # (a c1 that is a view: not contiguous)
            eraft_amd.motion_encoder(fd, cin, mod, out=both[:, 256:])
        flat = torch.empty(B * 256 * H * W + 64, device="cuda")
        c_in = flat[:B * 256 * H * W].view(B, 256, H, W)
        with pytest.raises(ValueError):
            eraft_amd.motion_encoder(fd, c_in, mod, out=flat[64:64 + B * OUT * H * W].view(B, OUT, H, W))
        assert eraft_amd.motion_encoder(fd, cd, mod, out=x[:, 128:]).data_ptr() == x[:, 128:].data_ptr()


@pytest.mark.filterwarnings("ignore:The CUDA Graph is empty")   # the refused capture recorded nothing
def test_pack_under_capture_is_refused():
    import eraft_amd
    flow, c1, _ = case((2, 3, 5))
    mod = copy.deepcopy(gpu_module())   # not packed yet
    fd, cd = flow.cuda(), c1.cuda()
    torch.cuda.synchronize()
    g = torch.cuda.CUDAGraph()
    with pytest.raises(RuntimeError, match="outside the captured region"):
        with torch.no_grad(), torch.cuda.graph(g):
            eraft_amd.motion_encoder(fd, cd, mod)
    with torch.no_grad():   # the refusal left nothing behind: an eager call packs and runs
        out = eraft_amd.motion_encoder(fd, cd, mod)
    d = mismatch(out.cpu().numpy(), run(flow, c1))
    assert d is None, d


def test_graph_capture():
    import eraft_amd
    B, H, W = 3, 9, 15
    sets = [make_inputs(200 + 10 * i, B, H, W) for i in range(2)]
    sets = [(a.cuda(), b.cuda()) for a, b in sets]
    flow, c1 = sets[0][0].clone(), sets[0][1].clone()
    x = torch.zeros(B, 256, H, W, device="cuda")
    mod = gpu_module()
    outs = []

    def step():
        with torch.no_grad():
            outs[:] = [eraft_amd.motion_encoder(flow, c1, mod), eraft_amd.motion_encoder(flow, c1, mod, out=x[:, 128:])]

    def mutate(i):
        flow.copy_(sets[i][0])
        c1.copy_(sets[i][1])

    replay_matches_eager(step, mutate, outs)
