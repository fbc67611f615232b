"""eraft_amd.sepconv_gru / ecorr_sepconv_gru (csrc/gru.hip) against an fp64 SepConvGRU on the CPU.

Reference: network.SepConvGRU(128, 256).double() on the CPU, fed the same fp32 inputs (the e2e goldens pin
that module to the reference's update.py:33-60).  Inputs from tests/prng.py: h = tanh(normal), x = 254
channels of relu(normal) and two flow-like channels of 3 * normal; weights and biases at PyTorch's default
scales as tests/e2e_weights.py draws them, and the same weights * 8 (saturated gates).

Accuracy bar: max |got - ref| / rms(ref) <= 1e-5 on h', the project's normwise bar for every GEMM (the fp32
ATen GRU itself gives 5.3e-7 .. 7.5e-7 at these shapes, 1.6e-6 .. 2.7e-6 with the weights * 8).
Shapes: ragged 64-pixel tiles crossing row ends with a batch offset, W = the tap count, H = 1, W = 1, both
axes shorter than the taps, a pyramid-sized map with W < 64, and a DSEC row length.
"""
import copy
import ctypes
import functools

import numpy as np
import pytest
import torch

import prng
from e2e_weights import make_state_dict
from gpu_guard import Workspace, check_guarded, guarded, mismatch
from graph_capture import replay_matches_eager

pytestmark = pytest.mark.gpu

HID, INP = 128, 256
BAR = 1e-5
SHAPES = [(2, 7, 70), (1, 3, 5), (1, 1, 130), (1, 130, 1), (1, 2, 2), (1, 15, 20), (1, 9, 80)]
SCALES = [1, 8]


@pytest.fixture(autouse=True)
def _device():
    if not torch.cuda.is_available():
        pytest.fail("no HIP device visible")


def make_inputs(seed, B, H, W):
    h = np.tanh(prng.normal(seed, (B, HID, H, W)).astype(np.float64)).astype(np.float32)
    x = np.maximum(prng.normal(seed + 1, (B, INP, H, W)), 0).astype(np.float32)
    x[:, -2:] = prng.normal(seed + 2, (B, 2, H, W), 3.0)
    return torch.from_numpy(h), torch.from_numpy(np.ascontiguousarray(x))


@functools.lru_cache(maxsize=None)
def cpu_module(scale):
    """The fp32 module on the CPU with the PRNG weights (times `scale`)."""
    from eraft_amd import network
    mod = network.SepConvGRU(HID, INP)
    mod.load_state_dict(make_state_dict(mod.state_dict()))
    with torch.no_grad():
        for p in mod.parameters():
            p.mul_(scale)
    return mod.eval()


@functools.lru_cache(maxsize=None)
def gpu_module(scale):
    return copy.deepcopy(cpu_module(scale)).cuda()


def reference(mod, h, x):
    """fp64 on the CPU from the fp32 inputs and fp32 weights -> numpy float64."""
    with torch.no_grad():
        return copy.deepcopy(mod).double()(h.double(), x.double()).numpy()


@functools.lru_cache(maxsize=None)
def case(shape, scale):
    """(h, x) on the CPU and the fp64 reference, computed once per case and never changed."""
    B, H, W = shape
    h, x = make_inputs(100 + 7 * H + W, B, H, W)
    return h, x, reference(cpu_module(scale), h, x)


def normwise(got, ref):
    d = np.abs(np.asarray(got, np.float64) - ref).max()
    return float(d / np.sqrt(np.mean(ref * ref)))


def run(h, x, mod):
    import eraft_amd
    with torch.no_grad():
        out = eraft_amd.sepconv_gru(h.cuda(), x.cuda(), mod)
    torch.cuda.synchronize()
    return out.cpu().numpy()


def raw_gru(h, x, mod, out, ws_ptr, packed=None):
    """ecorr_sepconv_gru through ctypes on device tensors h, x -> out (a device float tensor view), with its own
    pack of mod's weights unless one is given.  Returns the packed buffer."""
    import eraft_amd
    from eraft_amd import _lib
    L = eraft_amd.lib()
    B, _, H, W = h.shape
    st = _lib.stream_of(h)
    if packed is None:
        n = ctypes.c_int64()
        assert L.ecorr_sepconv_gru_packed_size(HID, INP, ctypes.byref(n)) == 0
        packed = torch.empty(n.value, dtype=torch.uint8, device=h.device)
        names = ("convz1", "convr1", "convq1", "convz2", "convr2", "convq2")
        ws = [getattr(mod, k).weight.detach().contiguous() for k in names]
        bs = [getattr(mod, k).bias.detach().contiguous() for k in names]
        wp = (ctypes.c_void_p * 6)(*[t.data_ptr() for t in ws])
        bp = (ctypes.c_void_p * 6)(*[t.data_ptr() for t in bs])
        assert L.ecorr_sepconv_gru_pack(wp, bp, HID, INP, packed.data_ptr(), st) == 0
        torch.cuda.synchronize()
    assert L.ecorr_sepconv_gru(h.data_ptr(), x.data_ptr(), B, HID, INP, H, W, packed.data_ptr(), out.data_ptr(),
                               ws_ptr, st) == 0
    torch.cuda.synchronize()
    return packed


def workspace_bytes(B, H, W):
    import eraft_amd
    n = ctypes.c_int64()
    assert eraft_amd.lib().ecorr_sepconv_gru_workspace_size(B, HID, INP, H, W, ctypes.byref(n)) == 0
    return n.value


@pytest.mark.parametrize("scale", SCALES, ids=lambda s: f"w{s}")
@pytest.mark.parametrize("shape", SHAPES, ids=lambda s: "x".join(map(str, s)))
def test_accuracy(shape, scale):
    h, x, ref = case(shape, scale)
    got = run(h, x, gpu_module(scale))
    err = normwise(got, ref)
    print(f"sepconv_gru {shape} weights*{scale}: max|err|/rms(ref) = {err:.3g} (rms {np.sqrt(np.mean(ref * ref)):.3g})")
    assert np.isfinite(got).all()
    assert err <= BAR


@pytest.mark.parametrize("side", ["last", "first"])
@pytest.mark.parametrize("shape", [(2, 5, 9), (1, 3, 70)], ids=lambda s: "x".join(map(str, s)))
def test_border_isolation_columns(shape, side):
    """h and x nonzero only in one border column of every row: the 1x5 half-step reads no further than two
    columns and the 5x1 half-step stays in its column, so the outputs more than two columns from it are
    those of an all-zero input, bit for bit -- for the last column W - 1 these are columns 0 .. W - 4 (column
    W - 3 reads column W - 1 through its +2 tap, in the reference as well: asserted below on the CPU module).
    A row wrap (the flattened neighbour of a row end is the next row's start) would leak the column into the
    first (last) two columns of the neighbouring row."""
    B, H, W = shape
    h, x = make_inputs(31, B, H, W)
    col = W - 1 if side == "last" else 0
    keep = torch.zeros(W, dtype=torch.bool)
    keep[col] = True
    h, x = h * keep, x * keep
    assert float(h[..., col].abs().min()) > 0   # every row's border element is nonzero (tanh of a nonzero draw)
    mod = gpu_module(1)
    got = run(h, x, mod)
    zero = run(torch.zeros_like(h), torch.zeros_like(x), mod)
    far = slice(0, W - 3) if side == "last" else slice(3, W)
    d = mismatch(got[..., far], zero[..., far])
    assert d is None, d
    assert (got[..., col] != zero[..., col]).any()
    with torch.no_grad():   # the reference reaches exactly two columns: the third from the border is the first unchanged
        cpu = cpu_module(1)
        moved = (cpu(h, x) != cpu(torch.zeros_like(h), torch.zeros_like(x))).numpy().any(axis=(0, 1, 2))
    near = np.zeros(W, dtype=bool)
    near[W - 3:] = True
    assert (moved == (near if side == "last" else near[::-1])).all()


@pytest.mark.parametrize("side", ["last", "first"])
@pytest.mark.parametrize("shape", [(2, 6, 9), (1, 70, 3)], ids=lambda s: "x".join(map(str, s)))
def test_border_isolation_rows(shape, side):
    """The mirror case for rows and channels: h and x nonzero only in the last (first) row of every channel.
    The 5x1 half-step reaches four rows, not two: r moves within two rows of the border, r * h1 with it (h1 is
    nonzero everywhere: the first half-step's biases), and q reads r * h1 two rows further -- in the reference
    as well, asserted below on the CPU module.  So the rows more than four away are those of an all-zero
    input, bit for bit (last row: rows 0 .. H - 6, row 0 among them).  A channel wrap (p - W on row 0 of
    channel c + 1 is the last row of channel c, p + W on the last row of channel c the first row of channel
    c + 1, both inside the buffer range) would leak into rows 0 and 1 (the last two rows) of every channel,
    and from one batch item's rows into the next item's."""
    B, H, W = shape
    h, x = make_inputs(37, B, H, W)
    row = H - 1 if side == "last" else 0
    keep = torch.zeros(H, 1, dtype=torch.bool)
    keep[row] = True
    h, x = h * keep, x * keep
    mod = gpu_module(1)
    got = run(h, x, mod)
    zero = run(torch.zeros_like(h), torch.zeros_like(x), mod)
    far = slice(0, H - 5) if side == "last" else slice(5, H)
    d = mismatch(got[:, :, far], zero[:, :, far])
    assert d is None, d
    assert (got[:, :, row] != zero[:, :, row]).any()
    with torch.no_grad():
        cpu = cpu_module(1)
        moved = (cpu(h, x) != cpu(torch.zeros_like(h), torch.zeros_like(x))).numpy().any(axis=(0, 1, 3))
    near = np.zeros(H, dtype=bool)
    near[H - 5:] = True
    assert (moved == (near if side == "last" else near[::-1])).all()


@pytest.mark.parametrize("shape", [(2, 7, 70), (1, 2, 2)], ids=lambda s: "x".join(map(str, s)))
def test_guards_and_raw_abi(shape):
    """h_out between guard bands and a workspace of exactly the reported size between guards, everything
    prefilled (the workspace with 0xff bytes: a read before a write is a NaN): the guards stay, every output
    element is written, and the bits are those of the unguarded call and of sepconv_gru."""
    B, H, W = shape
    h, x, ref = case(shape, 1)
    mod = gpu_module(1)
    hd, xd = h.cuda(), x.cuda()
    n = B * HID * H * W
    buf, out = guarded(n)
    ws = Workspace(workspace_bytes(B, H, W), 0xff)
    packed = raw_gru(hd, xd, mod, out, ws.ptr)
    ws.check("sepconv_gru workspace")
    got = check_guarded(buf, "sepconv_gru h_out").reshape(B, HID, H, W)
    assert np.isfinite(got).all()
    plain = torch.empty(n, dtype=torch.float32, device="cuda")
    ws2 = torch.zeros(workspace_bytes(B, H, W), dtype=torch.uint8, device="cuda")
    raw_gru(hd, xd, mod, plain, ws2.data_ptr(), packed)
    d = mismatch(got, plain.cpu().numpy().reshape(B, HID, H, W))
    assert d is None, f"guarded against unguarded: {d}"
    d = mismatch(got, run(h, x, mod))
    assert d is None, f"raw ABI against sepconv_gru: {d}"
    assert normwise(got, ref) <= BAR


def test_two_calls_same_bits():
    h, x, _ = case((2, 7, 70), 1)
    mod = gpu_module(1)
    d = mismatch(run(h, x, mod), run(h, x, mod))
    assert d is None, d


def test_nan_stays_on_its_footprint():
    """One NaN in item 0's x at an interior pixel: item 1 is the NaN-free run bit for bit; item 0 is NaN on
    the reference's set, all 128 channels: the 5 x 5 block around the pixel and, because r * h carries a NaN
    two taps further in each half-step, the whole 9 x 9 block (the fp32 CPU module's own NaN set, asserted) --
    and, with no shared exponent in the kernels, nowhere else (include/ecorr.h): the other elements keep the
    NaN-free run's bits."""
    B, H, W = 2, 12, 14
    h, x = make_inputs(53, B, H, W)
    mod = gpu_module(1)
    clean = run(h, x, mod)
    xn = x.clone()
    y0, x0 = 5, 6
    xn[0, 17, y0, x0] = float("nan")
    got = run(h, xn, mod)
    d = mismatch(got[1:], clean[1:])
    assert d is None, f"item 1: {d}"
    block = np.zeros((H, W), dtype=bool)
    block[y0 - 4:y0 + 5, x0 - 4:x0 + 5] = True
    with torch.no_grad():
        ref_nan = np.isnan(cpu_module(1)(h, xn).numpy())
    assert (ref_nan[0] == block[None]).all() and not ref_nan[1].any()   # the reference's own footprint
    assert block[y0 - 2:y0 + 3, x0 - 2:x0 + 3].all() and not block.all()
    assert np.isnan(got[0][:, block]).all()
    assert not np.isnan(got[0][:, ~block]).any()
    d = mismatch(got[0][None][:, :, ~block], clean[0][None][:, :, ~block])
    assert d is None, f"item 0 outside the block: {d}"


def test_weight_cache_follows_in_place_update():
    h, x, _ = case((1, 15, 20), 1)
    cpu = copy.deepcopy(cpu_module(1))
    mod = copy.deepcopy(cpu).cuda()
    before = run(h, x, mod)
    with torch.no_grad():
        cpu.convq1.weight.mul_(2)
        mod.convq1.weight.mul_(2)
    after = run(h, x, mod)
    err = normwise(after, reference(cpu, h, x))
    print(f"after convq1.weight.mul_(2): max|err|/rms(ref) = {err:.3g}")
    assert err <= BAR
    assert (after != before).any()
    with torch.no_grad():   # load_state_dict writes in place as well
        mod.load_state_dict(cpu_module(1).state_dict())
    d = mismatch(run(h, x, mod), before)
    assert d is None, d


def test_python_refusals():
    import eraft_amd
    h, x, _ = case((1, 2, 2), 1)
    mod = gpu_module(1)
    hd, xd = h.cuda(), x.cuda()
    with pytest.raises(RuntimeError, match="forward-only"):   # the weights require grad, grad mode is on
        eraft_amd.sepconv_gru(hd, xd, mod)
    frozen = copy.deepcopy(mod).requires_grad_(False)
    assert eraft_amd.sepconv_gru(hd, xd, frozen).shape == hd.shape   # nothing requires grad: allowed
    with pytest.raises(RuntimeError, match="forward-only"):
        eraft_amd.sepconv_gru(hd.clone().requires_grad_(True), xd, frozen)
    with torch.no_grad():
        with pytest.raises(TypeError):
            eraft_amd.sepconv_gru(hd.half(), xd, mod)
        with pytest.raises(RuntimeError, match="HIP devices"):
            eraft_amd.sepconv_gru(h, xd, mod)
        with pytest.raises(RuntimeError):
            eraft_amd.sepconv_gru(hd, xd[:, :, :1], mod)
        with pytest.raises(RuntimeError):
            eraft_amd.sepconv_gru(hd, xd.transpose(2, 3), mod)   # the same shape (H = W), non-contiguous
        fresh = copy.deepcopy(mod)   # never packed: the sizes are checked before the cache and the weights
        with pytest.raises(ValueError):   # an unsupported (hidden, input)
            eraft_amd.sepconv_gru(hd[:, :64].contiguous(), xd, fresh)
        with pytest.raises(ValueError):   # ... and the same from a module whose pack is cached
            eraft_amd.sepconv_gru(hd, xd, mod)
            eraft_amd.sepconv_gru(hd[:, :64].contiguous(), xd, mod)
        with pytest.raises(ValueError):
            eraft_amd.sepconv_gru(hd, xd[:, :128].contiguous(), fresh)
    with pytest.raises(RuntimeError, match="sepconv_gru"):   # the message names the op, not the CorrBlock
        eraft_amd.sepconv_gru(hd, xd, mod)


def test_cached_pack_on_a_second_stream():
    """The pack is enqueued on the first call's stream and cached on the module: a later call on another stream
    is ordered after it by the pack's event, and gives the same bits."""
    import eraft_amd
    h, x, _ = case((1, 15, 20), 1)
    mod = copy.deepcopy(gpu_module(1))   # not packed yet
    hd, xd = h.cuda(), x.cuda()
    side = torch.cuda.Stream()
    torch.cuda.synchronize()
    with torch.no_grad():
        first = eraft_amd.sepconv_gru(hd, xd, mod)        # packs on the current stream
        with torch.cuda.stream(side):
            second = eraft_amd.sepconv_gru(hd, xd, mod)   # no host sync in between
    torch.cuda.synchronize()
    d = mismatch(second.cpu().numpy(), first.cpu().numpy())
    assert d is None, d
    d = mismatch(first.cpu().numpy(), run(h, x, gpu_module(1)))
    assert d is None, d


@pytest.mark.filterwarnings("ignore:The CUDA Graph is empty")   # the refused capture recorded nothing
def test_pack_under_capture_is_refused():
    """A module that is not packed yet raises inside a captured region, before any launch: the pack would live
    in the graph's private pool and be handed to later eager calls."""
    import eraft_amd
    h, x, _ = case((1, 2, 2), 1)
    mod = copy.deepcopy(gpu_module(1))
    hd, xd = h.cuda(), x.cuda()
    torch.cuda.synchronize()
    g = torch.cuda.CUDAGraph()
    with pytest.raises(RuntimeError, match="outside the captured region"):
        with torch.no_grad(), torch.cuda.graph(g):
            eraft_amd.sepconv_gru(hd, xd, mod)
    with torch.no_grad():   # the refusal left nothing behind: an eager call packs and runs
        out = eraft_amd.sepconv_gru(hd, xd, mod)
    d = mismatch(out.cpu().numpy(), run(h, x, gpu_module(1)))
    assert d is None, d


def test_graph_capture():
    import eraft_amd
    B, H, W = 2, 7, 70
    sets = [make_inputs(200 + 10 * i, B, H, W) for i in range(2)]
    sets = [(a.cuda(), b.cuda()) for a, b in sets]
    h, x = sets[0][0].clone(), sets[0][1].clone()
    mod = gpu_module(1)
    outs = []

    def step():
        with torch.no_grad():
            outs[:] = [eraft_amd.sepconv_gru(h, x, mod)]

    def mutate(i):
        h.copy_(sets[i][0])
        x.copy_(sets[i][1])

    replay_matches_eager(step, mutate, outs)
