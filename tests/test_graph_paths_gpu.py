"""Every stream-ordered entry point under a graph capture, and on a second stream.

Each case is a `step` of one path with its static inputs and three input sets from tests/prng.py; the
blocks are created inside the step, so the weight pack, the presplit column scale and every temporary
the Python layer allocates are part of the graph.  graph_capture.replay_matches_eager captures the
step and replays it on the sets in turn, against the step run eagerly on the same inputs, bit for bit
(its docstring says what each assertion is for).  The shapes are the smallest of the project's own case
tables that reach the branch named.  No tolerance anywhere: the eager values are pinned to references
by the tests of each kernel family.

The three backward steps (grad.hip, conv_grad.hip, the upsample backward) are not captured: see
NOT_CAPTURED below.  They run in the second-stream test only.

test_second_stream_is_the_default_stream runs every non-ERAFT step eagerly under
`with torch.cuda.stream(s)`, inputs made on s: the same bits as on the default stream.  It cannot prove
ordering; it pins that no wrapper touches another stream than the current one in a way that changes
results.

The two entry points that read an error flag on the host (flow_16bit_to_float,
EventSequenceToVoxelGrid_Pytorch.__call__) raise under a capture, naming themselves.
"""
import numpy as np
import pytest
import torch

import alt_corr_cases as ac
import prng
from e2e_weights import make_state_dict
from graph_capture import first_difference, replay_matches_eager, snapshot

pytestmark = pytest.mark.gpu

DEV = torch.device("cuda", 0)
F16, BF16 = torch.float16, torch.bfloat16
NSETS = 3


@pytest.fixture(scope="module")
def ea():
    if not torch.cuda.is_available():
        pytest.fail("no HIP device visible: GPU tests must run on the MI355X box")
    import eraft_amd
    eraft_amd.lib()
    return eraft_amd


def _t(a, dtype=None):
    t = torch.from_numpy(np.ascontiguousarray(a))
    return t if dtype is None else t.to(dtype)


class Case:
    """One step with its static inputs.  gen(i) -> the CPU tensors of input set i; run(*inputs) -> the
    output tensors; grad: the indices of the inputs that are leaves requiring grad.  Everything is made
    on the stream that is current when the case is built."""

    def __init__(self, gen, run, grad=()):
        self.sets = [[t.to(DEV) for t in gen(i)] for i in range(NSETS)]
        self.inputs = [t.clone() for t in self.sets[0]]
        for k in grad:
            self.inputs[k].requires_grad_(True)
        self.outs = []
        self._run = run

    def step(self):
        self.outs[:] = self._run(*self.inputs)

    def mutate(self, i):
        with torch.no_grad():
            for t, v in zip(self.inputs, self.sets[i]):
                t.copy_(v)


# ---- lookup_conv1x1_relu: 17 x 20 (Q = 340, not PAIR) and 16 x 24 (PAIR), B 2, D 32, L 4, r 4, O 128
def _convc1_inputs(seed, shapes, dt=None):
    def gen(i):
        s = seed + 100 * i
        ts = [_t(prng.normal(s, (128, 324, 1, 1), 0.1)), _t(prng.normal(s + 1, (128,), 0.5))]
        for k, (H, W) in enumerate(shapes):
            q = s + 10 * (k + 1)
            c0 = prng.coords_with_flow(q + 2, 2, H, W, 2.0)
            c0[:, :, H // 2, W // 2] = np.nan                  # one NaN query per batch item
            ts += [_t(prng.normal(q, (2, 32, H, W))), _t(prng.normal(q + 1, (2, 32, H, W))),
                   _t(c0), _t(prng.coords_with_flow(q + 3, 2, H, W, 9.0))]
        return ts
    return gen


def _convc1(ea, modes, shapes=((17, 20), (16, 24)), dts=(None,), seed=21000):
    def run(w, b, *rest):
        outs = []
        for k in range(len(shapes)):
            f1, f2, c0, c1 = rest[4 * k:4 * k + 4]
            blk = ea.CorrBlock(f1, f2, num_levels=4, radius=4)
            for m in modes:
                for dt in dts:
                    outs += [blk.lookup_conv1x1_relu(c, w, b, mode=m, out_dtype=dt) for c in (c0, c1)]
        return outs
    return Case(_convc1_inputs(seed, shapes), run)


# ---- the 16-bit lookup on 16-bit fmaps, and another radius
def _lookup_half(ea, dt):
    B, D, H, W = 2, 32, 17, 20

    def gen(i):
        s = 22000 + 100 * i
        return [_t(prng.normal(s, (B, D, H, W)), dt), _t(prng.normal(s + 1, (B, D, H, W)), dt),
                _t(prng.coords_with_flow(s + 2, B, H, W, 3.0))]

    def run(h1, h2, c):
        blk = ea.CorrBlock(h1, h2, num_levels=4, radius=4, fmap_dtype=dt)
        return [blk(c, out_dtype=dt), blk(c)]
    return Case(gen, run)


def _lookup_other_radius(ea):
    B, D, H, W = 1, 16, 12, 16

    def gen(i):
        s = 23000 + 100 * i
        return [_t(prng.normal(s, (B, D, H, W))), _t(prng.normal(s + 1, (B, D, H, W))),
                _t(prng.coords_with_flow(s + 2, B, H, W, 2.0)), _t(prng.coords_with_flow(s + 3, B, H, W, 6.0))]

    def run(f1, f2, c0, c1):
        blk = ea.CorrBlock(f1, f2, num_levels=3, radius=2)
        return [blk(c0), blk(c1)]
    return Case(gen, run)


# ---- AlternateCorrBlock: the window kernel (r 4) and the generic kernel (r 5)
ALT_COORDS = [("smooth", "iid_large"), ("special", "edge"), ("half", "up")]   # set 1: NaN, inf and huge coordinates


def _alt(ea, name):
    r, B, D, H, W, L = ac.CASES[name]
    cs = ac.coord_sets(name)

    def gen(i):
        s = ac.seed_of(name) + 1000 * (i + 1)
        a, b = (cs[k].copy() for k in ALT_COORDS[i])
        if i == 1:
            b[B - 1, 0, H // 2, W // 2] = np.nan               # a NaN coordinate: the in-kernel generic sample
        return [_t(prng.normal(s, (B, D, H, W))), _t(prng.normal(s + 1, (B, D, H, W))), _t(a), _t(b)]

    def run(f1, f2, c0, c1):
        blk = ea.AlternateCorrBlock(f1, f2, num_levels=L, radius=r)
        return [blk(c0), blk(c1, out_dtype=F16)]
    return Case(gen, run)


# ---- the DSEC voxel grid: 5,000 events every round, set 1 with every event on one pixel
def _voxel(ea, normalize):
    C, H, W, n = 5, 48, 64, 5000

    def gen(i):
        p, t, x, y = prng.dsec_events(24000 + 100 * i, n, H, W)
        if i == 1:
            x[:] = 3.25
            y[:] = 4.75
        return [_t(v) for v in (p, t, x, y)]

    def run(p, t, x, y):
        return [ea.VoxelGrid((C, H, W), normalize).convert({"p": p, "t": t, "x": x, "y": y})]
    return Case(gen, run)


# ---- coords_grid, bilinear_sampler, flow_to_png16
def _sampler_grid_png(ea):
    N, C, H, W = 2, 8, 12, 20

    def gen(i):
        s = 25000 + 100 * i
        return [_t(prng.normal(s, (N, C, H, W))), _t(prng.normal(s + 1, (N, 2, H, W), 3.0)),
                _t(prng.normal(s + 2, (2, 2, 24, 32), 20.0))]

    def run(img, delta, flow):
        grid = ea.coords_grid(N, H, W, device=DEV)
        out, m = ea.bilinear_sampler(img, (grid + delta).permute(0, 2, 3, 1), mask=True)
        return [grid, out, m, ea.flow_to_png16(flow)]
    return Case(gen, run)


# ---- the backward families: autograd's worker thread takes its stream from the forward's
def _corr_backward(ea):
    B, D, H, W, L, R, O = 1, 32, 16, 24, 4, 4, 128
    C = L * (2 * R + 1) ** 2

    def gen(i):
        s = 26000 + 100 * i
        return [_t(prng.normal(s, (B, D, H, W))), _t(prng.normal(s + 1, (B, D, H, W))),
                _t(prng.normal(s + 2, (O, C, 1, 1), 0.1)), _t(prng.normal(s + 3, (O,), 0.5)),
                _t(prng.coords_with_flow(s + 4, B, H, W, 2.0)), _t(prng.coords_with_flow(s + 5, B, H, W, 5.0)),
                _t(prng.coords_with_flow(s + 6, B, H, W, 3.0)),
                _t(prng.normal(s + 7, (B, C, H, W))), _t(prng.normal(s + 8, (B, C, H, W))),
                _t(prng.normal(s + 9, (B, O, H, W)))]

    def run(f1, f2, w, b, c0, c1, c2, g0, g1, g2):
        blk = ea.CorrBlock(f1, f2, num_levels=L, radius=R, differentiable=True)
        o = [blk(c0), blk(c1), blk.lookup_conv1x1_relu(c2, w, b)]
        loss = sum((a * g).sum() for a, g in zip(o, (g0, g1, g2)))
        return o + list(torch.autograd.grad(loss, [f1, f2, w, b]))
    return Case(gen, run, grad=(0, 1, 2, 3))


def _corr_backward_small_r(ea):
    B, D, H, W, L, R = 2, 3, 8, 8, 3, 1                        # lookup_backward_kernel<-1>
    C = L * (2 * R + 1) ** 2

    def gen(i):
        s = 27000 + 100 * i
        return [_t(prng.normal(s, (B, D, H, W))), _t(prng.normal(s + 1, (B, D, H, W))),
                _t(prng.coords_with_flow(s + 2, B, H, W, 1.0)), _t(prng.coords_with_flow(s + 3, B, H, W, 3.0)),
                _t(prng.normal(s + 4, (B, C, H, W))), _t(prng.normal(s + 5, (B, C, H, W)))]

    def run(f1, f2, c0, c1, g0, g1):
        blk = ea.CorrBlock(f1, f2, num_levels=L, radius=R, differentiable=True)
        o = [blk(c0), blk(c1)]
        loss = sum((a * g).sum() for a, g in zip(o, (g0, g1)))
        return o + list(torch.autograd.grad(loss, [f1, f2]))
    return Case(gen, run, grad=(0, 1))


def _upsample_backward(ea):
    N, H, W = 2, 7, 9

    def gen(i):
        s = 28000 + 100 * i
        return [_t(prng.normal(s, (N, 2, H, W), 3.0)), _t(prng.normal(s + 1, (N, 576, H, W))),
                _t(prng.normal(s + 2, (N, 2, 8 * H, 8 * W)))]

    def run(flow, mask, go):
        outs = []
        for f, m in ((flow, mask), (flow, mask.detach()), (flow.detach(), mask)):   # both, flow alone, mask alone
            up = ea.upsample_flow(f, m)
            outs.append(up)
            outs += list(torch.autograd.grad((up * go).sum(), [v for v in (f, m) if v.requires_grad]))
        return outs
    return Case(gen, run, grad=(0, 1))


CASES = {
    "convc1_split": lambda ea: _convc1(ea, ("split",)),
    "convc1_presplit": lambda ea: _convc1(ea, ("presplit",)),
    "convc1_fused": lambda ea: _convc1(ea, ("fused",)),
    "convc1_half[f16]": lambda ea: _convc1(ea, ("split", "fused"), ((16, 24),), (F16,), 21500),
    "convc1_half[bf16]": lambda ea: _convc1(ea, ("split", "fused"), ((16, 24),), (BF16,), 21500),
    "lookup_half[f16]": lambda ea: _lookup_half(ea, F16),
    "lookup_half[bf16]": lambda ea: _lookup_half(ea, BF16),
    "lookup_other_radius": _lookup_other_radius,
    "alt_window": lambda ea: _alt(ea, "a4_17x21_d37"),
    "alt_generic": lambda ea: _alt(ea, "a5_17x21_d8"),
    "voxel_dsec[norm]": lambda ea: _voxel(ea, True),
    "voxel_dsec[raw]": lambda ea: _voxel(ea, False),
    "sampler_grid_png": _sampler_grid_png,
    "corr_backward": _corr_backward,
    "corr_backward_small_r": _corr_backward_small_r,
    "upsample_backward": _upsample_backward,
}


# The three backward steps are not captured.  corr_backward ended the process with a segmentation fault
# inside torch.cuda.graph's capture_end (torch/cuda/graphs.py, no frame of this project on the stack,
# torch 2.10 on ROCm 7.0; DESIGN.md §3.7 has the message), after the 13 forward steps had passed.  What
# sets it apart from them is autograd's worker thread launching into the capture, which the other two
# backward steps share, so they were not tried.  All three keep their second-stream check below.
NOT_CAPTURED = ("corr_backward", "corr_backward_small_r", "upsample_backward")


@pytest.mark.parametrize("name", [n for n in CASES if n not in NOT_CAPTURED])
def test_replay_is_eager(ea, name):
    case = CASES[name](ea)
    replay_matches_eager(case.step, case.mutate, case.outs, n=NSETS + 1)   # sets 0, 1, 2, then 0 again
    assert all(o.numel() > 0 for o in case.outs)


@pytest.mark.parametrize("name", list(CASES))
def test_second_stream_is_the_default_stream(ea, name):
    base = CASES[name](ea)
    base.mutate(1)
    base.step()
    want = snapshot(base.outs)
    s = torch.cuda.Stream(DEV)
    with torch.cuda.stream(s):
        case = CASES[name](ea)   # the inputs are produced on s
        case.mutate(1)
        case.step()
        s.synchronize()
        got = snapshot(case.outs)
    d = first_difference(got, want)
    assert d is None, f"{name} on a second stream against the default stream: {d}"


# ---- ERAFT.forward, one module-scoped net per variant
FUSED = {"fuse_motion_corr": True, "hip_upsample": True}
# variant: (subtype, constructor keywords, ECORR_CONVC1 or None)
ERAFT_VARIANTS = {
    "default": ("standard", {}, None),
    "fused_split": ("standard", FUSED, "split"),
    "fused_presplit": ("standard", FUSED, "presplit"),
    "fused_fused": ("standard", FUSED, "fused"),
    "mixed": ("standard", dict(FUSED, mixed_precision=True), "split"),
    "alternate": ("standard", {"alternate_corr": True, "hip_upsample": True}, None),
    "warm_start": ("warm_start", FUSED, "split"),
}


@pytest.fixture(scope="module")
def eraft_nets(ea):
    import eraft_amd.network as nw
    cache, weights = {}, {}

    def get(variant):
        if variant not in cache:
            subtype, kw, _ = ERAFT_VARIANTS[variant]
            net = nw.ERAFT({"subtype": subtype}, n_first_channels=5, **kw)
            if not weights:   # the keys and shapes do not depend on the variant
                weights.update(make_state_dict(net.state_dict()))
            net.load_state_dict(weights)
            cache[variant] = net.to(DEV).eval()
        return cache[variant]
    return get


@pytest.fixture
def deterministic_convs():
    saved = (torch.backends.cudnn.deterministic, torch.backends.cuda.matmul.allow_tf32, torch.backends.cudnn.allow_tf32)
    torch.backends.cudnn.deterministic = True   # MIOpen's deterministic algorithm choice, as test_alt_corr_gpu._flow
    torch.backends.cuda.matmul.allow_tf32 = False
    torch.backends.cudnn.allow_tf32 = False
    yield
    (torch.backends.cudnn.deterministic, torch.backends.cuda.matmul.allow_tf32, torch.backends.cudnn.allow_tf32) = saved


@pytest.mark.parametrize("variant", list(ERAFT_VARIANTS))
def test_eraft_replay_is_eager(ea, eraft_nets, deterministic_convs, monkeypatch, variant):
    subtype, _, convc1 = ERAFT_VARIANTS[variant]
    if convc1 is not None:
        monkeypatch.setenv("ECORR_CONVC1", convc1)
    net = eraft_nets(variant)
    warm = subtype == "warm_start"

    def gen(i):
        s = 29000 + 100 * i
        ts = [_t(prng.normal(s, (1, 5, 128, 128))), _t(prng.normal(s + 1, (1, 5, 128, 128)))]
        return ts + [_t(prng.normal(s + 2, (1, 2, 16, 16), 2.0))] if warm else ts

    def run(im1, im2, flow_init=None):
        with torch.no_grad():
            low, ups = net(im1, im2, iters=2, flow_init=flow_init)
        return [low] + list(ups)

    case = Case(gen, run)
    # without this the comparison below proves nothing: two eager runs are the same bits
    case.step()
    a = snapshot(case.outs)
    case.step()
    d = first_difference(snapshot(case.outs), a)
    assert d is None, f"ERAFT[{variant}]: two eager runs differ: {d}"
    assert len(case.outs) == 3 and all(bool(torch.isfinite(o).all()) for o in case.outs)
    replay_matches_eager(case.step, case.mutate, case.outs, n=NSETS)   # sets 0, 1, then 0 again


# ---- the entry points that read an error flag on the host say that they are not capturable
class _Seq:
    pass


def test_host_reading_entry_points_refuse_capture(ea):
    png = torch.zeros((6, 7, 3), dtype=torch.int16, device=DEV).view(torch.uint16)
    seq = _Seq()
    seq.features, seq.image_width, seq.image_height = prng.mvsec_events(640, 100, 6, 7), 7, 6
    vox = ea.EventSequenceToVoxelGrid_Pytorch(5, gpu=True, normalize=True)
    x = torch.zeros(8, device=DEV)
    torch.cuda.synchronize()
    g = torch.cuda.CUDAGraph()
    with torch.cuda.graph(g):
        y = x + 1                                               # (the graph is not empty)
        with pytest.raises(RuntimeError, match=r"flow_16bit_to_float .* cannot be captured"):
            ea.flow_16bit_to_float(png)
        with pytest.raises(RuntimeError, match=r"EventSequenceToVoxelGrid_Pytorch\.__call__ .* cannot be captured"):
            vox(seq)
    g.replay()
    torch.cuda.synchronize()
    assert bool((y == 1).all())
    # outside a capture both run as before
    flow, valid = ea.flow_16bit_to_float(png)
    assert tuple(flow.shape) == (6, 7, 2) and not bool(valid.any())
    assert tuple(vox(seq).shape) == (5, 6, 7)
