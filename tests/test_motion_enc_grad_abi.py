"""CPU-side checks of the motion encoder backward entries in the C ABI (ecorr_motion_encoder_backward_packed_size,
ecorr_motion_encoder_backward_pack, ecorr_motion_encoder_backward_workspace_size, ecorr_motion_encoder_backward; added
within ABI 17) and of the Python opt-ins (motion_encoder_train, ERAFT(train_motion_encoder=True)): the header declares
the entries, libecorr.so exports them, _lib registers them, the version is unchanged, the sizes are the header's
formulas, and every documented ECORR_EINVAL case returns it before any GPU call -- the device pointers are null or
fake throughout, so nothing can be launched."""
import ctypes
import inspect
import os
import subprocess

import pytest

from conftest import ROOT
from grad_slab_rule import assert_slab_shapes, slab_rule

NAMES = ("ecorr_motion_encoder_backward_packed_size", "ecorr_motion_encoder_backward_pack",
         "ecorr_motion_encoder_backward_workspace_size", "ecorr_motion_encoder_backward")
PACKED = 4 * (9 * 256 * 192 + 9 * 128 * 64 + 9 * 256 * 128 + 128 * 100 + 512)   # the forward pack
PACKED_T = 4 * 9 * (256 * 128 + 256 * 192 + 128 * 64)                            # the header's formula
HW_MAX = 2097151   # 256 * H * W * 4 <= 2^31 - 1
WSIZE = (192 * 256 * 9 * 4, 128 * 2 * 49 * 4, 64 * 128 * 9 * 4, 126 * 256 * 9 * 4)   # convc2 convf1 convf2 conv
BSIZE = (192 * 4, 128 * 4, 64 * 4, 126 * 4)


@pytest.fixture(scope="module")
def ea():
    lib = os.path.join(ROOT, "e-raft_amd", "libecorr.so")
    if not os.path.exists(lib):
        subprocess.run(["make", "-s", "-C", os.path.join(ROOT, "e-raft_amd", "csrc")], check=True)
    import eraft_amd
    eraft_amd.lib()
    return eraft_amd


def test_entries_within_abi_17(ea):
    from eraft_amd import _lib
    L = ea.lib()
    assert L.ecorr_abi_version() == 17 == _lib.ABI_VERSION
    header = open(os.path.join(ROOT, "include", "ecorr.h")).read()
    assert "#define ECORR_ABI_VERSION 17" in header
    for name in NAMES:
        assert name in _lib.SYMBOLS, name
        assert getattr(L, name).argtypes == _lib.SYMBOLS[name][1]
        assert getattr(L, name).restype is ctypes.c_int
    i, i64, i64p, p, pp = (ctypes.c_int, ctypes.c_int64, ctypes.POINTER(ctypes.c_int64), ctypes.c_void_p,
                           ctypes.POINTER(ctypes.c_void_p))
    assert _lib.SYMBOLS["ecorr_motion_encoder_backward_packed_size"][1] == [i64p]
    assert _lib.SYMBOLS["ecorr_motion_encoder_backward_pack"][1] == [pp, p, p]
    assert _lib.SYMBOLS["ecorr_motion_encoder_backward_workspace_size"][1] == [i, i, i, i64p]
    assert _lib.SYMBOLS["ecorr_motion_encoder_backward"][1] == [p, p, p, i64, i, i, i, p, p, p, p, pp, pp, p, p]
    assert "int ecorr_motion_encoder_backward_packed_size(int64_t* bytes);" in header
    assert ("int ecorr_motion_encoder_backward_pack(const float* const weight[4], void* packed_t, void* stream);"
            in header)
    assert "int ecorr_motion_encoder_backward_workspace_size(int B, int H, int W, int64_t* bytes);" in header
    assert ("int ecorr_motion_encoder_backward(const float* c1, const float* flow, const float* grad_out,\n"
            "                                  int64_t grad_out_batch_stride, int B, int H, int W,\n"
            "                                  const void* packed, const void* packed_t,\n"
            "                                  float* grad_c1, float* grad_flow,\n"
            "                                  float* const grad_weight[4], float* const grad_bias[4],\n"
            "                                  void* workspace, void* stream);") in header
    srcs = open(os.path.join(ROOT, "e-raft_amd", "csrc", "Makefile")).read().split("SRCS")[1].split("\n")[0]
    assert "motion_enc_grad.hip" in srcs.split() and "motion_enc.hip" in srcs.split()


def workspace_formula(B, H, W):
    """include/ecorr.h: 896 channels of [B][.][H W], the bias partials and the weight slab partials."""
    P = H * W
    n = B * P * 4
    _, nsl, _, _ = slab_rule(B, P)
    bias = (B * -(-P // 64) * 512 * 4 + 255) // 256 * 256
    return 896 * n + bias + B * nsl * 9 * 192 * 256 * 4


def test_sizes(ea):
    from eraft_amd import _lib
    L, E = ea.lib(), _lib.ECORR_EINVAL
    n = ctypes.c_int64(-1)
    assert L.ecorr_motion_encoder_backward_packed_size(ctypes.byref(n)) == _lib.ECORR_OK
    assert n.value == PACKED_T == 3244032
    assert n.value % 16 == 0
    assert L.ecorr_motion_encoder_backward_packed_size(None) == E

    def ws(B, H, W):
        m = ctypes.c_int64(-1)
        assert L.ecorr_motion_encoder_backward_workspace_size(B, H, W, ctypes.byref(m)) == _lib.ECORR_OK
        return m.value

    # one slab; two slabs of 1024 and 976; a doubled cap (16 x 5 > 64: 3 slabs of 1600); MVSEC B = 64; one pixel
    for B, H, W in ((2, 7, 70), (2, 40, 50), (16, 60, 80), (64, 32, 32), (1, 1, 1), (1, 60, 80), (4, 92, 160),
                    (100, 33, 33), (3, 9, 15)):
        assert ws(B, H, W) == workspace_formula(B, H, W), (B, H, W)
        assert ws(B, H, W) % 16 == 0
    assert workspace_formula(2, 40, 50) == 896 * 2 * 2000 * 4 + 2 * 32 * 512 * 4 + 4 * 9 * 192 * 256 * 4
    assert workspace_formula(16, 60, 80) == 896 * 16 * 4800 * 4 + 16 * 75 * 512 * 4 + 48 * 9 * 192 * 256 * 4
    assert workspace_formula(1, 1, 1) == 896 * 4 + 2048 + 9 * 192 * 256 * 4
    base = ws(2, 16, 24)
    assert ws(3, 16, 24) > base and ws(2, 17, 24) > base and ws(2, 16, 25) > base
    assert L.ecorr_motion_encoder_backward_workspace_size(1, 8, 8, None) == E
    # the forward's geometry limits: 2097151 pixels fit, one more does not; the batch does not count against it
    for B, H, W in ((0, 8, 8), (-1, 8, 8), (1, 0, 8), (1, 8, 0), (1, -3, 8), (65536, 1, 1), (1, 1, HW_MAX + 1),
                    (1, HW_MAX + 1, 1), (1, 1024, 2048), (1, 46341, 46341)):
        assert L.ecorr_motion_encoder_backward_workspace_size(B, H, W, ctypes.byref(n)) == E, (B, H, W)
    assert ws(1, 1, HW_MAX) == workspace_formula(1, 1, HW_MAX)
    assert ws(1, HW_MAX, 1) == workspace_formula(1, HW_MAX, 1)
    assert ws(65535, 1, HW_MAX) == workspace_formula(65535, 1, HW_MAX)


def test_slab_shapes(ea):
    """grad_slab_rule's table of the doubled cap and the second chain holds under the rule, and the library sizes
    its workspace by that geometry: 33 and 44 slabs of partials."""
    from eraft_amd import _lib
    assert_slab_shapes()
    for (B, H, W), slabs in (((33, 25, 41), 33), ((22, 33, 63), 44)):
        m = ctypes.c_int64(-1)
        assert ea.lib().ecorr_motion_encoder_backward_workspace_size(B, H, W, ctypes.byref(m)) == _lib.ECORR_OK
        assert m.value == workspace_formula(B, H, W), (B, H, W)
        assert (m.value - 896 * B * H * W * 4 - (B * -(-H * W // 64) * 512 * 4 + 255) // 256 * 256
                == slabs * 9 * 192 * 256 * 4), (B, H, W)


def test_validation_before_launch(ea):
    from eraft_amd import _lib
    L, E = ea.lib(), _lib.ECORR_EINVAL
    back, pack = L.ecorr_motion_encoder_backward, L.ecorr_motion_encoder_backward_pack
    ok = 1 << 26       # fake, 16-byte aligned device addresses 64 MB apart (the workspace below is 1.8 MB, a pack
    # 3.3 MB): never dereferenced on the host, and every call below fails its validation before a launch
    B, H, W = 2, 4, 4
    hw = H * W
    nc1, nfl, ngo = B * 256 * hw * 4, B * 2 * hw * 4, B * 128 * hw * 4
    c1, flow, go, packed, packed_t, gc, gf, ws = [ok * (k + 1) for k in range(8)]
    gws = [ok * 9 + (1 << 21) * k for k in range(4)]      # at most 1769472 bytes each, 2 MB apart
    gbs = [ok * 10 + 4096 * k for k in range(4)]          # at most 768 bytes each
    nws = workspace_formula(B, H, W)
    assert nws == 896 * B * hw * 4 + B * 512 * 4 + B * 9 * 192 * 256 * 4

    def four(ptrs):
        return None if ptrs is None else (ctypes.c_void_p * 4)(*ptrs)

    def call(c1=c1, flow=flow, go=go, packed=packed, packed_t=packed_t, gc=gc, gf=gf, gw=gws, gb=gbs, ws=ws,
             g=(B, H, W), stride=128 * hw):
        return back(c1, flow, go, stride, *g, packed, packed_t, gc, gf, four(gw), four(gb), ws, None)

    for k in ("c1", "flow", "go", "packed", "packed_t", "ws"):   # each required pointer null in turn
        assert call(**{k: None}) == E, k
    for k in ("packed", "packed_t", "ws"):                       # the packs and the workspace misaligned in turn
        assert call(**{k: locals()[k] + 4}) == E, k
    for stride in (128 * hw - 1, 0, -128 * hw, 1):               # a short grad_out_batch_stride
        assert call(stride=stride) == E, stride
    assert call(gc=None, gf=None, gw=None, gb=None) == E         # nothing wanted
    assert call(gb=None) == E                                    # grad_weight without grad_bias, and the reverse
    assert call(gw=None) == E
    for k in range(4):                                           # a hole in either array
        assert call(gw=gws[:k] + [None] + gws[k + 1:]) == E, k
        assert call(gb=gbs[:k] + [None] + gbs[k + 1:]) == E, k
    # an output overlapping an input, a pack or the workspace
    for k, name in ((c1, "c1"), (flow, "flow"), (go, "grad_out"), (packed, "packed"), (packed_t, "packed_t"),
                    (ws, "ws")):
        assert call(gc=k) == E, name
        assert call(gf=k + 64) == E, name
        assert call(gw=gws[:2] + [k] + gws[3:]) == E, name
        assert call(gb=gbs[:3] + [k + 128]) == E, name
    assert call(gc=c1 + nc1 - 16) == E and call(gc=c1 - nc1 + 16) == E
    assert call(gf=flow + nfl - 16) == E and call(gf=flow - nfl + 16) == E
    assert call(gc=ws + nws - 16) == E and call(gc=ws - nc1 + 16) == E
    assert call(gf=packed + PACKED - 16) == E and call(gf=packed_t + PACKED_T - 16) == E
    # grad_out's strided extent: with a batch stride of 256 H W the second item ends (256 + 128) H W floats behind
    # grad_out, so an output clear of the dense extent is still inside the strided one -- also in the gap
    wide = 256 * hw
    ext = (wide + 128 * hw) * 4
    assert ngo < ext
    assert call(gf=go + 128 * hw * 4 + 64, stride=wide) == E              # grad_flow wholly inside the gap
    assert call(gf=go + ext - 16, stride=wide) == E                       # under the last floats of item 1
    assert call(gb=gbs[:3] + [go + ngo + 16], stride=wide) == E           # behind the dense extent, inside item 1
    assert call(ws=go + ext - 16, stride=wide) == E                       # the workspace likewise
    # two outputs overlapping
    assert call(gf=gc) == E and call(gf=gc + nc1 - 16) == E and call(gc=gf - nc1 + 16) == E
    assert call(gw=gws[:1] + gws[:1] + gws[2:]) == E
    assert call(gw=gws[:3] + [gws[2] + WSIZE[2] - 16]) == E
    assert call(gw=[gws[0], gws[0] + WSIZE[0] - 16] + gws[2:]) == E
    assert call(gb=gbs[:1] + gbs[:1] + gbs[2:]) == E
    assert call(gb=gbs[:3] + [gbs[2] + BSIZE[2] - 16]) == E
    assert call(gb=gbs[:3] + [gws[1] + 1024]) == E
    assert call(gc=gws[3] + WSIZE[3] - 16) == E and call(gf=gbs[0]) == E
    # the workspace overlapping what is read while it is written
    for k, name in ((c1, "c1"), (flow, "flow"), (go, "grad_out"), (packed, "packed"), (packed_t, "packed_t")):
        assert call(ws=k) == E, name
        assert call(ws=k - nws + 16) == E, name
    for g in ((0, 4, 4), (-2, 4, 4), (1, 0, 4), (1, 4, 0), (1, 4, -1), (65536, 1, 1), (1, 1, HW_MAX + 1),
              (1, 1024, 2048)):
        assert call(g=g, stride=1 << 32) == E, g
    full = four([ok] * 4)
    assert pack(None, ok, None) == E
    assert pack(full, None, None) == E
    assert pack(full, ok + 4, None) == E
    for k in range(4):
        assert pack(four([None if j == k else ok for j in range(4)]), ok, None) == E, k
    with pytest.raises(ValueError):
        _lib.check(E, "motion_encoder backward")


def test_python_interface():
    import eraft_amd
    from eraft_amd import network
    assert callable(eraft_amd.motion_encoder_train) and "motion_encoder_train" in eraft_amd.__all__
    assert list(inspect.signature(eraft_amd.motion_encoder_train).parameters) == ["flow", "c1", "enc"]
    names = list(inspect.signature(network.ERAFT.__init__).parameters)
    a = inspect.signature(network.ERAFT.__init__).parameters["train_motion_encoder"]
    assert a.default is False and a.kind is inspect.Parameter.KEYWORD_ONLY
    assert names.index("train_motion_encoder") == names.index("hip_motion_encoder") + 1
    cfg = {"subtype": "standard"}
    plain = network.ERAFT(cfg, 3)
    assert not plain.train_motion_encoder
    net = network.ERAFT(cfg, 3, train_motion_encoder=True)
    assert net.train_motion_encoder and not net.hip_motion_encoder
    assert list(net.state_dict()) == list(plain.state_dict())   # the same keys
    for kw in ({"differentiable_corr": True}, {"train_motion_corr": True}, {"train_alternate_corr": True},
               {"train_gru": True}, {"fuse_motion_corr": True}, {"alternate_corr": True}, {"hip_upsample": True},
               {"train_motion_corr": True, "train_gru": True, "hip_upsample": True},
               {"differentiable_corr": True, "train_gru": True}, {"train_alternate_corr": True, "train_gru": True},
               {"train_gru": True, "hip_gru": True}):
        assert network.ERAFT(cfg, 3, train_motion_encoder=True, **kw).train_motion_encoder
        both = network.ERAFT(cfg, 3, train_motion_encoder=True, hip_motion_encoder=True, **kw)   # changes nothing
        assert both.train_motion_encoder and list(both.state_dict()) == list(plain.state_dict())
    with pytest.raises(ValueError, match="train_motion_encoder"):
        network.ERAFT(cfg, 3, train_motion_encoder=True, mixed_precision=True)
    with pytest.raises(ValueError, match="train_motion_encoder"):
        network.ERAFT(cfg, 3, train_motion_encoder=True, hip_motion_encoder=True, mixed_precision=True)
    with pytest.raises(ValueError, match="train_motion_encoder"):
        network.ERAFT(cfg, 3, train_motion_encoder=True, hip_gru=True)
    for kw in ({"mixed_precision": True}, {"differentiable_corr": True}, {"train_motion_corr": True},
               {"train_alternate_corr": True}, {"train_gru": True}):   # hip_motion_encoder alone keeps its refusals
        with pytest.raises(ValueError, match="hip_motion_encoder"):
            network.ERAFT(cfg, 3, hip_motion_encoder=True, **kw)
    doc = network.ERAFT.__doc__
    assert doc.rstrip().endswith("The defaults keep the reference's call pattern exactly.")
    assert "train_motion_encoder=True" in doc


def test_cpu_inputs_are_refused():
    """No fallback: a CPU tensor raises, whether or not a device is present and whether or not grad is wanted."""
    import torch

    import eraft_amd
    from eraft_amd import network
    enc = network.BasicMotionEncoder()
    with pytest.raises(RuntimeError, match="HIP devices"):
        eraft_amd.motion_encoder_train(torch.zeros(1, 2, 2, 2, requires_grad=True), torch.zeros(1, 256, 2, 2), enc)
    with torch.no_grad(), pytest.raises(RuntimeError, match="HIP devices"):
        eraft_amd.motion_encoder_train(torch.zeros(1, 2, 2, 2), torch.zeros(1, 256, 2, 2), enc)
