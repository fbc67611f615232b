"""CPU-side checks of the SepConvGRU backward entries in the C ABI (ecorr_sepconv_gru_backward_packed_size,
ecorr_sepconv_gru_backward_pack, ecorr_sepconv_gru_backward_workspace_size, ecorr_sepconv_gru_backward; added
within ABI 17) and of the Python opt-ins (sepconv_gru_train, ERAFT(train_gru=True)): the header declares the
entries, libecorr.so exports them, _lib registers them, the version is unchanged, the sizes are the header's
formulas, and every documented ECORR_EINVAL case returns it before any GPU call -- the device pointers are null
or fake throughout, so nothing can be launched."""
import ctypes
import inspect
import os
import subprocess

import pytest

from conftest import ROOT
from grad_slab_rule import assert_slab_shapes, slab_rule

NAMES = ("ecorr_sepconv_gru_backward_packed_size", "ecorr_sepconv_gru_backward_pack",
         "ecorr_sepconv_gru_backward_workspace_size", "ecorr_sepconv_gru_backward")
HID, INP = 128, 256


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
    i, i64p, p, pp = ctypes.c_int, ctypes.POINTER(ctypes.c_int64), ctypes.c_void_p, ctypes.POINTER(ctypes.c_void_p)
    assert _lib.SYMBOLS["ecorr_sepconv_gru_backward_packed_size"][1] == [i, i, i64p]
    assert _lib.SYMBOLS["ecorr_sepconv_gru_backward_pack"][1] == [pp, i, i, p, p]
    assert _lib.SYMBOLS["ecorr_sepconv_gru_backward_workspace_size"][1] == [i, i, i, i, i, i64p]
    assert _lib.SYMBOLS["ecorr_sepconv_gru_backward"][1] == [p, p, p, i, i, i, i, i, p, p, p, p, pp, pp, p, p]
    assert "int ecorr_sepconv_gru_backward_packed_size(int hidden, int input, int64_t* bytes);" in header
    assert ("int ecorr_sepconv_gru_backward_pack(const float* const weight[6], int hidden, int input, "
            "void* packed_t, void* stream);") in header
    assert ("int ecorr_sepconv_gru_backward_workspace_size(int B, int hidden, int input, int H, int W, "
            "int64_t* bytes);") in header
    assert ("int ecorr_sepconv_gru_backward(const float* h, const float* x, const float* grad_out,\n"
            "                               int B, int hidden, int input, int H, int W,\n"
            "                               const void* packed, const void* packed_t,\n"
            "                               float* grad_h, float* grad_x,\n"
            "                               float* const grad_weight[6], float* const grad_bias[6],\n"
            "                               void* workspace, void* stream);") in header
    srcs = open(os.path.join(ROOT, "e-raft_amd", "csrc", "Makefile")).read().split("SRCS")[1].split("\n")[0]
    assert "gru_grad.hip" in srcs.split() and "gru.hip" in srcs.split()


def workspace_formula(B, H, W):
    """include/ecorr.h: 13 tensors of h's size, the bias partials and the weight slab partials."""
    P = H * W
    n = B * HID * P * 4
    _, nsl, _, _ = slab_rule(B, P)
    bias = (B * -(-P // 64) * 384 * 4 + 255) // 256 * 256
    return 13 * n + bias + B * nsl * 5 * 256 * 384 * 4


def test_sizes(ea):
    from eraft_amd import _lib
    L, E = ea.lib(), _lib.ECORR_EINVAL
    n = ctypes.c_int64(-1)
    assert L.ecorr_sepconv_gru_backward_packed_size(HID, INP, ctypes.byref(n)) == _lib.ECORR_OK
    assert n.value == 4 * 6 * HID * (HID + INP) * 5 > 0    # the header's formula: the six weights, no biases
    assert n.value % 16 == 0

    def ws(B, H, W):
        m = ctypes.c_int64(-1)
        assert L.ecorr_sepconv_gru_backward_workspace_size(B, HID, INP, H, W, ctypes.byref(m)) == _lib.ECORR_OK
        return m.value

    # one slab; two slabs of 1024 and 976; a doubled cap (16 x 5 > 64: 3 slabs of 1600); MVSEC B = 64; one pixel
    for B, H, W in ((2, 7, 70), (2, 40, 50), (16, 60, 80), (64, 32, 32), (1, 1, 1), (1, 60, 80), (4, 92, 160),
                    (100, 33, 33)):
        assert ws(B, H, W) == workspace_formula(B, H, W), (B, H, W)
        assert ws(B, H, W) % 16 == 0
    assert workspace_formula(2, 40, 50) == 13 * 2 * HID * 2000 * 4 + 2 * 32 * 384 * 4 + 4 * 5 * 256 * 384 * 4
    assert workspace_formula(16, 60, 80) == 13 * 16 * HID * 4800 * 4 + 16 * 75 * 384 * 4 + 48 * 5 * 256 * 384 * 4
    base = ws(2, 16, 24)
    assert ws(3, 16, 24) > base and ws(2, 17, 24) > base and ws(2, 16, 25) > base
    assert L.ecorr_sepconv_gru_backward_packed_size(HID, INP, None) == E
    assert L.ecorr_sepconv_gru_backward_workspace_size(1, HID, INP, 8, 8, None) == E
    for hid, inp in ((64, 256), (128, 128), (256, 128), (0, 0), (-128, 256), (128, 320)):   # unsupported sizes
        assert L.ecorr_sepconv_gru_backward_packed_size(hid, inp, ctypes.byref(n)) == E, (hid, inp)
        assert L.ecorr_sepconv_gru_backward_workspace_size(1, hid, inp, 8, 8, ctypes.byref(n)) == E, (hid, inp)
    # the forward's geometry limits
    for B, H, W in ((0, 8, 8), (-1, 8, 8), (1, 0, 8), (1, 8, 0), (1, -3, 8), (65536, 1, 1), (1, 1, 1398102),
                    (2, 1, 699051), (1, 46341, 46341)):
        assert L.ecorr_sepconv_gru_backward_workspace_size(B, HID, INP, H, W, ctypes.byref(n)) == E, (B, H, W)
    assert ws(1, 1, 1398101) == workspace_formula(1, 1, 1398101)


def test_slab_shapes(ea):
    """grad_slab_rule's table of the doubled cap and the second chain holds under the rule, and the library sizes
    its workspace by that geometry: 33 and 44 slabs of partials."""
    from eraft_amd import _lib
    assert_slab_shapes()
    for (B, H, W), slabs in (((33, 25, 41), 33), ((22, 33, 63), 44)):
        m = ctypes.c_int64(-1)
        assert ea.lib().ecorr_sepconv_gru_backward_workspace_size(B, HID, INP, H, W, ctypes.byref(m)) == _lib.ECORR_OK
        assert m.value == workspace_formula(B, H, W), (B, H, W)
        assert (m.value - 13 * B * HID * H * W * 4 - (B * -(-H * W // 64) * 384 * 4 + 255) // 256 * 256
                == slabs * 5 * 256 * 384 * 4), (B, H, W)


def test_validation_before_launch(ea):
    from eraft_amd import _lib
    L, E = ea.lib(), _lib.ECORR_EINVAL
    back, pack = L.ecorr_sepconv_gru_backward, L.ecorr_sepconv_gru_backward_pack
    ok = 1 << 26       # fake, 16-byte aligned device addresses 64 MB apart (the workspace below is 4 MB, a pack
    # 5.9 MB): never dereferenced on the host, and every call below fails its validation before a launch
    geom = (1, HID, INP, 4, 4)               # B, hidden, input, H, W: 8 KB of h and grad_out, 16 KB of x
    h, x, go, packed, packed_t, gh, gx, ws = [ok * (k + 1) for k in range(8)]
    gws = [ok * 9 + (1 << 20) * k for k in range(6)]      # 983040 bytes each, 1 MB apart
    gbs = [ok * 10 + 4096 * k for k in range(6)]          # 512 bytes each

    def six(ptrs):
        return None if ptrs is None else (ctypes.c_void_p * 6)(*ptrs)

    def call(h=h, x=x, go=go, packed=packed, packed_t=packed_t, gh=gh, gx=gx, gw=gws, gb=gbs, ws=ws, g=geom):
        return back(h, x, go, *g, packed, packed_t, gh, gx, six(gw), six(gb), ws, None)

    for k in ("h", "x", "go", "packed", "packed_t", "ws"):   # each required pointer null in turn
        assert call(**{k: None}) == E, k
    for k in ("packed", "packed_t", "ws"):                   # the packs and the workspace misaligned in turn
        assert call(**{k: locals()[k] + 4}) == E, k
    assert call(gh=None, gx=None, gw=None, gb=None) == E     # nothing wanted
    assert call(gb=None) == E                                # grad_weight without grad_bias, and the reverse
    assert call(gw=None) == E
    for k in range(6):                                       # a hole in either array
        assert call(gw=gws[:k] + [None] + gws[k + 1:]) == E, k
        assert call(gb=gbs[:k] + [None] + gbs[k + 1:]) == E, k
    nws = 13 * HID * 16 * 4 + 384 * 4 + 5 * 256 * 384 * 4    # the workspace of this geometry (one slab)
    assert nws == workspace_formula(1, 4, 4)
    # an output overlapping an input, a pack or the workspace
    for k, name in ((h, "h"), (x, "x"), (go, "grad_out"), (packed, "packed"), (packed_t, "packed_t"), (ws, "ws")):
        assert call(gh=k) == E, name
        assert call(gx=k + 4096) == E, name
        assert call(gw=gws[:3] + [k] + gws[4:]) == E, name
        assert call(gb=gbs[:5] + [k + 256]) == E, name
    assert call(gh=h + 8192 - 16) == E and call(gh=h - 8192 + 16) == E
    assert call(gx=ws + nws - 16) == E and call(gx=ws - 16384 + 16) == E
    # two outputs overlapping
    assert call(gx=gh) == E and call(gx=gh + 4096) == E and call(gh=gx + 8192) == E
    assert call(gw=gws[:1] + gws[:1] + gws[2:]) == E
    assert call(gw=gws[:5] + [gws[4] + 983040 - 16]) == E
    assert call(gb=gbs[:1] + gbs[:1] + gbs[2:]) == E
    assert call(gb=gbs[:5] + [gbs[4] + 512 - 16]) == E
    assert call(gb=gbs[:5] + [gws[2] + 1024]) == E
    assert call(gh=gws[5] + 983040 - 16) == E and call(gx=gbs[0]) == E
    # the workspace overlapping what is read while it is written
    for k, name in ((h, "h"), (x, "x"), (go, "grad_out"), (packed, "packed"), (packed_t, "packed_t")):
        assert call(ws=k) == E, name
        assert call(ws=k - nws + 16) == E, name
    for B, H, W in ((0, 4, 4), (-2, 4, 4), (1, 0, 4), (1, 4, 0), (1, 4, -1), (65536, 1, 1), (1, 1, 1398102),
                    (2, 1, 699051)):
        assert call(g=(B, HID, INP, H, W)) == E, (B, H, W)
    for hid, inp in ((64, 256), (128, 128), (128, 320), (0, 256)):
        assert call(g=(1, hid, inp, 4, 4)) == E, (hid, inp)
    full = six([ok] * 6)
    assert pack(None, HID, INP, ok, None) == E
    assert pack(full, HID, INP, None, None) == E
    assert pack(full, HID, INP, ok + 4, None) == E
    assert pack(six([ok, ok, ok, None, ok, ok]), HID, INP, ok, None) == E
    assert pack(full, 64, INP, ok, None) == E
    assert pack(full, HID, 128, ok, None) == E


def test_python_interface():
    import eraft_amd
    from eraft_amd import network
    assert callable(eraft_amd.sepconv_gru_train) and "sepconv_gru_train" in eraft_amd.__all__
    assert list(inspect.signature(eraft_amd.sepconv_gru_train).parameters) == ["h", "x", "gru"]
    a = inspect.signature(network.ERAFT.__init__).parameters["train_gru"]
    assert a.default is False and a.kind is inspect.Parameter.KEYWORD_ONLY
    cfg = {"subtype": "standard"}
    plain = network.ERAFT(cfg, 3)
    assert not plain.train_gru and not plain.update_block.train_gru
    net = network.ERAFT(cfg, 3, train_gru=True)
    assert net.train_gru and net.update_block.train_gru and not net.hip_gru
    assert list(net.state_dict()) == list(plain.state_dict())   # the same keys
    for kw in ({"differentiable_corr": True}, {"train_motion_corr": True}, {"train_alternate_corr": True},
               {"fuse_motion_corr": True}, {"hip_upsample": True}, {"alternate_corr": True},
               {"differentiable_corr": True, "hip_upsample": True}, {"train_motion_corr": True, "hip_upsample": True}):
        assert network.ERAFT(cfg, 3, train_gru=True, **kw).update_block.train_gru
        both = network.ERAFT(cfg, 3, train_gru=True, hip_gru=True, **kw)   # hip_gru passed along changes nothing
        assert both.update_block.train_gru and list(both.state_dict()) == list(plain.state_dict())
    with pytest.raises(ValueError, match="train_gru"):
        network.ERAFT(cfg, 3, train_gru=True, mixed_precision=True)
    with pytest.raises(ValueError, match="train_gru"):
        network.ERAFT(cfg, 3, train_gru=True, hip_gru=True, mixed_precision=True)
    for kw in ({"mixed_precision": True}, {"differentiable_corr": True}, {"train_motion_corr": True},
               {"train_alternate_corr": True}):   # hip_gru alone keeps its refusals
        with pytest.raises(ValueError, match="hip_gru"):
            network.ERAFT(cfg, 3, hip_gru=True, **kw)


def test_cpu_inputs_are_refused():
    """No fallback: a CPU tensor raises, whether or not a device is present and whether or not grad is wanted."""
    import torch

    import eraft_amd
    from eraft_amd import network
    gru = network.SepConvGRU(HID, INP)
    with pytest.raises(RuntimeError, match="HIP devices"):
        eraft_amd.sepconv_gru_train(torch.zeros(1, HID, 2, 2, requires_grad=True), torch.zeros(1, INP, 2, 2), gru)
    with torch.no_grad(), pytest.raises(RuntimeError, match="HIP devices"):
        eraft_amd.sepconv_gru_train(torch.zeros(1, HID, 2, 2), torch.zeros(1, INP, 2, 2), gru)
