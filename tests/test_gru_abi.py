"""CPU-side checks of the SepConvGRU entries in the C ABI (ecorr_sepconv_gru_packed_size, ecorr_sepconv_gru_pack,
ecorr_sepconv_gru_workspace_size, ecorr_sepconv_gru; added within ABI 17) and of the Python opt-ins: the header
declares the entries, libecorr.so exports them, _lib registers them, the version is unchanged, the sizes are
the header's formulas, and every documented ECORR_EINVAL case returns it before any GPU call -- the device
pointers are null or fake throughout, so nothing can be launched."""
import ctypes
import inspect
import os
import subprocess

import pytest

from conftest import ROOT

NAMES = ("ecorr_sepconv_gru_packed_size", "ecorr_sepconv_gru_pack", "ecorr_sepconv_gru_workspace_size",
         "ecorr_sepconv_gru")
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
    assert _lib.SYMBOLS["ecorr_sepconv_gru_packed_size"][1] == [i, i, i64p]
    assert _lib.SYMBOLS["ecorr_sepconv_gru_pack"][1] == [pp, pp, i, i, p, p]
    assert _lib.SYMBOLS["ecorr_sepconv_gru_workspace_size"][1] == [i, i, i, i, i, i64p]
    assert _lib.SYMBOLS["ecorr_sepconv_gru"][1] == [p, p, i, i, i, i, i, p, p, p, p]
    assert "int ecorr_sepconv_gru_packed_size(int hidden, int input, int64_t* bytes);" in header
    assert ("int ecorr_sepconv_gru_pack(const float* const weight[6], const float* const bias[6],\n"
            "                           int hidden, int input, void* packed, void* stream);") in header
    assert "int ecorr_sepconv_gru_workspace_size(int B, int hidden, int input, int H, int W, int64_t* bytes);" in header
    assert ("int ecorr_sepconv_gru(const float* h, const float* x, int B, int hidden, int input, int H, int W,\n"
            "                      const void* packed, float* h_out, void* workspace, void* stream);") in header
    assert "hidden = 128 and input = 256 only" in header   # the header says which sizes are supported
    srcs = open(os.path.join(ROOT, "e-raft_amd", "csrc", "Makefile")).read().split("SRCS")[1].split("\n")[0]
    assert "gru.hip" in srcs.split()


def test_sizes(ea):
    from eraft_amd import _lib
    L, E = ea.lib(), _lib.ECORR_EINVAL
    n = ctypes.c_int64(-1)
    assert L.ecorr_sepconv_gru_packed_size(HID, INP, ctypes.byref(n)) == _lib.ECORR_OK
    # the header's formula: six [hidden][hidden + input][5] weights and six biases, fp32
    assert n.value == 4 * (6 * HID * (HID + INP) * 5 + 6 * HID) > 0
    assert n.value % 16 == 0

    def ws(B, H, W):
        m = ctypes.c_int64(-1)
        assert L.ecorr_sepconv_gru_workspace_size(B, HID, INP, H, W, ctypes.byref(m)) == _lib.ECORR_OK
        return m.value

    assert ws(2, 7, 70) == 3 * 2 * HID * 7 * 70 * 4     # the header's formula: h1, z and r*h
    assert ws(16, 60, 80) == 3 * 16 * HID * 4800 * 4    # DSEC B = 16: 118 MB
    assert ws(1, 1, 1) == 3 * HID * 4 > 0
    base = ws(2, 16, 24)
    assert ws(3, 16, 24) > base and ws(2, 17, 24) > base and ws(2, 16, 25) > base
    assert L.ecorr_sepconv_gru_packed_size(HID, INP, None) == E
    assert L.ecorr_sepconv_gru_workspace_size(1, HID, INP, 8, 8, None) == E
    for hid, inp in ((64, 256), (128, 128), (256, 128), (0, 0), (-128, 256), (128, 320)):   # unsupported sizes
        assert L.ecorr_sepconv_gru_packed_size(hid, inp, ctypes.byref(n)) == E, (hid, inp)
        assert L.ecorr_sepconv_gru_workspace_size(1, hid, inp, 8, 8, ctypes.byref(n)) == E, (hid, inp)
    for B, H, W in ((0, 8, 8), (-1, 8, 8), (1, 0, 8), (1, 8, 0), (1, -3, 8), (65536, 1, 1)):
        assert L.ecorr_sepconv_gru_workspace_size(B, HID, INP, H, W, ctypes.byref(n)) == E, (B, H, W)
    # B (hidden + input) H W 4 within the 2^31 - 1 buffer range: 1398101 pixels fit, one more does not
    assert ws(1, 1, 1398101) > 0
    assert L.ecorr_sepconv_gru_workspace_size(1, HID, INP, 1, 1398102, ctypes.byref(n)) == E
    assert L.ecorr_sepconv_gru_workspace_size(2, HID, INP, 1, 699051, ctypes.byref(n)) == E
    assert L.ecorr_sepconv_gru_workspace_size(1, HID, INP, 46341, 46341, ctypes.byref(n)) == E   # H W past an int


def test_validation_before_launch(ea):
    from eraft_amd import _lib
    L, E = ea.lib(), _lib.ECORR_EINVAL
    gru, pack = L.ecorr_sepconv_gru, L.ecorr_sepconv_gru_pack
    ok = 1 << 24       # fake, 16-byte aligned device addresses 16 MB apart (the pack is 5.9 MB): never dereferenced
    far = [ok * (k + 1) for k in range(5)]   # on the host, and every call below fails its validation before a launch
    geom = (1, HID, INP, 4, 4)               # B, hidden, input, H, W: 8 KB of h, 16 KB of x

    def call(h, x, packed, out, ws, g=geom):
        return gru(h, x, *g, packed, out, ws, None)

    assert call(None, None, None, None, None) == E
    for k in range(5):   # each pointer null in turn, the others fake
        ptrs = list(far)
        ptrs[k] = None
        assert call(*ptrs) == E, k
    for k in (2, 4):     # the packed buffer and the workspace misaligned in turn
        ptrs = list(far)
        ptrs[k] += 4
        assert call(*ptrs) == E, k
    h, x, packed, out, ws = far
    assert call(h, x, packed, h, ws) == E            # h_out aliasing h
    assert call(h, x, packed, x, ws) == E            # h_out aliasing x
    assert call(h, x, packed, h + 4096, ws) == E     # ... or overlapping either
    assert call(h, x, packed, x + 8192, ws) == E
    assert call(h, x, packed, x - 4096, ws) == E
    nws = 3 * HID * 16 * 4                            # the workspace of this geometry: 24 KB
    assert call(h, x, packed, out, h) == E           # the workspace overlapping h, x or h_out
    assert call(h, x, packed, out, x + 16384 - 16) == E
    assert call(h, x, packed, out, out - nws + 16) == E
    assert call(h, x, packed, out, out + 8192 - 16) == E
    assert call(h, x, packed, ws + nws - 16, ws) == E
    assert call(h, x, packed, out, packed + 4096) == E   # the pack overlapping the workspace or h_out
    assert call(h, x, out - 4096, out, ws) == E
    for B, H, W in ((0, 4, 4), (-2, 4, 4), (1, 0, 4), (1, 4, 0), (1, 4, -1), (65536, 1, 1), (1, 1, 1398102),
                    (2, 1, 699051)):
        assert call(*far, g=(B, HID, INP, H, W)) == E, (B, H, W)
    for hid, inp in ((64, 256), (128, 128), (128, 320), (0, 256)):
        assert call(*far, g=(1, hid, inp, 4, 4)) == E, (hid, inp)
    six = (ctypes.c_void_p * 6)(*[ok] * 6)
    hole = (ctypes.c_void_p * 6)(ok, ok, ok, None, ok, ok)
    assert pack(None, six, HID, INP, ok, None) == E
    assert pack(six, None, HID, INP, ok, None) == E
    assert pack(six, six, HID, INP, None, None) == E
    assert pack(six, six, HID, INP, ok + 4, None) == E
    assert pack(hole, six, HID, INP, ok, None) == E
    assert pack(six, hole, HID, INP, ok, None) == E
    assert pack(six, six, 64, INP, ok, None) == E
    assert pack(six, six, HID, 128, ok, None) == E
    with pytest.raises(ValueError):
        _lib.check(E, "sepconv_gru")


def test_python_interface():
    import eraft_amd
    from eraft_amd import network
    assert callable(eraft_amd.sepconv_gru) and "sepconv_gru" in eraft_amd.__all__
    assert list(inspect.signature(eraft_amd.sepconv_gru).parameters) == ["h", "x", "gru"]
    a = inspect.signature(network.ERAFT.__init__).parameters["hip_gru"]
    assert a.default is False and a.kind is inspect.Parameter.KEYWORD_ONLY
    cfg = {"subtype": "standard"}
    plain = network.ERAFT(cfg, 3)
    assert not plain.hip_gru and not plain.update_block.hip_gru
    net = network.ERAFT(cfg, 3, hip_gru=True)
    assert net.hip_gru and net.update_block.hip_gru
    assert list(net.state_dict()) == list(plain.state_dict())   # the same keys
    for kw in ({"fuse_motion_corr": True}, {"hip_upsample": True}, {"alternate_corr": True},
               {"fuse_motion_corr": True, "hip_upsample": True}):
        assert network.ERAFT(cfg, 3, hip_gru=True, **kw).update_block.hip_gru
    for kw in ({"mixed_precision": True}, {"differentiable_corr": True}, {"train_motion_corr": True},
               {"train_alternate_corr": True}):
        with pytest.raises(ValueError, match="hip_gru"):
            network.ERAFT(cfg, 3, hip_gru=True, **kw)


def test_cpu_inputs_are_refused():
    """No fallback: a CPU tensor raises, whether or not a device is present."""
    import torch

    import eraft_amd
    from eraft_amd import network
    gru = network.SepConvGRU(HID, INP)
    with torch.no_grad(), pytest.raises(RuntimeError, match="HIP devices"):
        eraft_amd.sepconv_gru(torch.zeros(1, HID, 2, 2), torch.zeros(1, INP, 2, 2), gru)
