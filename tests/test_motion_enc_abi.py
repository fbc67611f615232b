"""CPU-side checks of the motion encoder entries in the C ABI (ecorr_motion_encoder_packed_size,
ecorr_motion_encoder_pack, ecorr_motion_encoder_workspace_size, ecorr_motion_encoder; added within ABI 17) and of
the Python opt-ins: the header declares the entries, libecorr.so exports them, _lib registers them, the version is
unchanged, the sizes are the header's formulas, and every documented ECORR_EINVAL case returns it before any GPU
call -- the device pointers are null or fake throughout, so nothing can be launched."""
import ctypes
import inspect
import os
import subprocess

import pytest

from conftest import ROOT

NAMES = ("ecorr_motion_encoder_packed_size", "ecorr_motion_encoder_pack", "ecorr_motion_encoder_workspace_size",
         "ecorr_motion_encoder")
PACKED = 4 * (9 * 256 * 192 + 9 * 128 * 64 + 9 * 256 * 128 + 128 * 100 + 512)   # the header's formula
HW_MAX = 2097151   # 256 * H * W * 4 <= 2^31 - 1


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
    assert _lib.SYMBOLS["ecorr_motion_encoder_packed_size"][1] == [i64p]
    assert _lib.SYMBOLS["ecorr_motion_encoder_pack"][1] == [pp, pp, p, p]
    assert _lib.SYMBOLS["ecorr_motion_encoder_workspace_size"][1] == [i, i, i, i64p]
    assert _lib.SYMBOLS["ecorr_motion_encoder"][1] == [p, p, i, i, i, p, p, i64, p, p]
    assert "int ecorr_motion_encoder_packed_size(int64_t* bytes);" in header
    assert ("int ecorr_motion_encoder_pack(const float* const weight[4], const float* const bias[4], void* packed, "
            "void* stream);") in header
    assert "int ecorr_motion_encoder_workspace_size(int B, int H, int W, int64_t* bytes);" in header
    assert ("int ecorr_motion_encoder(const float* c1, const float* flow, int B, int H, int W, const void* packed,\n"
            "                         float* out, int64_t out_batch_stride, void* workspace, void* stream);") in header
    srcs = open(os.path.join(ROOT, "e-raft_amd", "csrc", "Makefile")).read().split("SRCS")[1].split("\n")[0]
    assert "motion_enc.hip" in srcs.split()
    assert "motion.hip" in srcs.split()   # the fused lookup + convc1 stays its own source


def test_sizes(ea):
    from eraft_amd import _lib
    L, E = ea.lib(), _lib.ECORR_EINVAL
    n = ctypes.c_int64(-1)
    assert L.ecorr_motion_encoder_packed_size(ctypes.byref(n)) == _lib.ECORR_OK
    assert n.value == PACKED == 3297280
    assert n.value % 16 == 0
    assert L.ecorr_motion_encoder_packed_size(None) == E

    def ws(B, H, W):
        m = ctypes.c_int64(-1)
        assert L.ecorr_motion_encoder_workspace_size(B, H, W, ctypes.byref(m)) == _lib.ECORR_OK
        return m.value

    assert ws(2, 7, 70) == 384 * 2 * 7 * 70 * 4          # the header's formula: cor, f1 and flo
    assert ws(16, 60, 80) == 384 * 16 * 4800 * 4         # DSEC B = 16: 118 MB
    assert ws(1, 1, 1) == 384 * 4 > 0
    for B, H, W in ((1, 1, 1), (2, 7, 70), (3, 9, 15), (16, 60, 80), (1, 1, 7)):
        assert ws(B, H, W) % 16 == 0
    base = ws(2, 16, 24)
    assert ws(3, 16, 24) > base and ws(2, 17, 24) > base and ws(2, 16, 25) > base
    assert L.ecorr_motion_encoder_workspace_size(1, 8, 8, None) == E
    for B, H, W in ((0, 8, 8), (-1, 8, 8), (1, 0, 8), (1, 8, 0), (1, -3, 8), (65536, 1, 1)):
        assert L.ecorr_motion_encoder_workspace_size(B, H, W, ctypes.byref(n)) == E, (B, H, W)
    # 256 H W 4 within the 2^31 - 1 buffer range of one batch item: 2097151 pixels fit, one more does not; the
    # batch does not count against it
    assert ws(1, 1, HW_MAX) == 384 * HW_MAX * 4
    assert ws(1, HW_MAX, 1) > 0
    assert ws(65535, 1, HW_MAX) == 384 * 65535 * HW_MAX * 4
    assert L.ecorr_motion_encoder_workspace_size(1, 1, HW_MAX + 1, ctypes.byref(n)) == E
    assert L.ecorr_motion_encoder_workspace_size(1, HW_MAX + 1, 1, ctypes.byref(n)) == E
    assert L.ecorr_motion_encoder_workspace_size(1, 1024, 2048, ctypes.byref(n)) == E     # exactly 2^21 pixels
    assert ws(1, 1023, 2050) > 0                                                          # 2097150
    assert L.ecorr_motion_encoder_workspace_size(1, 46341, 46341, ctypes.byref(n)) == E   # H W past an int


def test_validation_before_launch(ea):
    from eraft_amd import _lib
    L, E = ea.lib(), _lib.ECORR_EINVAL
    enc, pack = L.ecorr_motion_encoder, L.ecorr_motion_encoder_pack
    ok = 1 << 24       # fake, 16-byte aligned device addresses 16 MB apart (the pack is 3.3 MB): never dereferenced
    far = [ok * (k + 1) for k in range(5)]   # on the host, and every call below fails its validation before a launch
    B, H, W = 2, 4, 4
    hw = H * W
    nc1, nfl, nws, nout = B * 256 * hw * 4, B * 2 * hw * 4, 384 * B * hw * 4, B * 128 * hw * 4

    def call(c1, flow, packed, out, ws, g=(B, H, W), stride=128 * hw):
        return enc(c1, flow, *g, packed, out, stride, ws, None)

    assert call(None, None, None, None, None) == E
    for k in range(5):   # each pointer null in turn, the others fake
        ptrs = list(far)
        ptrs[k] = None
        assert call(*ptrs) == E, k
    for k in (2, 4):     # the packed buffer and the workspace misaligned in turn
        ptrs = list(far)
        ptrs[k] += 4
        assert call(*ptrs) == E, k
    c1, flow, packed, out, ws = far
    for stride in (128 * hw - 1, 0, -128 * hw, 1):   # a short out_batch_stride
        assert call(*far, stride=stride) == E, stride
    assert call(c1, flow, packed, c1, ws) == E                    # out aliasing or overlapping c1
    assert call(c1, flow, packed, c1 + nc1 - 4, ws) == E
    assert call(c1, flow, packed, c1 - nout + 4, ws) == E
    assert call(c1, flow, packed, flow, ws) == E                  # ... flow
    assert call(c1, flow, packed, flow + nfl - 4, ws) == E
    assert call(c1, flow, packed, flow - nout + 4, ws) == E
    assert call(c1, flow, packed, packed + 4096, ws) == E         # ... the pack
    assert call(c1, flow, packed, packed + PACKED - 4, ws) == E
    assert call(c1, flow, packed, ws + nws - 4, ws) == E          # ... the workspace
    assert call(c1, flow, packed, ws - nout + 4, ws) == E
    # out's strided extent: with a batch stride of 256 H W the second item ends (256 + 128) H W floats behind out,
    # so an input that lies clear of the dense extent is still inside the strided one -- also in the gap
    wide = 256 * hw
    ext = (wide + 128 * hw) * 4
    assert nout < ext
    gap = out + 128 * hw * 4 + 64   # flow (256 bytes) wholly inside the gap between the two items
    assert gap + nfl <= out + wide * 4
    assert call(c1, gap, packed, out, ws, stride=wide) == E
    assert call(c1, out + ext - 4, packed, out, ws, stride=wide) == E     # flow under the last float of item 1
    assert call(out + nout, flow, packed, out, ws, stride=wide) == E      # c1 behind the dense extent, inside item 1
    assert call(c1, flow, out + nout + 16, out, ws, stride=wide) == E
    assert call(c1, flow, packed, out, out + ext - 16, stride=wide) == E
    assert call(c1, flow, packed, out, c1) == E                  # the workspace overlapping c1, flow or the pack
    assert call(c1, flow, packed, out, c1 + nc1 - 16) == E
    assert call(c1, flow, packed, out, c1 - nws + 16) == E
    assert call(c1, flow, packed, out, flow) == E
    assert call(c1, flow, packed, out, flow + nfl - 16) == E
    assert call(c1, flow, packed, out, flow - nws + 16) == E
    assert call(c1, flow, packed, out, packed + 4096) == E
    assert call(c1, flow, packed, out, packed + PACKED - 16) == E
    for g in ((0, 4, 4), (-2, 4, 4), (1, 0, 4), (1, 4, 0), (1, 4, -1), (65536, 1, 1), (1, 1, HW_MAX + 1),
              (1, 1024, 2048)):
        assert call(*far, g=g, stride=1 << 32) == E, g
    four = (ctypes.c_void_p * 4)(*[ok] * 4)
    assert pack(None, four, ok, None) == E
    assert pack(four, None, ok, None) == E
    assert pack(four, four, None, None) == E
    assert pack(four, four, ok + 4, None) == E
    for k in range(4):   # a hole in either array
        hole = (ctypes.c_void_p * 4)(*[None if j == k else ok for j in range(4)])
        assert pack(hole, four, ok, None) == E, k
        assert pack(four, hole, ok, None) == E, k
    with pytest.raises(ValueError):
        _lib.check(E, "motion_encoder")


def test_python_interface():
    import eraft_amd
    from eraft_amd import network
    assert callable(eraft_amd.motion_encoder) and "motion_encoder" in eraft_amd.__all__
    sig = inspect.signature(eraft_amd.motion_encoder)
    assert list(sig.parameters) == ["flow", "c1", "enc", "out"] and sig.parameters["out"].default is None
    a = inspect.signature(network.ERAFT.__init__).parameters["hip_motion_encoder"]
    assert a.default is False and a.kind is inspect.Parameter.KEYWORD_ONLY
    cfg = {"subtype": "standard"}
    plain = network.ERAFT(cfg, 3)
    assert not plain.hip_motion_encoder
    net = network.ERAFT(cfg, 3, hip_motion_encoder=True)
    assert net.hip_motion_encoder
    assert list(net.state_dict()) == list(plain.state_dict())   # the same keys
    for kw in ({"fuse_motion_corr": True}, {"hip_upsample": True}, {"hip_gru": True}, {"alternate_corr": True},
               {"fuse_motion_corr": True, "hip_upsample": True, "hip_gru": True},
               {"alternate_corr": True, "hip_gru": True, "hip_upsample": True}):
        assert network.ERAFT(cfg, 3, hip_motion_encoder=True, **kw).hip_motion_encoder
    for kw in ({"mixed_precision": True}, {"differentiable_corr": True}, {"train_motion_corr": True},
               {"train_alternate_corr": True}, {"train_gru": True}):
        with pytest.raises(ValueError, match="hip_motion_encoder"):
            network.ERAFT(cfg, 3, hip_motion_encoder=True, **kw)
    assert network.ERAFT.__doc__.rstrip().endswith("The defaults keep the reference's call pattern exactly.")
    assert "hip_motion_encoder=True" in network.ERAFT.__doc__


def test_cpu_inputs_are_refused():
    """No fallback: a CPU tensor raises, whether or not a device is present."""
    import torch

    import eraft_amd
    from eraft_amd import network
    enc = network.BasicMotionEncoder()
    with torch.no_grad(), pytest.raises(RuntimeError, match="HIP devices"):
        eraft_amd.motion_encoder(torch.zeros(1, 2, 2, 2), torch.zeros(1, 256, 2, 2), enc)
