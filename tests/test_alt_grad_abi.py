"""CPU-side checks of the volume-free lookup's backward in the C ABI (ecorr_alt_backward_workspace_size,
ecorr_alt_lookup_backward, ecorr_alt_pack_backward; added within ABI 17) and of its Python opt-ins: the
header declares the entries, libecorr.so exports them, _lib registers them, the version is unchanged,
and every documented ECORR_EINVAL case returns it before any GPU call -- the device pointers are null
or fake throughout, so nothing can be launched."""
import ctypes
import inspect
import os
import subprocess

import pytest

from conftest import ROOT

NAMES = ("ecorr_alt_backward_workspace_size", "ecorr_alt_lookup_backward", "ecorr_alt_pack_backward")


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
    assert "int ecorr_alt_backward_workspace_size(int B, int H, int W, int levels, int radius, int64_t* bytes);" in header
    assert ("int ecorr_alt_lookup_backward(const float* feat, const float* coords, const float* grad_out, int B, int D,\n"
            "                              int H, int W, int levels, int radius, float* grad_feat, void* workspace, "
            "void* stream);") in header
    assert ("int ecorr_alt_pack_backward(float* grad_feat, int B, int D, int H, int W, int levels,\n"
            "                            float* grad_fmap1, float* grad_fmap2, void* stream);") in header
    assert "alt_grad.hip" in open(os.path.join(ROOT, "e-raft_amd", "csrc", "Makefile")).read().split("SRCS")[1].split("\n")[0]


def test_workspace_size(ea):
    from eraft_amd import _lib
    size, E = ea.lib().ecorr_alt_backward_workspace_size, _lib.ECORR_EINVAL

    def ws(B, H, W, L, r):
        n = ctypes.c_int64(-1)
        assert size(B, H, W, L, r, ctypes.byref(n)) == _lib.ECORR_OK
        return n.value

    # per (batch item, level, query): two ints of origin and (2r+3)^2 floats of window
    assert ws(2, 17, 21, 4, 4) == 2 * 4 * 17 * 21 * (8 + 4 * 121)
    assert ws(16, 60, 80, 4, 4) == 16 * 4 * 4800 * (8 + 4 * 121)   # DSEC B = 16: 151 MB
    assert ws(1, 8, 8, 1, 0) == 64 * (8 + 4 * 9) > 0
    base = ws(2, 16, 24, 2, 2)
    assert base > 0
    assert ws(3, 16, 24, 2, 2) > base and ws(2, 16, 24, 3, 2) > base and ws(2, 16, 24, 2, 3) > base
    assert ws(1, 16, 16, 2, 32) == 2 * 256 * (8 + 4 * 67 * 67)     # every radius of ecorr_lookup_backward
    n = ctypes.c_int64(-1)
    assert size(1, 8, 8, 1, 4, None) == E
    for bad in ((0, 8, 8, 1, 4), (-1, 8, 8, 1, 4), (1, 0, 8, 1, 4), (1, 8, 0, 1, 4), (1, 8, 8, 0, 4),
                (1, 8, 8, _lib.MAX_LEVELS + 1, 4), (1, 4, 4, 4, 4), (1, 8, 8, 1, -1), (1, 8, 8, 1, 33)):
        assert size(*bad, ctypes.byref(n)) == E, bad


def test_validation_before_launch(ea):
    from eraft_amd import _lib
    E = _lib.ECORR_EINVAL
    # (feat, coords, grad_out, B, D, H, W, levels, radius, grad_feat, workspace, stream)
    look = ea.lib().ecorr_alt_lookup_backward
    # (grad_feat, B, D, H, W, levels, grad_fmap1, grad_fmap2, stream)
    pack = ea.lib().ecorr_alt_pack_backward
    ok = 4096          # a fake, 16-byte aligned device address: never dereferenced on the host, and every
    geom = (1, 8, 8, 8, 1)   # call below fails its validation before a launch
    assert look(None, None, None, *geom, 4, None, None, None) == E
    for i in range(5):   # each pointer null in turn, the others fake
        ptrs = [ok] * 5
        ptrs[i] = None
        feat, coords, go, gf, ws = ptrs
        assert look(feat, coords, go, *geom, 4, gf, ws, None) == E, i
    for i in (0, 3, 4):   # feat, grad_feat and the workspace misaligned in turn
        ptrs = [ok] * 5
        ptrs[i] = ok + 4
        feat, coords, go, gf, ws = ptrs
        assert look(feat, coords, go, *geom, 4, gf, ws, None) == E, i
    for radius in (-1, -100, 33):
        assert look(ok, ok, ok, *geom, radius, ok, ok, None) == E
    for B, D, H, W, L in ((0, 8, 8, 8, 1), (1, 0, 8, 8, 1), (1, 8, 0, 8, 1), (1, 8, 8, 0, 1), (1, 8, 8, 8, 0),
                          (1, 8, 8, 8, 17), (1, 8, 4, 4, 4)):
        assert look(ok, ok, ok, B, D, H, W, L, 4, ok, ok, None) == E
        assert pack(ok, B, D, H, W, L, ok, ok, None) == E
    assert pack(None, *geom, ok, ok, None) == E
    assert pack(ok + 4, *geom, ok, ok, None) == E
    with pytest.raises(ValueError):
        _lib.check(E, "AlternateCorrBlock lookup backward")


def test_python_interface():
    import eraft_amd
    from eraft_amd import network
    p = inspect.signature(eraft_amd.AlternateCorrBlock.__init__).parameters
    assert p["trainable"].default is False and p["trainable"].kind is inspect.Parameter.KEYWORD_ONLY
    assert p["differentiable"].default is False
    a = inspect.signature(network.ERAFT.__init__).parameters["train_alternate_corr"]
    assert a.default is False and a.kind is inspect.Parameter.KEYWORD_ONLY
    cfg = {"subtype": "standard"}
    assert not network.ERAFT(cfg, 3).train_alternate_corr
    net = network.ERAFT(cfg, 3, train_alternate_corr=True)
    assert net.alternate_corr and net.train_alternate_corr
    assert network.ERAFT(cfg, 3, train_alternate_corr=True, mixed_precision=True, hip_upsample=True).alternate_corr
    plain = network.ERAFT(cfg, 3, alternate_corr=True)
    assert plain.alternate_corr and not plain.train_alternate_corr
    for kw in ({"fuse_motion_corr": True}, {"train_motion_corr": True}, {"differentiable_corr": True}):
        with pytest.raises(ValueError, match="train_alternate_corr"):
            network.ERAFT(cfg, 3, train_alternate_corr=True, **kw)
        with pytest.raises(ValueError, match="alternate_corr"):
            network.ERAFT(cfg, 3, alternate_corr=True, **kw)
