"""CPU-side checks of the volume-free correlation entries in the C ABI (ecorr_alt_size,
ecorr_alt_pack_as, ecorr_alt_lookup_as; added within ABI 17): the header declares them, libecorr.so
exports them, _lib registers them, the version is unchanged, and every documented ECORR_EINVAL case
returns it before any GPU call -- the device pointers are null throughout, so nothing can be launched;
the geometry checks, which the three entries share, are exercised through ecorr_alt_size with a real
result pointer."""
import ctypes
import inspect
import os
import subprocess

import pytest

from conftest import ROOT

NAMES = ("ecorr_alt_size", "ecorr_alt_pack_as", "ecorr_alt_lookup_as")


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
    assert "int ecorr_alt_size(int B, int D, int H, int W, int levels, int64_t* floats);" in header
    assert ("int ecorr_alt_pack_as(const void* fmap1, const void* fmap2, int fmap_format, int B, int D, int H, int W,\n"
            "                      int levels, float* feat, void* stream);") in header
    assert ("int ecorr_alt_lookup_as(const float* feat, const float* coords, int B, int D, int H, int W, int levels,\n"
            "                        int radius, void* out, int out_format, void* stream);") in header
    assert "alt.hip" in open(os.path.join(ROOT, "e-raft_amd", "csrc", "Makefile")).read()


def test_size_and_geometry_validation(ea):
    from eraft_amd import _lib
    size, E = ea.lib().ecorr_alt_size, _lib.ECORR_EINVAL
    n = ctypes.c_int64(-1)
    # fmap1 [B][Q][Dp] + the pooled fmap2 levels [B][h_i w_i][Dp], Dp = D rounded up to a multiple of 4
    assert size(2, 37, 17, 21, 4, ctypes.byref(n)) == _lib.ECORR_OK
    assert n.value == 2 * 40 * (17 * 21 + 17 * 21 + 8 * 10 + 4 * 5 + 2 * 2)
    assert size(16, 256, 60, 80, 4, ctypes.byref(n)) == _lib.ECORR_OK
    assert n.value * 4 == 16 * 256 * 4 * (4800 + 4800 + 1200 + 300 + 70)   # 183 MB against the 1.96 GB pyramid
    assert size(1, 8, 8, 32, 4, None) == E                                   # null result pointer
    for bad in ((0, 8, 8, 8, 1), (1, 0, 8, 8, 1), (1, 8, 0, 8, 1), (1, 8, 8, 0, 1), (-1, 8, 8, 8, 1),
                (1, 8, 8, 8, 0), (1, 8, 8, 8, _lib.MAX_LEVELS + 1), (1, 8, 8, 8, -1),
                (1, 8, 8, 32, 5), (1, 8, 4, 4, 4)):                        # a level that pools to 0 pixels
        assert size(*bad, ctypes.byref(n)) == E, bad
    assert size(1, 8, 8, 32, 4, ctypes.byref(n)) == _lib.ECORR_OK            # level 3 is 1 x 4: allowed (NaN samples)
    assert size(1, 8, 1, 1, _lib.MAX_LEVELS, ctypes.byref(n)) == E


def test_pack_and_lookup_validation_before_launch(ea):
    from eraft_amd import _lib
    E = _lib.ECORR_EINVAL
    pack = ea.lib().ecorr_alt_pack_as      # (fmap1, fmap2, fmap_format, B, D, H, W, levels, feat, stream)
    look = ea.lib().ecorr_alt_lookup_as    # (feat, coords, B, D, H, W, levels, radius, out, out_format, stream)
    for fmt in (0, 1, 2, -1, 3, 1 << 20):
        assert pack(None, None, fmt, 1, 8, 8, 8, 1, None, None) == E
        assert look(None, None, 1, 8, 8, 8, 1, 4, None, fmt, None) == E
    for B, D, H, W, L in ((0, 8, 8, 8, 1), (1, 0, 8, 8, 1), (1, 8, 0, 8, 1), (1, 8, 8, 0, 1), (1, 8, 8, 8, 0),
                          (1, 8, 8, 8, 17), (1, 8, 4, 4, 4)):
        assert pack(None, None, 0, B, D, H, W, L, None, None) == E
        assert look(None, None, B, D, H, W, L, 4, None, 0, None) == E
    for radius in (-1, -100):
        assert look(None, None, 1, 8, 8, 8, 1, radius, None, 0, None) == E
    with pytest.raises(ValueError):
        _lib.check(E, "AlternateCorrBlock lookup")


def test_python_interface():
    import eraft_amd
    from eraft_amd import network
    assert "AlternateCorrBlock" in eraft_amd.__all__
    p = inspect.signature(eraft_amd.AlternateCorrBlock.__init__).parameters
    assert (p["num_levels"].default, p["radius"].default, p["fmap_dtype"].default) == (4, 4, None)
    assert p["fmap_dtype"].kind is inspect.Parameter.KEYWORD_ONLY
    assert inspect.signature(eraft_amd.AlternateCorrBlock.__call__).parameters["out_dtype"].default is None
    a = inspect.signature(network.ERAFT.__init__).parameters["alternate_corr"]
    assert a.default is False and a.kind is inspect.Parameter.KEYWORD_ONLY
    cfg = {"subtype": "standard"}
    assert not network.ERAFT(cfg, n_first_channels=3).alternate_corr
    assert network.ERAFT(cfg, n_first_channels=3, alternate_corr=True, mixed_precision=True, hip_upsample=True).alternate_corr
    for kw in ({"fuse_motion_corr": True}, {"train_motion_corr": True}, {"differentiable_corr": True}):
        with pytest.raises(ValueError, match="alternate_corr"):
            network.ERAFT(cfg, n_first_channels=3, alternate_corr=True, **kw)
