"""CPU-side checks of the hi-only split build in the C ABI (ecorr_build_split_hi_workspace_size,
ecorr_build_split_pack_hi_as, ecorr_build_split_gemm_hi, ecorr_build_split_hi_as; added within ABI 17):
the symbols exist, the version is unchanged, the hi workspace is the split workspace + 256 bytes, the
header states the bitwise contract, and argument validation returns before any launch (dummy non-null
pointers, no device) with the codes, in the order, of the *_as entries."""
import ctypes
import os
import re
import subprocess

import pytest

from conftest import ROOT

NEW = ("ecorr_build_split_hi_workspace_size", "ecorr_build_split_pack_hi_as", "ecorr_build_split_gemm_hi",
       "ecorr_build_split_hi_as")
P = 256   # a dummy non-null pointer, 256-byte aligned (the workspace's alignment is validated)
BAD_FORMATS = (-1, 3, 16, 1 << 20)


@pytest.fixture(scope="module")
def ea():
    lib = os.path.join(ROOT, "e-raft_amd", "libecorr.so")
    if not os.path.exists(lib):
        subprocess.run(["make", "-s", "-C", os.path.join(ROOT, "e-raft_amd", "csrc")], check=True)
    import eraft_amd
    eraft_amd.lib()
    return eraft_amd


def test_symbols_within_abi_17(ea):
    from eraft_amd import _lib
    L = ea.lib()
    assert L.ecorr_abi_version() == 17 == _lib.ABI_VERSION
    header = open(os.path.join(ROOT, "include", "ecorr.h")).read()
    assert "#define ECORR_ABI_VERSION 17" in header
    for name in NEW:
        assert name in _lib.SYMBOLS, name
        assert getattr(L, name).argtypes == _lib.SYMBOLS[name][1]
        assert re.search(rf"^int {name}\(", header, re.M), name
    # the hi entries take what their plain siblings take
    for hi, plain in (("ecorr_build_split_hi_workspace_size", "ecorr_build_split_workspace_size"),
                      ("ecorr_build_split_pack_hi_as", "ecorr_build_split_pack_as"),
                      ("ecorr_build_split_gemm_hi", "ecorr_build_split_gemm"),
                      ("ecorr_build_split_hi_as", "ecorr_build_split_as")):
        assert _lib.SYMBOLS[hi] == _lib.SYMBOLS[plain], hi
    assert "the pyramid is bitwise that of ecorr_build_split_as on the same inputs" in header


@pytest.mark.parametrize("dims", [(2, 256, 23, 40, 920), (16, 256, 60, 80, 4800), (1, 40, 16, 20, 320),
                                  (2, 256, 23, 40, 120)])
def test_hi_workspace_is_the_split_workspace_plus_256(ea, dims):
    L = ea.lib()
    a, b = ctypes.c_int64(), ctypes.c_int64()
    assert L.ecorr_build_split_workspace_size(*dims, ctypes.byref(a)) == 0
    assert L.ecorr_build_split_hi_workspace_size(*dims, ctypes.byref(b)) == 0
    assert a.value > 0 and b.value == a.value + 256


def test_size_validation(ea):
    from eraft_amd import _lib
    L = ea.lib()
    n = ctypes.c_int64(-7)
    for dims in ((0, 8, 8, 8, 64), (65536, 8, 8, 8, 64), (1, 0, 8, 8, 64), (1, 8, 0, 8, 64), (1, 8, 8, 8, 65),
                 (1, 8, 8, 8, 0)):
        assert L.ecorr_build_split_hi_workspace_size(*dims, ctypes.byref(n)) == _lib.ECORR_EINVAL, dims
        assert n.value == -7   # untouched on failure
    assert L.ecorr_build_split_hi_workspace_size(1, 8, 8, 8, 64, None) == _lib.ECORR_EINVAL


def test_pack_hi_validation_before_launch(ea):
    from eraft_amd import _lib
    L = ea.lib()
    E = _lib.ECORR_EINVAL
    AS = L.ecorr_build_split_pack_as      # (fmap1, fmap2, fmap_format, B, D, H, W, q_count, workspace, stream)
    HI = L.ecorr_build_split_pack_hi_as
    bad = [((None, P), (1, 8, 8, 8, 64), P), ((P, None), (1, 8, 8, 8, 64), P), ((P, P), (1, 8, 8, 8, 64), None),
           ((P, P), (0, 8, 8, 8, 64), P), ((P, P), (1, 0, 8, 8, 64), P), ((P, P), (1, 8, 8, 8, 65), P),
           ((P, P), (1, 8, 8, 8, 0), P), ((P, P), (1, 8, 0, 8, 64), P), ((P, P), (65536, 8, 8, 8, 64), P),
           ((P, P), (1, 8, 8, 8, 64), P + 8)]                         # workspace not 256-byte aligned
    for fm, dims, ws in bad:
        for fmt in (0, 1, 2) + BAD_FORMATS:
            want = AS(*fm, fmt, *dims, ws, None)
            assert want == E
            assert HI(*fm, fmt, *dims, ws, None) == want, (fm, dims, ws, fmt)
    for fmt in BAD_FORMATS:   # an unknown format alone: after every other check, before the memset and the launch
        assert HI(P, P, fmt, 1, 8, 8, 8, 64, P, None) == E
        assert HI(P, P, fmt, 1, 256, 8, 8, 64, P, None) == E


def test_gemm_hi_validation_before_launch(ea):
    from eraft_amd import _lib
    L = ea.lib()
    E = _lib.ECORR_EINVAL
    G = L.ecorr_build_split_gemm        # (B, D, H, W, q_count, levels, pyramid, workspace, stream)
    HI = L.ecorr_build_split_gemm_hi
    bad = [((1, 8, 8, 8, 64, 1), None, P, E), ((1, 8, 8, 8, 64, 1), P, None, E), ((0, 8, 8, 8, 64, 1), P, P, E),
           ((1, 0, 8, 8, 64, 1), P, P, E), ((1, 8, 8, 8, 65, 1), P, P, E),
           ((1, 8, 8, 8, 64, 0), P, P, _lib.ECORR_ELEVELS), ((1, 8, 8, 8, 64, 17), P, P, _lib.ECORR_ELEVELS),
           ((1, 8, 4, 4, 16, 4), P, P, _lib.ECORR_ESHAPE), ((1, 256, 4, 4, 16, 4), P, P, _lib.ECORR_ESHAPE),
           ((1, 8, 8, 8, 64, 1), P, P + 8, E),                       # workspace not 256-byte aligned
           ((1, 8, 8, 8, 64, 1), P + 8, P, E)]                       # pyramid not 16-byte aligned
    for dims, pyr, ws, code in bad:
        assert G(*dims, pyr, ws, None) == code, dims
        assert HI(*dims, pyr, ws, None) == code, dims


def test_build_split_hi_as_validation_before_launch(ea):
    from eraft_amd import _lib
    L = ea.lib()
    E = _lib.ECORR_EINVAL
    AS = L.ecorr_build_split_as   # (fmap1, fmap2, fmap_format, B, D, H, W, q_count, levels, pyramid, workspace, stream)
    HI = L.ecorr_build_split_hi_as
    bad = [((None, P), (1, 8, 8, 8, 64, 1), P, P, E), ((P, P), (1, 8, 8, 8, 64, 1), None, P, E),
           ((P, P), (1, 8, 8, 8, 64, 1), P, None, E), ((P, P), (1, 8, 8, 8, 65, 1), P, P, E),
           ((P, P), (1, 8, 8, 8, 64, 0), P, P, _lib.ECORR_ELEVELS), ((P, P), (1, 8, 8, 8, 64, 17), P, P, _lib.ECORR_ELEVELS),
           ((P, P), (1, 8, 4, 4, 16, 4), P, P, _lib.ECORR_ESHAPE), ((P, P), (1, 256, 4, 4, 16, 4), P, P, _lib.ECORR_ESHAPE),
           ((P, P), (1, 8, 8, 8, 64, 1), P + 8, P, E)]                # pyramid not 16-byte aligned
    for fm, dims, pyr, ws, code in bad:
        for fmt in (0, 1, 2) + BAD_FORMATS:
            assert AS(*fm, fmt, *dims, pyr, ws, None) == code
            assert HI(*fm, fmt, *dims, pyr, ws, None) == code, (fm, dims, fmt)
    for fmt in BAD_FORMATS:
        assert HI(P, P, fmt, 1, 8, 8, 8, 64, 1, P, P, None) == E
        assert HI(P, P, fmt, 1, 256, 8, 8, 64, 1, P, P, None) == E


def test_switch(ea, monkeypatch):
    """ECORR_BUILD_HI in {0, 1}, read once at import beside set_build_hi / build_hi; anything else raises."""
    import importlib.util
    from eraft_amd import _lib
    before = _lib.build_hi()
    assert isinstance(before, bool)
    try:
        _lib.set_build_hi(True)
        assert _lib.build_hi() is True
        _lib.set_build_hi(False)
        assert _lib.build_hi() is False
        for bad in ("1", None, 2, "on"):
            with pytest.raises(ValueError):
                _lib.set_build_hi(bad)
        assert _lib.build_hi() is False
    finally:
        _lib.set_build_hi(before)

    def fresh(value):   # the module's import-time read, on a private copy of the module
        if value is None:
            monkeypatch.delenv("ECORR_BUILD_HI", raising=False)
        else:
            monkeypatch.setenv("ECORR_BUILD_HI", value)
        spec = importlib.util.spec_from_file_location("_lib_env_probe", _lib.__file__)
        m = importlib.util.module_from_spec(spec)
        spec.loader.exec_module(m)
        return m
    assert fresh("1").build_hi() is True
    assert fresh("0").build_hi() is False
    assert fresh(None).build_hi() is (_lib.BUILD_HI_DEFAULT == "1")
    for bad in ("", "2", "true", "01"):
        with pytest.raises(ValueError, match="ECORR_BUILD_HI"):
            fresh(bad)
