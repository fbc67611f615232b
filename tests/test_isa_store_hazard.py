"""CPU guard of the store-data hazard behind round 3's lost level-0 stores (VERDICT r4 item 3,
DESIGN.md §3.1 "Stores and soffset").

Root cause (round 5, tools/soff_repro.py + tools/soff_lab.hip on the GPU): a buffer store of more
than 8 bytes reads its data VGPRs after it issues; a VALU that overwrites them in the next cycle
needs one wait state.  hipcc (LLVM's GCNHazardRecognizer) inserts it only when the store's soffset is
NOT a register -- with the wave-uniform row term in an SGPR soffset it emitted
`buffer_store_dwordx4 v[174:177], ..., s65 offen nt` followed at once by `v_cndmask_b32 v174, 0, 1`,
and that store wrote the integer 1 (1.4e-45) instead of the value: 192 elements of 20 query rows of a
B = 16 build, every element still written (the round-3 diagnosis read it as unwritten rows).  With the
term in the voffset (soffset = 0) the pad is there and every build is bitwise.  The range check
(tools/soff_lab.hip): an access happens iff voffset < num_records and voffset + soffset <
num_records, so soffset itself is safe wherever both stay in range (the split16 / conv LDS-DMA and
query loads) -- the hazard is the store-data one only.

This test compiles every kernel source for gfx950 and requires that no wide (dwordx3/x4) buffer
store takes its soffset from an SGPR; the detector itself is checked on the round-3 variant
(tools/lab_build.py soff_full), where it must find the hazard."""
import concurrent.futures
import os
import re
import shutil
import sys
import tempfile

import pytest

import isa_listing
from test_isa_waits import CSRC, HIPCC, ROOT

SOURCES = isa_listing.sources(CSRC)   # every source of libecorr.so
WIDE = re.compile(r"buffer_store_(?:dwordx3|dwordx4|b96|b128)\s+v\[(\d+):(\d+)\],\s*\S+,\s*s\[\d+:\d+\],\s*(\S+)")
VDST = re.compile(r"v_\S+\s+v(?:\[(\d+):(\d+)\]|(\d+))\b")


def _ins(text):
    """Every instruction line of a listing, in file order."""
    return isa_listing.instructions(text.splitlines())


def scan(ins):
    """(wide stores with an SGPR soffset, of which immediately followed by a VALU writing their data)."""
    sgpr, hazards = [], []
    for i, l in enumerate(ins):
        m = WIDE.match(l)
        if not m or not re.fullmatch(r"s\d+", m.group(3)):
            continue
        sgpr.append(l)
        lo, hi = int(m.group(1)), int(m.group(2))
        w = VDST.match(ins[i + 1]) if i + 1 < len(ins) else None
        if w:
            a = int(w.group(1) or w.group(3))
            b = int(w.group(2) or w.group(3))
            if not (b < lo or a > hi):
                hazards.append(l + " || " + ins[i + 1])
    return sgpr, hazards


@pytest.fixture(scope="module")
def compiled():
    if not os.path.exists(HIPCC):
        pytest.skip("hipcc not installed")
    sys.path.insert(0, os.path.join(ROOT, "tools"))
    import lab_build
    d = tempfile.mkdtemp()
    try:
        bad = os.path.join(d, "e-raft_amd", "csrc")   # the tree's layout: the sources include ../../include
        shutil.copytree(CSRC, bad, ignore=shutil.ignore_patterns("build"))
        shutil.copytree(os.path.join(ROOT, "include"), os.path.join(d, "include"))
        for fname, old, new in lab_build.PATCHES["soff_full"]:   # each patch in the file it names
            p = os.path.join(bad, fname)
            s = open(p).read()
            assert old in s
            open(p, "w").write(s.replace(old, new))
        with concurrent.futures.ThreadPoolExecutor(1) as ex:   # the variant beside the tree's sources
            soff = ex.submit(isa_listing.listing, bad, "build.hip")
            res = {n: _ins(t) for n, t in isa_listing.compile_all(CSRC, SOURCES).items()}
            res["soff_full"] = _ins(soff.result())
        yield res
    finally:
        shutil.rmtree(d, ignore_errors=True)


def test_no_wide_store_with_sgpr_soffset(compiled):
    assert "build.hip" in SOURCES and "grad.hip" in SOURCES, f"SRCS of the Makefile not read: {SOURCES}"
    for n in SOURCES:
        sgpr, hazards = scan(compiled[n])
        assert not sgpr, f"{n}: wide buffer stores with an SGPR soffset: {sgpr[:3]}"


def test_detector_finds_round3_variant(compiled):
    sgpr, hazards = scan(compiled["soff_full"])
    assert sgpr and hazards, "the soffset FULL epilogue should show the unpadded store-data hazard"
