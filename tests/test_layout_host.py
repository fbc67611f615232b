"""The pyramid addressing helpers of csrc/ecorr_device.h, checked exhaustively on the host: the
slab's first float + the row term + the cell term is pix_off(), and pix_off() is the format written
as nested array indices, for every pixel of every query row
of a slab (interleaved levels 1-3 and a tiled level at 7 x 11, a compact level at 3 x 5; first rows
0, 37, 64, 100 x row counts 1, 27, 64, 200: unaligned slabs and slabs across one and several 64-row
groups), the slab's byte span covers exactly the groups / rows touched, the cell-existence
predicate and the tile-line base agree with their spelled-out forms.  tests/layout_host_check.cpp
is compiled for the host only (no HIP API, no device code) and run; needs hipcc, not a GPU."""
import os
import re
import subprocess

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
HIPCC = "/opt/rocm/bin/hipcc"


def test_addressing_helpers_agree_with_pix_off(tmp_path):
    if not os.path.exists(HIPCC):
        pytest.skip("hipcc not installed")
    exe = str(tmp_path / "layout_host_check")
    subprocess.run([HIPCC, "--offload-host-only", "-x", "hip", "-std=c++17", "-O1",
                    "-I" + os.path.join(ROOT, "e-raft_amd", "csrc"), os.path.join(ROOT, "tests", "layout_host_check.cpp"),
                    "-o", exe], check=True, capture_output=True)
    r = subprocess.run([exe], capture_output=True, text=True)
    assert r.returncode == 0, r.stdout + r.stderr
    m = re.search(r"(\d+) comparisons ok", r.stdout)
    assert m and int(m.group(1)) > 200000, r.stdout
