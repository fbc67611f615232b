"""CPU: the Python mirrors of the splat's and the voxel grid's dispatch (tests/splat_cases.py,
tests/voxel_dispatch.py) against the kernels' sources, and the cases against the mirrors.

The thresholds the mirrors restate are read from csrc/splat.hip and csrc/voxel.hip: a retune of one
fails here instead of silently moving a GPU test case onto another branch.  Every case takes the
branches it is there for, and every branch of the two BRANCHES lists has a case.
"""
import os
import re

import pytest

import splat_cases as sc
import voxel_dispatch as vd

CSRC = os.path.join(os.path.dirname(os.path.abspath(__file__)), "..", "e-raft_amd", "csrc")


def constant(src, name):
    """The value of `constexpr <type> ... name = <integer expression>` in src; the expression may use
    other such constants of the file."""
    m = re.search(r"constexpr\s+\w+\s+(?:\w+\s*=[^,;]+,\s*)*%s\s*=\s*([^,;]+)[,;]" % re.escape(name), src)
    assert m, f"no constexpr {name}"
    expr = m.group(1).strip()
    assert re.fullmatch(r"[\w\s()+\-*/]+", expr), f"{name} = {expr!r}: not an integer expression"
    for ident in set(re.findall(r"[A-Za-z_]\w*", expr)):
        expr = re.sub(r"\b%s\b" % ident, str(constant(src, ident)), expr)
    return int(eval(expr.replace("/", "//"), {"__builtins__": {}}))


@pytest.mark.parametrize("name", ["kBandMaxN", "kBandPts", "kBandCap", "kBandTargets", "kLdsTargets"])
def test_splat_constants_match_source(name):
    src = open(os.path.join(CSRC, "splat.hip")).read()
    assert getattr(sc, name) == constant(src, name)


@pytest.mark.parametrize("name", ["VB_TY", "VB_TX", "VB_MAXNB", "VB_MAXRUN", "VB_CAP", "VB_EPB", "kGatherBlocks",
                                  "VB_WK"])
def test_voxel_constants_match_source(name):
    src = open(os.path.join(CSRC, "voxel.hip")).read()
    assert getattr(vd, name) == constant(src, name)


def test_constant_reader():
    src = "constexpr int A = 4, B = 16;\nconstexpr int64_t C = (A + 1) * B;   // c\nconstexpr int D = 8 * C / 3, E = D;"
    assert [constant(src, n) for n in "ABCDE"] == [4, 16, 80, 213, 213]
    with pytest.raises(AssertionError):
        constant(src, "F")


@pytest.mark.parametrize("name", list(sc.CASES))
def test_splat_case_takes_its_branches(name):
    want, got = sc.CASES[name]["expect"], sc.tags(name)
    assert want <= set(sc.BRANCHES) and want <= got, f"{name}: expected {sorted(want)}, the mirror says {sorted(got)}"
    assert sc.workspace_needed(sc.CASES[name]["n"]) == any(t.startswith("large.") for t in got)


@pytest.mark.parametrize("name", list(vd.CASES))
def test_voxel_case_takes_its_branches(name):
    want, got = vd.CASES[name]["expect"], vd.tags(name)
    assert want <= set(vd.BRANCHES) and want <= got, f"{name}: expected {sorted(want)}, the mirror says {sorted(got)}"


def test_every_branch_has_a_case():
    for mod in (sc, vd):
        covered = set().union(*(c["expect"] for c in mod.CASES.values()))
        assert covered == set(mod.BRANCHES), f"{mod.__name__}: no case for {sorted(set(mod.BRANCHES) - covered)}"


def test_tile_count_boundary_cases():
    """The two tile-count cases sit on either side of VB_MAXNB, the two C cases of the suite on either
    side of the run table (test_voxel_gpu's C = 23 / 24), the splat pairs on either side of their switches."""
    assert vd.tiles(384, 2048)[2] == vd.VB_MAXNB and vd.path(True, 40_000, 2, 384, 2048) == ("tiled", None)
    assert vd.tiles(385, 2048)[2] > vd.VB_MAXNB and vd.path(True, 40_000, 2, 385, 2048) == ("key_range", "nb")
    assert vd.path(True, 20_000, 23, 13, 37) == ("tiled", None) and vd.path(True, 20_000, 24, 13, 37) == ("key_range", "C")
    assert vd.tiles(720, 1280)[2] == 14400
    assert vd.gather_blocks(24, 100) == (2048, 2) and vd.gather_blocks(15, 260) == (2048, 2)
    assert sc.kernel(65_536) == "band" and sc.kernel(65_537) == "large"
    assert sc.staged(True, 5_120) and not sc.staged(True, 5_121) and not sc.staged(True, 5_135)
    assert sc.counts(15_000) == "lds" and sc.counts(16_384) == "lds" and sc.counts(18_000) == "ws"
    assert [sc.staging(True, 63, b) for b in range(3)] == ["aligned", "scalar", "aligned"]
