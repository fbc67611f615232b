"""CPU guard of the hi-only split GEMM's hand-counted waits (e-raft_amd/csrc/build_hi.hip).

build_split16_hi_kernel<MUL, 1> runs build_split16_kernel's K loop on one MFMA per product: the same
four-buffer ring, one barrier per chunk pair and static `s_waitcnt vmcnt(N)` waits, with 2 LDS-DMA
pieces per wave and pair (the hi KB of two 16-target groups) and 4 query fragment loads -- the counts
s16_vm_after(j, 2, 4) of build_split16.h.  This test takes build_hi.hip's gfx950 listing
(isa_listing.py: what the Makefile gives each object, checked below for every source) and replays
the one-term kernel's emitted instruction order with the checker of tests/test_isa_waits.py (RAW
at every barrier, WAR on every refill, LDS read offsets per barrier region); the three-term kernel of the pair is replayed with build_split16_kernel's parameters.
From the assembly's kernel descriptors: no scratch, no spilled VGPRs, and at most 256 VGPRs and
the parent's LDS -- the two blocks per CU the kernels are launched for (__launch_bounds__(256, 2)).
MFMA counts: 256 in the one-term kernel, 768 in the three-term kernel (the two-kernel form)."""
import re

import pytest

import isa_listing
from test_isa_waits import CSRC, check_loop, hoist_query_loads, is_dma, kernel_loop, listing

ONE = "build_split16_hi_kernelILb1ELi1EE"
ONE_DIV = "build_split16_hi_kernelILb0ELi1EE"
THREE = "build_split16_hi_kernelILb1ELi3EE"
# LDS buffers, DMA pieces per pair, chunk pairs, bytes per buffer, query loads per pair, barriers a
# pair's reads span, barriers up to the loop's closing one
LOOPS = {
    ONE: dict(nbuf=4, copies=2, nk=8, chunk=16384, qloads=4, span=2, barriers=9, mfma=256),
    ONE_DIV: dict(nbuf=4, copies=2, nk=8, chunk=16384, qloads=4, span=2, barriers=9, mfma=256),
    THREE: dict(nbuf=4, copies=4, nk=8, chunk=16384, qloads=8, span=2, barriers=9, mfma=768),
}
LDS_PARENT = 75776   # build_split16_kernel's LDS (TILE_LDS): two blocks fit a CU's 160 KB


@pytest.fixture(scope="module")
def asm():
    return listing("build_hi.hip")


def test_listings_are_compiled_with_each_objects_flags():
    """Every source's listing command is its object's `make -n` line but for `-c` -> device-only `-S`
    and the output; -fno-slp-vectorize is build.hip's alone."""
    srcs = isa_listing.sources(CSRC)
    assert "build.hip" in srcs and "build_hi.hip" in srcs and "conv.hip" in srcs
    for src in srcs:
        obj = isa_listing.object_command(CSRC, src)
        cmd = isa_listing.compile_command(CSRC, src, "out.s")
        assert obj.count("-c") == 1 and obj[-2] == "-o" and src in obj
        flags = [a for a in obj[:-2] if a not in ("-c", src)]
        assert [a for a in cmd[:-2] if a not in ("--cuda-device-only", "-S", src)] == flags
        assert cmd[-2:] == ["-o", "out.s"] and "-c" not in cmd and "-S" in cmd and "--cuda-device-only" in cmd
        assert {"--offload-arch=gfx950", "-O3", "-ffp-contract=off"} <= set(flags)
        assert ("-fno-slp-vectorize" in flags) == (src == "build.hip")


@pytest.mark.parametrize("name", sorted(LOOPS))
def test_static_waits_match_issue_order(asm, name):
    k = LOOPS[name]
    ins = kernel_loop(asm, name)
    assert sum(1 for ln in ins if ln == "s_barrier") == k["barriers"]
    assert sum(1 for ln in ins if is_dma(ln)) == k["copies"] * k["nk"]
    assert sum(1 for ln in ins if ln.startswith("buffer_load") and not is_dma(ln)) == k["qloads"] * k["nk"]
    assert sum(1 for ln in ins if ln.startswith("v_mfma_f32_16x16x32_f16")) == k["mfma"]
    errs = check_loop(ins, k["nbuf"], k["copies"], k["nk"], k["chunk"], True, k["span"])
    assert not errs, "\n".join(errs)


def test_one_term_waits_are_the_hand_checked_counts(asm):
    """The vmcnt of the nine waits in front of the barriers: s16_vm_after(j, 2, 4), j = 0 .. 7."""
    ins = kernel_loop(asm, ONE)
    waits = []
    for i, ln in enumerate(ins):
        if ln == "s_barrier" and len(waits) < 8:
            w = next(x for x in reversed(ins[:i]) if x.startswith("s_waitcnt") and "vmcnt" in x)
            waits.append(int(re.search(r"vmcnt\((\d+)\)", w).group(1)))
    assert waits == [8, 10, 14, 10, 10, 10, 10, 8]


def test_checker_flags_the_three_term_counts_on_the_one_term_stream(asm):
    """The waits are not slack: with the three-term loop's larger counts the one-term stream races."""
    ins = [re.sub(r"vmcnt\((\d+)\)", lambda m: f"vmcnt({2 * int(m.group(1))})", ln) if ln.startswith("s_waitcnt") else ln
           for ln in kernel_loop(asm, ONE)]
    errs = check_loop(ins, 4, 2, 8, 16384, True, 2)
    assert any("DMA may be in flight" in e for e in errs), errs
    # and a hoisted q(0), as for the parent kernel
    errs = check_loop(hoist_query_loads(kernel_loop(asm, ONE), 4), 4, 2, 8, 16384, True, 2)
    assert any(e.startswith("barrier 0:") for e in errs), errs


@pytest.mark.parametrize("name", ["build_split16_hi_kernelILb1ELi1EE", "build_split16_hi_kernelILb0ELi1EE",
                                  "build_split16_hi_kernelILb1ELi3EE", "build_split16_hi_kernelILb0ELi3EE"])
def test_resources_keep_two_blocks_per_cu(asm, name):
    k = isa_listing.find(asm, name)
    field = k.meta.__getitem__   # the kernel's amdhsa.kernels metadata record
    assert field("private_segment_fixed_size") == 0                    # no scratch
    assert field("vgpr_spill_count") == 0 and field("sgpr_spill_count") == 0
    assert field("vgpr_count") <= 256                                   # two waves per SIMD of 512 registers
    assert field("group_segment_fixed_size") <= LDS_PARENT              # two blocks in a CU's 160 KB
    assert field("max_flat_workgroup_size") == 256
    # the compiler's own account behind the kernel's code
    assert k.occupancy == 2   # waves per SIMD = blocks per CU for 256-thread blocks
