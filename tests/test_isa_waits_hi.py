"""CPU guard of the hi-only split GEMM's hand-counted waits (e-raft_amd/csrc/build_hi.hip).

build_split16_hi_kernel<MUL, 1> runs build_split16_kernel's K loop on one MFMA per product: the same
four-buffer ring, one barrier per chunk pair and static `s_waitcnt vmcnt(N)` waits, with 2 LDS-DMA
pieces per wave and pair (the hi KB of two 16-target groups) and 4 query fragment loads -- the counts
s16_vm_after(j, 2, 4) of build_split16.h.  This test compiles build_hi.hip for gfx950 with the
Makefile's flags and replays the one-term kernel's emitted instruction order with the checker of
tests/test_isa_waits.py (RAW at every barrier, WAR on every refill, LDS read offsets per barrier
region); the three-term kernel of the pair is replayed with build_split16_kernel's parameters.
From the assembly's kernel descriptors: no scratch, no spilled VGPRs, and at most 256 VGPRs and
the parent's LDS -- the two blocks per CU the kernels are launched for (__launch_bounds__(256, 2)).
MFMA counts: 256 in the one-term kernel, 768 in the three-term kernel (the two-kernel form)."""
import os
import re
import subprocess
import tempfile

import pytest

from test_isa_waits import CSRC, HIPCC, ROOT, check_loop, is_dma, is_vmem, kernel_loop

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
    if not os.path.exists(HIPCC):
        pytest.skip("hipcc not installed")
    with tempfile.TemporaryDirectory() as d:
        out = os.path.join(d, "build_hi.s")
        subprocess.run([HIPCC, "--offload-arch=gfx950", "-O3", "-std=c++17", "-ffp-contract=off",
                        "-I" + os.path.join(ROOT, "include"), "--cuda-device-only", "-S",
                        os.path.join(CSRC, "build_hi.hip"), "-o", out],
                       check=True, capture_output=True)
        return open(out).read()


def test_makefile_builds_it_with_these_flags():
    mk = open(os.path.join(CSRC, "Makefile")).read()
    assert re.search(r"^SRCS\s*:=.*\bbuild_hi\.hip\b", mk, re.M)
    assert not re.search(r"build_hi\.o:\s*FLAGS", mk)   # no per-file flags: what this test compiles is what ships


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
    ins = kernel_loop(asm, ONE)
    first = next(i for i, ln in enumerate(ins) if is_dma(ln))
    q = [i for i, ln in enumerate(ins) if i > first and is_vmem(ln) and not is_dma(ln)][:4]
    swapped = ins[:first] + [ins[i] for i in q] + [ln for i, ln in enumerate(ins[first:], first) if i not in q]
    errs = check_loop(swapped, 4, 2, 8, 16384, True, 2)
    assert any(e.startswith("barrier 0:") for e in errs), errs


@pytest.mark.parametrize("name", ["build_split16_hi_kernelILb1ELi1EE", "build_split16_hi_kernelILb0ELi1EE",
                                  "build_split16_hi_kernelILb1ELi3EE", "build_split16_hi_kernelILb0ELi3EE"])
def test_resources_keep_two_blocks_per_cu(asm, name):
    m = re.search(r"^(_Z\S*" + re.escape(name) + r"\S*):", asm, re.M)
    assert m, f"{name} not in the listing"
    mangled = m.group(1)
    # the kernel's metadata record (amdhsa.kernels: YAML, one `- .agpr_count` .. record per kernel)
    records = re.split(r"\n  - \.", asm[asm.index("amdhsa.kernels:"):])
    rec = next(r for r in records if re.search(r"\.name:\s+" + re.escape(mangled) + r"\n", r))

    def field(f):
        return int(re.search(r"\." + f + r":\s+(\d+)", rec).group(1))
    assert field("private_segment_fixed_size") == 0                    # no scratch
    assert field("vgpr_spill_count") == 0 and field("sgpr_spill_count") == 0
    assert field("vgpr_count") <= 256                                   # two waves per SIMD of 512 registers
    assert field("group_segment_fixed_size") <= LDS_PARENT              # two blocks in a CU's 160 KB
    assert field("max_flat_workgroup_size") == 256
    # the compiler's own account behind the kernel's code
    occ = re.search(r"; Occupancy: (\d+)", asm[asm.index(".Lfunc_end", m.start()):])
    assert int(occ.group(1)) == 2   # waves per SIMD = blocks per CU for 256-thread blocks
