#!/usr/bin/env python3
"""Are the kernels two source trees have in common the same gfx950 instructions?

    python tools/isa_identity.py [--renamed REGEX=REPL ...] BEFORE_CSRC AFTER_CSRC [file.hip ...] \
        > profiles/<topic>/isa_identity.txt

BEFORE_CSRC / AFTER_CSRC: two copies of e-raft_amd/csrc (each beside its ../../include, e.g. a
`git worktree` of the parent commit and the working tree).  Every listed source (default: all of
AFTER's Makefile SRCS; one absent in BEFORE has only-after kernels) is compiled with the Makefile's
code-generation flags to assembly; per kernel the instruction stream (no directives, comments or label definitions; the function index
in local labels `.LBB<n>_` dropped, as a kernel added earlier in the file shifts it) and the
resource block (VGPRs, LDS, scratch) are compared.  One line per kernel: identical / DIFFERS /
only-before / only-after; exit status 1 when a common kernel differs.  CPU only (hipcc -S).

--renamed REGEX=REPL (repeatable): a kernel of AFTER whose mangled name is absent in BEFORE is
compared with the BEFORE kernel named re.sub(REGEX, REPL, name), when that exists -- for a kernel
whose name changed but whose code must not have, e.g. an instantiation that gained a defaulted
template parameter (`Li0E` appended to its argument list).  Such a line names both kernels.
"""
import os
import re
import subprocess
import sys
import tempfile

HIPCC = os.environ.get("HIPCC", "/opt/rocm/bin/hipcc")


def sources(csrc):
    m = re.search(r"^SRCS\s*:=\s*(.*)$", open(os.path.join(csrc, "Makefile")).read(), re.M)
    return m.group(1).split()


def kernels(csrc, src, tmp):
    out = os.path.join(tmp, src + ".s")
    flags = ["-fno-slp-vectorize"] if src == "build.hip" else []
    subprocess.run([HIPCC, "--offload-arch=gfx950", "-O3", "-std=c++17", "-ffp-contract=off", *flags,
                    "-I" + os.path.join(csrc, "..", "..", "include"), "--cuda-device-only", "-S",
                    os.path.join(csrc, src), "-o", out], check=True, capture_output=True)
    s = open(out).read()
    res = {}
    for m in re.finditer(r"^(_Z\S+):\s*; @\S+\n(.*?)^\.Lfunc_end\d+:", s, re.M | re.S):
        name, body = m.group(1), m.group(2)
        if f".amdhsa_kernel {name}\n" not in s:
            continue   # a device function, not a kernel
        ins = [re.sub(r"\.LBB\d+_", ".LBB_", ln.split(";")[0].strip()) for ln in body.splitlines()
               if ln.startswith("\t") and not ln.strip().startswith((".", ";"))]
        k = s[s.index(f".amdhsa_kernel {name}\n"):]
        k = k[:k.index(".end_amdhsa_kernel")]

        def field(f):
            return int(re.search(r"\." + f + r"\s+(\d+)", k).group(1))
        res[name] = (ins, field("amdhsa_next_free_vgpr"), field("amdhsa_group_segment_fixed_size"),
                     field("amdhsa_private_segment_fixed_size"))
    return res


def main():
    args, renames = sys.argv[1:], []
    while args and args[0] == "--renamed":
        pat, repl = args[1].split("=", 1)
        renames.append((re.compile(pat), repl))
        args = args[2:]
    before, after, only = args[0], args[1], args[2:]
    srcs = only or sources(after)
    bad = 0
    with tempfile.TemporaryDirectory() as ta, tempfile.TemporaryDirectory() as tb:
        for src in srcs:
            a = kernels(before, src, ta) if os.path.exists(os.path.join(before, src)) else {}   # a new file
            b = kernels(after, src, tb)
            was = {}   # AFTER name -> its BEFORE name, for the renamed kernels
            for name in b:
                if name not in a:
                    for pat, repl in renames:
                        old = pat.sub(repl, name)
                        if old != name and old in a and old not in b:
                            was[name] = old
                            break
            for name in sorted((set(a) - set(was.values())) | set(b)):
                if name in was:
                    ins, v, l, sc = b[name]
                    same = a[was[name]] == b[name]
                    bad += not same
                    print(f"{src} {name} (before: {was[name]}): {len(ins)} instr, {v} vgpr, {l} lds, {sc} scratch, "
                          + ("identical" if same else "DIFFERS"))
                elif name not in b:
                    print(f"{src} {name}: only-before")
                elif name not in a:
                    ins, v, l, sc = b[name]
                    print(f"{src} {name}: {len(ins)} instr, {v} vgpr, {l} lds, {sc} scratch, only-after")
                else:
                    ins, v, l, sc = b[name]
                    same = a[name] == b[name]
                    bad += not same
                    print(f"{src} {name}: {len(ins)} instr, {v} vgpr, {l} lds, {sc} scratch, "
                          + ("identical" if same else "DIFFERS"))
    return 1 if bad else 0


if __name__ == "__main__":
    sys.exit(main())
