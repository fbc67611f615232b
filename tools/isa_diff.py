#!/usr/bin/env python3
"""Kernel-by-kernel comparison of the gfx950 instruction streams of two source trees: every .hip of
the csrc Makefile's SRCS compiled device-only to assembly with that file's Makefile flags, then per
kernel the instruction count, VGPRs (arch + acc), LDS and scratch bytes of tree B, and `identical`
or the first differing instruction lines.  An instruction is a line that starts with a tab and is
neither a directive nor a comment; .LBB<n>_ label numbers are normalised (they count the functions
of the file).  Exit status 1 if any kernel differs.
    python tools/isa_diff.py <tree A> <tree B> [file.hip ...]   # e.g. a worktree of the parent and ."""
import concurrent.futures
import os
import re
import subprocess
import sys
import tempfile


def makefile(csrc):
    """SRCS, the common flags and the per-source extra flags of csrc/Makefile."""
    mk = open(os.path.join(csrc, "Makefile")).read().replace("\\\n", " ")
    var = {k: v.strip() for k, v in re.findall(r"^(\w+)\s*[:?]?=\s*(.*)$", mk, re.M)}
    flags = var["FLAGS"].replace("$(ARCH)", var["ARCH"]).split()
    extra = {s + ".hip": f.split() for s, f in re.findall(r"^build/(\w+)\.o:\s*FLAGS\s*\+=\s*(.*)$", mk, re.M)}
    return var["SRCS"].split(), var["HIPCC"], flags, extra


def kernels(csrc, src, hipcc, flags, out):
    """{kernel: (instruction lines, vgprs, lds bytes, scratch bytes)} of one source file."""
    asm = os.path.join(out, src + ".s")
    subprocess.run([hipcc, *flags, "--cuda-device-only", "-S", src, "-o", asm], cwd=csrc, check=True,
                   stderr=subprocess.DEVNULL)
    s = open(asm).read()
    res = {}
    for m in re.finditer(r"^\t\.amdhsa_kernel (\S+)\n(.*?)^\t\.end_amdhsa_kernel", s, re.M | re.S):
        name, desc = m.group(1), m.group(2)
        start = re.search("^" + re.escape(name) + ":", s, re.M).start()
        body = s[start:s.index(".Lfunc_end", start)]
        ins = [re.sub(r"\.LBB\d+_", ".LBB_", l.strip()) for l in body.splitlines()
               if l.startswith("\t") and not l.strip().startswith((".", ";"))]
        num = {k: int(v) for k, v in re.findall(r"\.amdhsa_(\w+) (\d+)", desc)}
        res[name] = (ins, num["next_free_vgpr"], num["group_segment_fixed_size"], num["private_segment_fixed_size"])
    return res


def tree(root, out, only):
    csrc = os.path.join(root, "e-raft_amd", "csrc")
    srcs, hipcc, flags, extra = makefile(csrc)
    srcs = [s for s in srcs if not only or s in only]
    with concurrent.futures.ThreadPoolExecutor(min(8, os.cpu_count() or 1)) as ex:
        futs = {s: ex.submit(kernels, csrc, s, hipcc, flags + extra.get(s, []), out) for s in srcs}
        return {s: f.result() for s, f in futs.items()}


def main():
    a_root, b_root, only = sys.argv[1], sys.argv[2], sys.argv[3:]
    with tempfile.TemporaryDirectory() as da, tempfile.TemporaryDirectory() as db:
        A, B = tree(a_root, da, only), tree(b_root, db, only)
    ndiff = nk = 0
    for src in sorted(set(A) | set(B)):
        ka, kb = A.get(src, {}), B.get(src, {})
        for name in sorted(set(ka) | set(kb)):
            nk += 1
            if name not in ka or name not in kb:
                ndiff += 1
                print(f"{src} {name}: only in {'B' if name in kb else 'A'}")
                continue
            (ia, *ra), (ib, *rb) = ka[name], kb[name]
            head = f"{src} {name}: {len(ib)} instr, {rb[0]} vgpr, {rb[1]} lds, {rb[2]} scratch"
            if ia == ib and ra == rb:
                print(head + ", identical")
                continue
            ndiff += 1
            print(head + f", DIFFERS (A: {len(ia)} instr, {ra[0]} vgpr, {ra[1]} lds, {ra[2]} scratch)")
            first = next((i for i, (x, y) in enumerate(zip(ia, ib)) if x != y), min(len(ia), len(ib)))
            for i in range(first, min(first + 4, max(len(ia), len(ib)))):
                print(f"    [{i}] A: {ia[i] if i < len(ia) else '-'}")
                print(f"    [{i}] B: {ib[i] if i < len(ib) else '-'}")
    print(f"{nk} kernels, {ndiff} differ")
    sys.exit(1 if ndiff else 0)


if __name__ == "__main__":
    main()
