#!/usr/bin/env python3
"""Are the kernels two source trees have in common the same gfx950 instructions?

    python tools/isa_identity.py [--renamed REGEX=REPL ...] BEFORE_CSRC AFTER_CSRC [file.hip ...] \
        > profiles/<topic>/isa_identity.txt

BEFORE_CSRC / AFTER_CSRC: two copies of e-raft_amd/csrc (each beside its ../../include, e.g. a
`git worktree` of the parent commit and the working tree).  Every listed source (default: all of
AFTER's Makefile SRCS; one absent in BEFORE has only-after kernels) is compiled to assembly with
the flags its own tree's Makefile gives that object (tests/isa_listing.py); per kernel the
instruction stream (no directives, comments or label definitions; the function index in local
labels `.LBB<n>_` dropped, as a kernel added earlier in the file shifts it) and the resource block
(VGPRs, LDS, scratch) are compared.  One line per kernel: identical / DIFFERS / only-before /
only-after, the first differing instruction lines under a DIFFERS line; exit status 1 when a
common kernel differs.  CPU only (hipcc -S).

--renamed REGEX=REPL (repeatable): a kernel of AFTER whose mangled name is absent in BEFORE is
compared with the BEFORE kernel named re.sub(REGEX, REPL, name), when that exists -- for a kernel
whose name changed but whose code must not have, e.g. an instantiation that gained a defaulted
template parameter (`Li0E` appended to its argument list).  The first rule that yields a BEFORE
kernel wins, so specific rules go before general ones.  Such a line names both kernels.
"""
import os
import re
import sys

sys.path.insert(0, os.path.join(os.path.dirname(os.path.dirname(os.path.abspath(__file__))), "tests"))
import isa_listing  # noqa: E402


def main():
    args, renames = sys.argv[1:], []
    while args and args[0] == "--renamed":
        pat, repl = args[1].split("=", 1)
        renames.append((re.compile(pat), repl))
        args = args[2:]
    before, after, only = args[0], args[1], args[2:]
    srcs = only or isa_listing.sources(after)
    B = isa_listing.compile_all(after, srcs)
    A = isa_listing.compile_all(before, [s for s in srcs if os.path.exists(os.path.join(before, s))])   # else: a new file
    bad = 0
    for src in srcs:
        a = isa_listing.kernels(A[src]) if src in A else {}
        b = isa_listing.kernels(B[src])
        was = {}   # AFTER name -> its BEFORE name, for the renamed kernels
        for name in b:
            if name not in a:
                for pat, repl in renames:
                    old = pat.sub(repl, name)
                    if old != name and old in a and old not in b:
                        was[name] = old
                        break
        for name in sorted((set(a) - set(was.values())) | set(b)):
            if name not in b:
                print(f"{src} {name}: only-before")
                continue
            kb, ka = b[name], a.get(was.get(name, name))
            line = f"{src} {name}" + (f" (before: {was[name]})" if name in was else "")
            line += f": {len(kb.ins)} instr, {kb.vgpr} vgpr, {kb.lds} lds, {kb.scratch} scratch, "
            if ka is None:
                print(line + "only-after")
                continue
            same = (ka.ins, ka.vgpr, ka.lds, ka.scratch) == (kb.ins, kb.vgpr, kb.lds, kb.scratch)
            print(line + ("identical" if same else
                          f"DIFFERS (before: {len(ka.ins)} instr, {ka.vgpr} vgpr, {ka.lds} lds, {ka.scratch} scratch)"))
            if not same:
                bad += 1
                n = max(len(ka.ins), len(kb.ins))
                first = next((i for i, (x, y) in enumerate(zip(ka.ins, kb.ins)) if x != y), min(len(ka.ins), len(kb.ins)))
                for i in range(first, min(first + 4, n)):
                    print(f"    [{i}] before: {ka.ins[i] if i < len(ka.ins) else '-'}")
                    print(f"    [{i}] after:  {kb.ins[i] if i < len(kb.ins) else '-'}")
    return 1 if bad else 0


if __name__ == "__main__":
    sys.exit(main())
