#!/usr/bin/env python3
"""Static instruction mix of one kernel in a hipcc -S listing, split at the last MFMA (K loop +
prologue vs epilogue).  usage: tools/isa_count.py build.s build_split_kernelILb1EE"""
import collections
import os
import sys

sys.path.insert(0, os.path.join(os.path.dirname(os.path.dirname(os.path.abspath(__file__))), "tests"))
import isa_listing  # noqa: E402

k = isa_listing.find(open(sys.argv[1]).read(), sys.argv[2])
ins = k.ins
last = max(i for i, l in enumerate(ins) if l.startswith("v_mfma"))


def mix(seq):
    c = collections.Counter()
    for l in seq:
        op = l.split()[0]
        if op.startswith("v_mfma"):
            c["mfma"] += 1
        elif op.startswith("v_"):
            c["valu"] += 1
            c["v:" + op] += 1
        elif op.startswith("ds_"):
            c["ds"] += 1
        elif op.startswith(("buffer_", "global_")):
            c["vmem"] += 1
        elif op.startswith("s_"):
            c["salu"] += 1
    return c


for name, seq in (("loop+prologue", ins[: last + 1]), ("epilogue", ins[last + 1 :])):
    c = mix(seq)
    top = sorted(((v, k) for k, v in c.items() if k.startswith("v:")), reverse=True)[:14]
    print(f"{name}: {len(seq)} instr, mfma {c['mfma']} valu {c['valu']} ds {c['ds']} vmem {c['vmem']} salu {c['salu']}")
    print("   " + ", ".join(f"{k[2:]} {v}" for v, k in top))
for f in ("vgpr_count", "agpr_count", "sgpr_count", "private_segment_fixed_size", "vgpr_spill_count", "sgpr_spill_count"):
    print(f, k.meta[f])
