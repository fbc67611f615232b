#!/usr/bin/env python3
"""csrc/grad.hip on the CPU: the kernel source itself (one textual substitution: the dynamic LDS
declaration) and the headers it includes, csrc/mfma_f32_frame.h among them, compiled as C++ against
tools/grad_emul/shim (one host thread per GPU thread; it maps the MFMA accumulator's ext_vector_type
onto g++'s vector_size) with AddressSanitizer + UBSan, run as a stand-alone program on a case of
tests/backward_cases.py and compared with the reference's gradients (tests/golden/backward_*.npz).
For finding an out-of-bounds access or a wrong index without a GPU; it says nothing about speed.
    python tools/grad_emul.py d3_l3r1 [y0 y1]      # optional query-row slab
"""
import os
import re
import subprocess
import sys
import tempfile

import numpy as np
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
for p in (ROOT, os.path.join(ROOT, "tests")):
    sys.path.insert(0, p)
import backward_cases as bc  # noqa: E402

CSRC = os.path.join(ROOT, "e-raft_amd", "csrc")
EMUL = os.path.join(ROOT, "tools", "grad_emul")


def nw(a, b):
    return float(np.abs(a.astype(np.float64) - b).max() / np.sqrt((b.astype(np.float64) ** 2).mean()))


def main():
    case = sys.argv[1]
    B, D, H, W, L, r, _ = bc.CASES[case]
    y0, y1 = (int(sys.argv[2]), int(sys.argv[3])) if len(sys.argv) > 3 else (0, H)
    q = (y1 - y0) * W
    with tempfile.TemporaryDirectory() as d:
        src = open(os.path.join(CSRC, "grad.hip")).read()
        src, n1 = re.subn(r"extern __shared__ float lds\[\];", "float* lds = g_dynlds;", src)
        assert n1 == 1
        open(os.path.join(d, "grad_emul.cpp"), "w").write(src)
        exe = os.path.join(d, "emul")
        subprocess.run(["g++", "-std=c++20", "-O1", "-g", "-fsanitize=address,undefined", "-ffp-contract=off",
                        "-pthread", "-w", "-I" + os.path.join(EMUL, "shim"), "-I" + os.path.join(ROOT, "include"),
                        "-I" + CSRC, "-x", "c++", os.path.join(d, "grad_emul.cpp"), os.path.join(CSRC, "abi.hip"),
                        os.path.join(EMUL, "main.cpp"), "-o", exe, "-Wl,--unresolved-symbols=ignore-all"], check=True)
        f1, f2 = bc.fmaps(case)
        np.ascontiguousarray(f1[:, :, y0:y1]).tofile(os.path.join(d, "f1.bin"))
        f2.tofile(os.path.join(d, "f2.bin"))
        looks = bc.lookups(case)
        for i, (_, c, gs) in enumerate(looks):
            np.ascontiguousarray(c[:, :, y0:y1]).tofile(os.path.join(d, f"coords{i}.bin"))
            np.ascontiguousarray(bc.upstream(case, gs)[:, :, y0:y1]).tofile(os.path.join(d, f"go{i}.bin"))
        open(os.path.join(d, "meta.txt"), "w").write(f"{B} {D} {H} {W} {L} {r} {len(looks)} {q}\n")
        subprocess.run([exe, d], check=True)
        G = torch.from_numpy(np.fromfile(os.path.join(d, "G.bin"), np.float32))
        g1 = np.fromfile(os.path.join(d, "g1.bin"), np.float32).reshape(B, D, y1 - y0, W)
        g2 = np.fromfile(os.path.join(d, "g2.bin"), np.float32).reshape(B, D, H, W)
    print(f"{case} rows {y0}..{y1 - 1}: finite {bool(np.isfinite(g1).all() and np.isfinite(g2).all())}")
    if (y0, y1) != (0, H):
        return
    gold = os.path.join(ROOT, "tests", "golden")
    z = np.load(os.path.join(gold, f"backward_{case}.npz"))
    if "pyr_all_l0" in z:
        from eraft_amd.layout import levels_of
        for i, lv in enumerate(levels_of(G, B * H * W, H, W, L)):
            a, ref = lv[:, 0].numpy(), z[f"pyr_all_l{i}"]
            print(f"  level {i}: support mismatches {int(((a != 0) != (ref != 0)).sum())}, normwise {nw(a, ref):.3g}")
    print(f"  grad_fmap1 normwise {nw(g1, z['grad_fmap1']):.3g}, grad_fmap2 "
          f"{nw(g2, np.load(os.path.join(gold, f'backward_{case}_g2.npz'))['grad_fmap2']):.3g}")


if __name__ == "__main__":
    main()
