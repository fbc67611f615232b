#!/usr/bin/env python3
"""Every result of the event side (csrc/splat.hip, csrc/voxel.hip) as bits, for comparing two trees:
both are deterministic, so a refactor that leaves behaviour alone leaves every array here bit for bit.
The suite pins raw grids and splats to the serial oracle bit for bit but normalized grids only within
1e-6, so a change in the order of the moments' tree shows here and not there.
    python tools/dump_events.py --out DIR [--against OTHER_DIR] [--arrays]
runs, with the package of the tree the tool stands in,
  splat_<case>  every case of tests/splat_cases.py through forward_interpolate_pytorch (flow mode: out)
                or grid_sample_values (points mode: values, valid);
  voxel_<case>  every case of tests/voxel_dispatch.py through VoxelGrid.convert (DSEC) or
                EventSequenceToVoxelGrid_Pytorch (MVSEC), normalize off and on: grid_norm0, grid_norm1
and writes DIR/sha256.txt (one line per array; --arrays: DIR/<group>.npz too).  --against: compares
with another tree's DIR afterwards; exit status 1 when an array differs or is missing.  Needs a HIP
device.
"""
import argparse
import hashlib
import os
import sys
import types

import numpy as np
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
for p in (ROOT, os.path.join(ROOT, "oracle"), os.path.join(ROOT, "tests")):
    sys.path.insert(0, p)
import splat_cases as sc  # noqa: E402
import voxel_dispatch as vd  # noqa: E402

DEV = "cuda:0"


def cuda(a):
    return torch.from_numpy(np.ascontiguousarray(a)).to(DEV)


def splat(name):
    import eraft_amd
    c, data = sc.CASES[name], cuda(sc.inputs(name))
    if c["mode"] == "flow":
        return {"out": eraft_amd.forward_interpolate_pytorch(data)}
    values, valid = eraft_amd.grid_sample_values(data, c["h"], c["w"])
    return {"values": values, "valid": valid}


def voxel(name):
    import eraft_amd
    dsec, _, C, H, W = vd.CASES[name]["shape"]
    ev, out = vd.events(name), {}
    for norm in (0, 1):
        if dsec:
            grid = eraft_amd.VoxelGrid((C, H, W), normalize=bool(norm)).convert(dict(zip("ptxy", map(cuda, ev))))
        else:
            seq = types.SimpleNamespace(features=ev, image_width=W, image_height=H)
            grid = eraft_amd.EventSequenceToVoxelGrid_Pytorch(C, normalize=bool(norm))(seq)
        out[f"grid_norm{norm}"] = grid
    return out


def groups():
    for name in sc.CASES:
        yield f"splat_{name}", splat(name)
    for name in vd.CASES:
        yield f"voxel_{name}", voxel(name)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--out", required=True)
    ap.add_argument("--against")
    ap.add_argument("--arrays", action="store_true")
    a = ap.parse_args()
    if not torch.cuda.is_available():
        raise SystemExit("dump_events: no HIP device (there is no CPU path)")
    os.makedirs(a.out, exist_ok=True)
    lines = []
    with torch.no_grad():
        for group, arrays in groups():
            torch.cuda.synchronize()
            arrays = {k: v.cpu().numpy() for k, v in arrays.items()}
            if a.arrays:
                np.savez(os.path.join(a.out, group + ".npz"), **arrays)
            lines += [f"{hashlib.sha256(v.tobytes()).hexdigest()}  {group}/{k} {v.dtype} {v.shape}"
                      for k, v in arrays.items()]
    open(os.path.join(a.out, "sha256.txt"), "w").write("\n".join(lines) + "\n")
    print(f"dump_events: {len(lines)} arrays in {a.out}")
    if a.against:
        other = set(open(os.path.join(a.against, "sha256.txt")).read().splitlines())
        bad = [ln for ln in lines if ln not in other]
        print(f"against {a.against}: {len(lines) - len(bad)} of {len(lines)} arrays bit for bit"
              + "".join(f"\n  DIFFERS {ln.split('  ')[1]}" for ln in bad))
        if bad or len(other) != len(lines):
            raise SystemExit(1)


if __name__ == "__main__":
    main()
