#!/usr/bin/env python3
"""Capture the reference CorrBlock's gradients (wzygzlm/E-RAFT at /root/reference) for the backward.

Run ONLY in the build container (the reference does not exist on the GPU box):
    PYTHONDONTWRITEBYTECODE=1 python tests/golden/make_golden_backward.py

Conventions of make_golden.py: the reference is imported read-only and run on torch-CPU; inputs
come from tests/prng.py (tests/backward_cases.py: cases, coordinate sets, upstream seeds), so the
fixtures store sha256 of the regenerated inputs and the reference's OUTPUTS only.

For every case the reference CorrBlock is built on leaf fmaps, looked up at the case's coordinate
sets, and the loss sum_i (out_i * go_i).sum() is differentiated -- once in fp64 (fmaps and coords
cast to double) and once in fp32:
  backward_<case>.npz     grad_fmap1: the fp64 gradient rounded to float32 (6e-8 relative, far below
                          the 1e-5 bar); for PYRAMID_CASES also the fp32 per-level gradients of the
                          lookups alone, of the whole loss (pyr_all_l<i>) and of the sigma = 40 lookup
                          alone (pyr_s40_l<i>).  For these the block's corr_pyramid entries are
                          replaced by detached leaf copies before the lookups: retain_grad() on the
                          original levels would add the avg_pool2d chain's share of the coarser
                          levels (the fold, which grad_fmap1 / grad_fmap2 already cover) and hide
                          which pixels each level's own taps touched.
  backward_<case>_g2.npz  grad_fmap2, likewise (its own file: the 1-MiB limit per committed file)
  backward_errors.json    the reference's own fp32-vs-fp64 error per case and gradient: normwise
                          (max |d| / rms, oracle.normwise_err: the statistic of the 1e-5 bar) and,
                          as *_l2, the relative Frobenius error
"""
import hashlib
import json
import os
import sys

sys.dont_write_bytecode = True
HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, os.path.dirname(HERE))          # tests/ (prng, backward_cases)
sys.path.insert(0, "/root/reference")

import numpy as np  # noqa: E402
import torch  # noqa: E402

import backward_cases as bc  # noqa: E402
from model.corr import CorrBlock  # noqa: E402  (reference)

torch.set_num_threads(8)


def sha(a):
    return hashlib.sha256(np.ascontiguousarray(a).tobytes()).hexdigest()


def normwise(got, ref):
    got, ref = np.asarray(got, np.float64), np.asarray(ref, np.float64)
    return float(np.max(np.abs(got - ref)) / np.sqrt(np.mean(ref * ref)))


def rel_l2(got, ref):
    got, ref = np.asarray(got, np.float64), np.asarray(ref, np.float64)
    return float(np.linalg.norm(got - ref) / np.linalg.norm(ref))


def run(case, dtype, only=None, keep_levels=False):
    """(grad_fmap1, grad_fmap2, [level grads]) of the loss over the case's lookups (or `only` one)."""
    _, _, _, _, L, r, _ = bc.CASES[case]
    f1, f2 = (torch.from_numpy(f).to(dtype).requires_grad_(True) for f in bc.fmaps(case))
    blk = CorrBlock(f1, f2, num_levels=L, radius=r)
    if keep_levels:   # the lookups' own gradient per level (module docstring)
        blk.corr_pyramid = [lv.detach().requires_grad_(True) for lv in blk.corr_pyramid]
    loss = 0.0
    for name, coords, gseed in bc.lookups(case):
        if only is not None and name != only:
            continue
        out = blk(torch.from_numpy(coords).to(dtype))
        assert torch.isfinite(out).all(), (case, name)
        loss = loss + (out * torch.from_numpy(bc.upstream(case, gseed))).sum()
    loss.backward()
    if keep_levels:
        return None, None, [lv.grad[:, 0].numpy().copy() for lv in blk.corr_pyramid]
    return f1.grad.numpy(), f2.grad.numpy(), None


def main():
    errors = {}
    total = 0
    for case, (B, D, H, W, L, r, seed) in bc.CASES.items():
        f1, f2 = bc.fmaps(case)
        g1d, g2d, _ = run(case, torch.float64)
        pyr = case in bc.PYRAMID_CASES
        g1f, g2f, _ = run(case, torch.float32)
        errors[case] = {"grad_fmap1": normwise(g1f, g1d), "grad_fmap2": normwise(g2f, g2d),
                        "grad_fmap1_l2": rel_l2(g1f, g1d), "grad_fmap2_l2": rel_l2(g2f, g2d)}
        rec = {"B": B, "D": D, "H": H, "W": W, "L": L, "r": r, "seed": seed,
               "sha_fmap1": sha(f1), "sha_fmap2": sha(f2),
               "lookups": np.asarray([n for n, _, _ in bc.lookups(case)]),
               "sha_coords": np.asarray([sha(c) for _, c, _ in bc.lookups(case)]),
               "grad_fmap1": g1d.astype(np.float32)}
        if pyr:
            _, _, lv_all = run(case, torch.float32, keep_levels=True)
            _, _, lv_s40 = run(case, torch.float32, only="s40", keep_levels=True)
            for i in range(L):
                rec[f"pyr_all_l{i}"] = lv_all[i]
                rec[f"pyr_s40_l{i}"] = lv_s40[i]
        p1 = os.path.join(HERE, f"backward_{case}.npz")
        p2 = os.path.join(HERE, f"backward_{case}_g2.npz")
        np.savez_compressed(p1, **rec)
        np.savez_compressed(p2, grad_fmap2=g2d.astype(np.float32))
        total += os.path.getsize(p1) + os.path.getsize(p2)
        print(f"backward_{case}: ref fp32 vs fp64 normwise g1 {errors[case]['grad_fmap1']:.2e} "
              f"g2 {errors[case]['grad_fmap2']:.2e}  ({os.path.getsize(p1)} + {os.path.getsize(p2)} bytes)")
    with open(os.path.join(HERE, "backward_errors.json"), "w") as fh:
        json.dump(errors, fh, indent=1, sort_keys=True)
    assert total < 4 * 1024 * 1024, total
    print(f"total {total} bytes")


if __name__ == "__main__":
    main()
