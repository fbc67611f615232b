#!/usr/bin/env python3
"""Every gradient of the backward paths as bits, for comparing two trees: the backward is
deterministic, so a refactor that leaves behaviour alone leaves every array here bit for bit.
    python tools/dump_backward.py --out DIR [--against OTHER_DIR]
runs, with the package of the tree the tool stands in,
  corr_<case>   CorrBlock(differentiable=True) on tests/backward_cases.py (all five: D = 3, 64, 100, 256,
                8 x 8 .. 17 x 20): grad_fmap1, grad_fmap2;
  alt_<case>    AlternateCorrBlock(trainable=True) on tests/alt_corr_cases.py (all but the case with a
                1-pixel level, which a trainable block refuses), nine lookups each: grad_fmap1, grad_fmap2;
  conv_<shape>  ecorr_conv1x1_relu_backward on the shapes of tests/test_conv_grad_gpu.py: grad_in,
                grad_weight, grad_bias;
  motion_t16x24 the same three through CorrBlock.lookup_conv1x1_relu (live block): grad_fmap1,
                grad_fmap2, grad_weight, grad_bias
and writes DIR/<group>.npz and DIR/sha256.txt (one line per array).  --against: compares with another
tree's DIR afterwards; exit status 1 when an array differs or is missing.  Needs a HIP device.
"""
import argparse
import ctypes
import hashlib
import os
import sys

import numpy as np
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
for p in (ROOT, os.path.join(ROOT, "oracle"), os.path.join(ROOT, "tests")):
    sys.path.insert(0, p)
import alt_corr_cases as ac  # noqa: E402
import backward_cases as bc  # noqa: E402
import prng  # noqa: E402

DEV = "cuda:0"
CONV_SHAPES = [(2, 324, 2500, 256), (1, 324, 64, 256), (3, 243, 130, 96), (1, 81, 70, 300), (2, 100, 200, 20),
               (2, 20, 1, 64)]   # tests/test_conv_grad_gpu.py SHAPES


def cuda(a):
    return torch.from_numpy(np.ascontiguousarray(a)).to(DEV)


def block_grads(make, f1n, f2n, lookups):
    """Gradients of sum_i (blk(coords_i) * go_i).sum() for blk = make(f1, f2)."""
    f1, f2 = cuda(f1n).requires_grad_(True), cuda(f2n).requires_grad_(True)
    blk = make(f1, f2)
    loss = 0.0
    for coords, go in lookups:
        loss = loss + (blk(cuda(coords)) * cuda(go)).sum()
    loss.backward()
    return {"grad_fmap1": f1.grad, "grad_fmap2": f2.grad}


def conv_grads(shape):
    from eraft_amd import _lib
    B, C, Q, O = shape
    x = cuda(prng.normal(801, (B, C, Q)))
    w = cuda((prng.normal(802, (O, C)) * np.float32(0.05)).astype(np.float32))
    bias = cuda((prng.normal(803, (O,)) * np.float32(0.1)).astype(np.float32))
    go = cuda(prng.normal(804, (B, O, Q)))
    st = _lib.stream_of(x)
    out = torch.empty((B, O, Q), dtype=torch.float32, device=DEV)
    _lib.check(_lib.lib().ecorr_conv1x1_relu_split(
        x.data_ptr(), B, C, Q, None, 0, _lib.packed_conv1x1_weight(w, O, C, "split", st, {}).data_ptr(),
        bias.data_ptr(), O, out.data_ptr(), st), "split conv")
    n = ctypes.c_int64()
    _lib.check(_lib.lib().ecorr_conv1x1_relu_backward_workspace_size(B, C, Q, O, ctypes.byref(n)), "size")
    ws = torch.zeros(n.value // 4, dtype=torch.float32, device=DEV)
    res = {"grad_in": torch.zeros((B, C, Q), device=DEV), "grad_weight": torch.zeros((O, C), device=DEV),
           "grad_bias": torch.zeros((O,), device=DEV)}
    _lib.check(_lib.lib().ecorr_conv1x1_relu_backward(
        go.data_ptr(), out.data_ptr(), x.data_ptr(), _lib.packed_conv1x1_weight(w, O, C, "split_t", st, {}).data_ptr(),
        B, C, Q, O, res["grad_in"].data_ptr(), res["grad_weight"].data_ptr(), res["grad_bias"].data_ptr(),
        ws.data_ptr(), st), "conv backward")
    return res


def motion_grads(case):
    import eraft_amd
    _, _, _, _, L, r, seed = bc.CASES[case]
    C, O = L * (2 * r + 1) ** 2, 256
    f1n, f2n = bc.fmaps(case)
    f1, f2 = cuda(f1n).requires_grad_(True), cuda(f2n).requires_grad_(True)
    w = cuda((prng.normal(seed + 300, (O, C, 1, 1)) * np.float32(0.05)).astype(np.float32)).requires_grad_(True)
    bias = cuda((prng.normal(seed + 301, (O,)) * np.float32(0.1)).astype(np.float32)).requires_grad_(True)
    blk = eraft_amd.CorrBlock(f1, f2, num_levels=L, radius=r, differentiable=True)
    loss = 0.0
    for i, (_, coords, _) in enumerate(bc.lookups(case)):
        out = blk.lookup_conv1x1_relu(cuda(coords), w, bias)
        loss = loss + (out * cuda(prng.normal(seed + 310 + i, tuple(out.shape)))).sum()
    loss.backward()
    return {"grad_fmap1": f1.grad, "grad_fmap2": f2.grad, "grad_weight": w.grad, "grad_bias": bias.grad}


def groups():
    import eraft_amd
    for case, (_, _, _, _, L, r, _) in bc.CASES.items():
        looks = [(c, bc.upstream(case, gseed)) for _, c, gseed in bc.lookups(case)]
        yield f"corr_{case}", block_grads(
            lambda a, b: eraft_amd.CorrBlock(a, b, num_levels=L, radius=r, differentiable=True), *bc.fmaps(case), looks)
    for name, (r, B, _, H, W, L) in ac.CASES.items():
        if ac.h1_level(name) is not None:
            continue
        s = ac.seed_of(name)
        looks = [(c, prng.normal(s + 20 + i, (B, ac.channels(name), H, W)))
                 for i, c in enumerate(ac.coord_sets(name).values())]
        yield f"alt_{name}", block_grads(
            lambda a, b: eraft_amd.AlternateCorrBlock(a, b, num_levels=L, radius=r, trainable=True), *ac.fmaps(name), looks)
    for shape in CONV_SHAPES:
        yield "conv_b%d_c%d_q%d_o%d" % shape, conv_grads(shape)
    yield "motion_t16x24", motion_grads("t16x24")


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--out", required=True)
    ap.add_argument("--against")
    a = ap.parse_args()
    if not torch.cuda.is_available():
        raise SystemExit("dump_backward: no HIP device (there is no CPU path)")
    os.makedirs(a.out, exist_ok=True)
    lines = []
    for group, arrays in groups():
        torch.cuda.synchronize()
        arrays = {k: v.cpu().numpy() for k, v in arrays.items()}
        np.savez(os.path.join(a.out, group + ".npz"), **arrays)
        lines += [f"{hashlib.sha256(v.tobytes()).hexdigest()}  {group}/{k} {v.shape}" for k, v in arrays.items()]
    open(os.path.join(a.out, "sha256.txt"), "w").write("\n".join(lines) + "\n")
    print(f"dump_backward: {len(lines)} arrays in {a.out}")
    if a.against:
        other = set(open(os.path.join(a.against, "sha256.txt")).read().splitlines())
        bad = [ln for ln in lines if ln not in other]
        print(f"against {a.against}: {len(lines) - len(bad)} of {len(lines)} arrays bit for bit"
              + "".join(f"\n  DIFFERS {ln.split('  ')[1]}" for ln in bad))
        if bad or len(other) != len(lines):
            raise SystemExit(1)


if __name__ == "__main__":
    main()
