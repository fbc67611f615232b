#!/usr/bin/env python3
"""What training through the HIP motion encoder costs: forward + backward of eraft_amd.motion_encoder_train
(csrc/motion_enc.hip + csrc/motion_enc_grad.hip, fp32 MFMA, intermediates recomputed) against stock autograd over
network.BasicMotionEncoder.forward(flow, c1, corr_is_convc1=True) on MIOpen fp32 with TF32 off; flow, c1 and the
eight parameters behind convc1 all require grad.  A measurement tool, not a gate; writes
profiles/motion_encoder/bench_backward.json (--out to change), which DESIGN.md §3.12.1 and the README quote.  It
fails without a HIP device: there is no fallback.

Shapes and method as tools/bench_motion_encoder.py: DSEC's 60 x 80 map at B = 1 and B = 16, MVSEC's 32 x 32 map at
B = 64, a 92 x 160 map at B = 4; per shape the two arms alternate call by call in one process, HIP events around each
forward + backward, --warmup (>= 5) unrecorded rounds, then the median of --steps (>= 20) with min and max.  The loss
is sum(out * grad_out) with a fixed grad_out; the parameters' .grad is dropped between calls.  The two arms'
gradients are compared as a relative Frobenius difference pooled over the ten tensors; the largest single-element
difference is recorded beside it and is no accuracy figure at the large shapes: among 10^7 pre-activations a few
lie within an fp32 rounding of 0, the arms (or either and an fp64 module) then disagree on that ReLU's mask, and the
3 x 3 patch of grad_c1 behind it moves by a whole term (10^-2 of the largest element).

Memory: torch.cuda.max_memory_allocated over one training step of 12 encoder calls, as the 12 iterations of the
network make them -- every call on a fresh c1 and flow (c1 * s_i, flow + d_i: both arms keep those, as the network
keeps convc1's output), the losses summed, then one backward -- minus what was allocated before the step, per arm.

--trace-only runs ten forward + backward calls at DSEC B = 16 and nothing else: the program of a
`rocprofv3 --kernel-trace --stats` run of its own.
"""
import argparse
import json
import os
import statistics
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(ROOT, "tools"))

from bench_motion_encoder import SHAPES, make_inputs, timed   # noqa: E402  (the forward tool's recipe)

ITERS = 12
OUT = 128


def make_encoder(torch, nw):
    torch.manual_seed(7)
    enc = nw.BasicMotionEncoder().cuda().train()
    enc.convc1.requires_grad_(False)   # in front of both arms: not part of either
    return enc


def step(torch, fn, enc, flow, c1, go, iters=1):
    for p in enc.parameters():
        p.grad = None
    flow.grad = c1.grad = None
    if iters == 1:
        loss = (fn(flow, c1) * go).sum()
    else:
        loss = sum((fn(flow + 0.01 * i, c1 * (1.0 + 0.01 * i)) * go).sum() for i in range(iters))
    loss.backward()


def summary(ms):
    return {"ms": round(statistics.median(ms), 4), "ms_min": round(min(ms), 4), "ms_max": round(max(ms), 4),
            "calls": len(ms)}


def bench_shape(torch, eraft_amd, enc, shape, steps, warmup):
    B, H, W = SHAPES[shape]
    flow, c1 = make_inputs(torch, B, H, W)
    flow.requires_grad_(True)
    c1.requires_grad_(True)
    go = torch.randn((B, OUT, H, W), generator=torch.Generator(device="cuda").manual_seed(11), device="cuda")
    arms = {"miopen": lambda f, c: enc(f, c, corr_is_convc1=True),
            "hip": lambda f, c: eraft_amd.motion_encoder_train(f, c, enc)}
    ms = {k: [] for k in arms}
    for i in range(warmup + steps):
        for k, fn in arms.items():   # alternating
            t = timed(torch, lambda: step(torch, fn, enc, flow, c1, go))
            if i >= warmup:
                ms[k].append(t)
    rec = {k: summary(v) for k, v in ms.items()}
    rec["hip_over_miopen_ms"] = round(rec["hip"]["ms"] / rec["miopen"]["ms"], 4)
    # the gap counts only where the two arms' ranges do not overlap
    rec["ranges_disjoint"] = bool(rec["hip"]["ms_max"] < rec["miopen"]["ms_min"] or
                                  rec["miopen"]["ms_max"] < rec["hip"]["ms_min"])
    grads = {}
    for k, fn in arms.items():
        step(torch, fn, enc, flow, c1, go)
        grads[k] = [flow.grad.clone(), c1.grad.clone()] + [p.grad.clone() for p in enc.parameters() if p.grad is not None]
    # pooled over the ten tensors; the largest single element beside it: two fp32 encoders can disagree on the sign
    # of a pre-activation at 0, and one flipped ReLU mask moves a 3 x 3 patch of grad_c1 by a whole term
    rec["rel_frobenius_difference"] = float((sum(float(((a - b).double() ** 2).sum()) for a, b in
                                                 zip(grads["hip"], grads["miopen"])) /
                                             sum(float((b.double() ** 2).sum()) for b in grads["miopen"])) ** 0.5)
    rec["max_rel_difference"] = max(float((a - b).abs().max() / b.abs().max())
                                    for a, b in zip(grads["hip"], grads["miopen"]))
    del grads
    for k, fn in arms.items():   # peak memory of 12 calls, forward + backward
        step(torch, fn, enc, flow, c1, go)   # the packs, the workspace sizes: not part of a step
        torch.cuda.synchronize()
        for p in enc.parameters():
            p.grad = None
        flow.grad = c1.grad = None
        torch.cuda.reset_peak_memory_stats()
        base = torch.cuda.memory_allocated()
        step(torch, fn, enc, flow, c1, go, iters=ITERS)
        torch.cuda.synchronize()
        rec[k][f"peak_bytes_{ITERS}_calls"] = int(torch.cuda.max_memory_allocated() - base)
    rec["hip_over_miopen_peak_bytes"] = round(rec["hip"][f"peak_bytes_{ITERS}_calls"] /
                                              rec["miopen"][f"peak_bytes_{ITERS}_calls"], 4)
    rec["out_bytes"] = B * OUT * H * W * 4
    rec["B_H_W"] = [B, H, W]
    return rec


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--shapes", nargs="+", default=list(SHAPES), choices=list(SHAPES))
    ap.add_argument("--steps", type=int, default=20)
    ap.add_argument("--warmup", type=int, default=5)
    ap.add_argument("--trace-only", action="store_true")
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "motion_encoder", "bench_backward.json"))
    a = ap.parse_args()
    if a.steps < 20 or a.warmup < 5:
        raise SystemExit("bench_motion_encoder_backward: --steps >= 20 and --warmup >= 5")
    import torch
    sys.path.insert(0, ROOT)
    import eraft_amd
    from eraft_amd import network as nw
    if not torch.cuda.is_available():
        raise SystemExit("bench_motion_encoder_backward: no HIP device (there is no CPU path)")
    torch.backends.cuda.matmul.allow_tf32 = False
    torch.backends.cudnn.allow_tf32 = False
    enc = make_encoder(torch, nw)
    if a.trace_only:
        flow, c1 = make_inputs(torch, *SHAPES["dsec_b16"])
        flow.requires_grad_(True)
        c1.requires_grad_(True)
        go = torch.ones((c1.shape[0], OUT) + tuple(c1.shape[2:]), device="cuda")
        for _ in range(10):
            step(torch, lambda f, c: eraft_amd.motion_encoder_train(f, c, enc), enc, flow, c1, go)
        torch.cuda.synchronize()
        return
    doc = {"device": torch.cuda.get_device_name(0),
           "what": "forward + backward of the motion encoder behind convc1; flow, c1 and the eight parameters require grad",
           "protocol": f"alternating arms, {a.warmup} warm-up rounds, median of {a.steps}, HIP events, TF32 off",
           "source_digest": eraft_amd._lib.source_digest(), "shapes": {}}
    for shape in a.shapes:
        doc["shapes"][shape] = bench_shape(torch, eraft_amd, enc, shape, a.steps, a.warmup)
        print(shape, json.dumps(doc["shapes"][shape]), flush=True)
    os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
    json.dump(doc, open(a.out, "w"), indent=1, sort_keys=True)


if __name__ == "__main__":
    main()
