#!/usr/bin/env python3
"""What training through the HIP SepConvGRU costs: forward + backward of eraft_amd.sepconv_gru_train
(csrc/gru.hip + csrc/gru_grad.hip, fp32 MFMA, gates recomputed) against stock autograd over network.SepConvGRU
on MIOpen fp32 with TF32 off, hidden 128 / input 256; h, x and the twelve parameters all require grad.  A
measurement tool, not a gate; writes profiles/gru/bench_backward.json (--out to change), which DESIGN.md
§3.11.1 and the README quote.  It fails without a HIP device: there is no fallback.

Shapes and method as tools/bench_gru.py: DSEC's 60 x 80 map at B = 1 and B = 16, MVSEC's 32 x 32 map at B = 64,
a 92 x 160 map at B = 4; per shape the two arms alternate call by call in one process, HIP events around each
forward + backward, --warmup (>= 5) unrecorded rounds, then the median of --steps (>= 20) with min and max.
The loss is sum(h' * grad_out) with a fixed grad_out; the parameters' .grad is dropped between calls.

Memory: torch.cuda.max_memory_allocated over one training step of the GRU chained over 12 iterations
(h <- gru(h, x), then one backward), minus what was allocated before the step, per arm.

--trace-only runs ten forward + backward calls at DSEC B = 16 and nothing else: the program of a
`rocprofv3 --kernel-trace --stats` run of its own (profiles/gru/kernel_stats_backward.csv).
"""
import argparse
import json
import os
import statistics
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(ROOT, "tools"))

from bench_gru import HID, INP, SHAPES, make_gru, make_inputs, timed   # noqa: E402  (the forward tool's recipe)

ITERS = 12


def step(torch, fn, gru, h, x, go, iters=1):
    for p in gru.parameters():
        p.grad = None
    h.grad = x.grad = None
    out = h
    for _ in range(iters):
        out = fn(out, x)
    (out * go).sum().backward()


def summary(ms):
    return {"ms": round(statistics.median(ms), 4), "ms_min": round(min(ms), 4), "ms_max": round(max(ms), 4),
            "calls": len(ms)}


def bench_shape(torch, eraft_amd, gru, shape, steps, warmup):
    B, H, W = SHAPES[shape]
    h, x = make_inputs(torch, B, H, W)
    h.requires_grad_(True)
    x.requires_grad_(True)
    go = torch.randn(h.shape, generator=torch.Generator(device="cuda").manual_seed(11), device="cuda")
    arms = {"miopen": lambda a, b: gru(a, b), "hip": lambda a, b: eraft_amd.sepconv_gru_train(a, b, gru)}
    ms = {k: [] for k in arms}
    for i in range(warmup + steps):
        for k, fn in arms.items():   # alternating
            t = timed(torch, lambda: step(torch, fn, gru, h, x, go))
            if i >= warmup:
                ms[k].append(t)
    rec = {k: summary(v) for k, v in ms.items()}
    rec["hip_over_miopen_ms"] = round(rec["hip"]["ms"] / rec["miopen"]["ms"], 4)
    # the gap counts only where the two arms' ranges do not overlap
    rec["ranges_disjoint"] = bool(rec["hip"]["ms_max"] < rec["miopen"]["ms_min"] or
                                  rec["miopen"]["ms_max"] < rec["hip"]["ms_min"])
    grads = {}
    for k, fn in arms.items():
        step(torch, fn, gru, h, x, go)
        grads[k] = [h.grad.clone(), x.grad.clone()] + [p.grad.clone() for p in gru.parameters()]
    rec["max_rel_difference"] = max(float((a - b).abs().max() / b.abs().max())
                                    for a, b in zip(grads["hip"], grads["miopen"]))
    del grads
    for k, fn in arms.items():   # peak memory of a 12-iteration chain, forward + backward
        step(torch, fn, gru, h, x, go)   # the packs, the workspace sizes: not part of a step
        torch.cuda.synchronize()
        for p in gru.parameters():
            p.grad = None
        h.grad = x.grad = None
        torch.cuda.reset_peak_memory_stats()
        base = torch.cuda.memory_allocated()
        step(torch, fn, gru, h, x, go, iters=ITERS)
        torch.cuda.synchronize()
        rec[k][f"peak_bytes_{ITERS}_iterations"] = int(torch.cuda.max_memory_allocated() - base)
    rec["hip_over_miopen_peak_bytes"] = round(rec["hip"][f"peak_bytes_{ITERS}_iterations"] /
                                              rec["miopen"][f"peak_bytes_{ITERS}_iterations"], 4)
    rec["h_bytes"] = B * HID * H * W * 4
    rec["B_H_W"] = [B, H, W]
    return rec


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--shapes", nargs="+", default=list(SHAPES), choices=list(SHAPES))
    ap.add_argument("--steps", type=int, default=20)
    ap.add_argument("--warmup", type=int, default=5)
    ap.add_argument("--trace-only", action="store_true")
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "gru", "bench_backward.json"))
    a = ap.parse_args()
    if a.steps < 20 or a.warmup < 5:
        raise SystemExit("bench_gru_backward: --steps >= 20 and --warmup >= 5")
    import torch
    sys.path.insert(0, ROOT)
    import eraft_amd
    from eraft_amd import network as nw
    if not torch.cuda.is_available():
        raise SystemExit("bench_gru_backward: no HIP device (there is no CPU path)")
    torch.backends.cuda.matmul.allow_tf32 = False
    torch.backends.cudnn.allow_tf32 = False
    gru = make_gru(torch, nw).train()
    if a.trace_only:
        h, x = make_inputs(torch, *SHAPES["dsec_b16"])
        h.requires_grad_(True)
        x.requires_grad_(True)
        go = torch.ones_like(h)
        for _ in range(10):
            step(torch, lambda p, q: eraft_amd.sepconv_gru_train(p, q, gru), gru, h, x, go)
        torch.cuda.synchronize()
        return
    doc = {"device": torch.cuda.get_device_name(0),
           "what": "forward + backward of one SepConvGRU; h, x and the twelve parameters require grad",
           "protocol": f"alternating arms, {a.warmup} warm-up rounds, median of {a.steps}, HIP events, TF32 off",
           "source_digest": eraft_amd._lib.source_digest(), "shapes": {}}
    for shape in a.shapes:
        doc["shapes"][shape] = bench_shape(torch, eraft_amd, gru, shape, a.steps, a.warmup)
        print(shape, json.dumps(doc["shapes"][shape]), flush=True)
    os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
    json.dump(doc, open(a.out, "w"), indent=1, sort_keys=True)


if __name__ == "__main__":
    main()
