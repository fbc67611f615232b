#!/usr/bin/env python3
"""Times of the convex upsampling's backward (ecorr_upsample_flow_backward) at DSEC size (60 x 80,
B = 4 and B = 16) against the stock alternative: the reference expression (ERAFT.upsample_flow:
softmax, unfold, broadcast multiply, sum, permute) under autograd on the same GPU.  A measurement
tool, not a gate; appends one record per process run to profiles/upsample_backward/bench_upsample.json
(--out to change) and recomputes the summary over the runs, which DESIGN.md §3.5 quotes.

Per batch size, HIP events around each call, warm-up, median of --steps (>= 20):
  forward_us            ecorr_upsample_flow
  backward_both_us      ecorr_upsample_flow_backward, grad_flow and grad_mask
  backward_flow_us      grad_flow only        backward_mask_us    grad_mask only
  stock_fwd_bwd_us      the reference expression forward + backward (autograd, both gradients)
  ours_fwd_bwd_us       eraft_amd.upsample_flow forward + backward through the autograd Function
  peak bytes            torch.cuda.max_memory_allocated over 12 calls + the backward of each, ours and stock
Algorithmic bytes are computed here from the shapes: mask in, grad_out in, grad_mask out (+ flow in,
grad_flow out); the share of the HBM roofline is those bytes at 8 TB/s over the measured time.

One process run measures everything; run it at least three times, each under its own time limit,
chained, for the spread between runs:
  timeout -k 10 240 python tools/bench_upsample_backward.py && \\
  timeout -k 10 240 python tools/bench_upsample_backward.py && \\
  timeout -k 10 240 python tools/bench_upsample_backward.py
"""
import argparse
import ctypes
import json
import os
import statistics
import sys

import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

H, W, CALLS = 60, 80, 12
HBM_PEAK = 8.0e12   # bytes / s (spec)


def timed(fn, steps, warmup):
    for _ in range(warmup):
        fn()
    ts = []
    for _ in range(steps):
        e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        e0.record()
        fn()
        e1.record()
        e1.synchronize()
        ts.append(e0.elapsed_time(e1) * 1e3)
    return round(statistics.median(ts), 2)


def peak_of(fn):
    torch.cuda.synchronize()
    torch.cuda.empty_cache()
    torch.cuda.reset_peak_memory_stats()
    base = torch.cuda.memory_allocated()
    fn()
    torch.cuda.synchronize()
    return torch.cuda.max_memory_allocated() - base


def measure(B, steps, warmup):
    import eraft_amd
    from eraft_amd import _lib
    from eraft_amd.network import ERAFT
    g = torch.Generator(device="cuda").manual_seed(B)
    flow = torch.randn((B, 2, H, W), generator=g, device="cuda") * 3.0
    mask = torch.randn((B, 576, H, W), generator=g, device="cuda") * 0.5
    go = torch.randn((B, 2, 8 * H, 8 * W), generator=g, device="cuda")
    L = _lib.lib()
    st = ctypes.c_void_p(torch.cuda.current_stream().cuda_stream)
    n = ctypes.c_int64()
    _lib.check(L.ecorr_upsample_backward_workspace_size(B, H, W, ctypes.byref(n)), "size")
    ws = torch.empty(n.value, dtype=torch.uint8, device="cuda")
    gf, gm, out = torch.empty_like(flow), torch.empty_like(mask), torch.empty_like(go)

    def fwd():
        _lib.check(L.ecorr_upsample_flow(flow.data_ptr(), mask.data_ptr(), B, H, W, out.data_ptr(), st), "forward")

    def bwd(a, b):
        _lib.check(L.ecorr_upsample_flow_backward(go.data_ptr(), flow.data_ptr(), mask.data_ptr(), B, H, W,
                                                  None if a is None else a.data_ptr(),
                                                  None if b is None else b.data_ptr(), ws.data_ptr(), st), "backward")

    def step(op):   # one forward + backward with both gradients through autograd
        f, m = flow.detach().requires_grad_(True), mask.detach().requires_grad_(True)
        op(f, m).backward(go)

    def twelve(op):   # the training pattern: 12 upsampled predictions alive, then the backward of each
        f, m = flow.detach().requires_grad_(True), mask.detach().requires_grad_(True)
        sum((op(f, m) * go).sum() for _ in range(CALLS)).backward()

    px = B * H * W
    bytes_fwd = px * (2304 + 8 + 512)
    bytes_mask = px * (2304 + 512 + 2304 + 8)     # mask, grad_out, grad_mask, flow
    bytes_flow = px * (2304 + 512 + 8)            # mask, grad_out, grad_flow (t stays on chip or in the workspace)
    bytes_both = px * (2304 + 512 + 2304 + 8 + 8)
    rec = {
        "B": B, "steps": steps, "warmup": warmup,
        "forward_us": timed(fwd, steps, warmup),
        "backward_both_us": timed(lambda: bwd(gf, gm), steps, warmup),
        "backward_flow_us": timed(lambda: bwd(gf, None), steps, warmup),
        "backward_mask_us": timed(lambda: bwd(None, gm), steps, warmup),
        "ours_fwd_bwd_us": timed(lambda: step(eraft_amd.upsample_flow), steps, warmup),
        "stock_fwd_bwd_us": timed(lambda: step(ERAFT.upsample_flow), steps, warmup),
        "ours_peak_bytes_12_calls": peak_of(lambda: twelve(eraft_amd.upsample_flow)),
        "stock_peak_bytes_12_calls": peak_of(lambda: twelve(ERAFT.upsample_flow)),
        "workspace_bytes": n.value,
        "forward_algorithmic_bytes": bytes_fwd, "backward_both_algorithmic_bytes": bytes_both,
        "backward_flow_algorithmic_bytes": bytes_flow, "backward_mask_algorithmic_bytes": bytes_mask,
    }
    return rec


def summarize(runs):
    """Per batch size and timing: the median over the process runs' medians, with their min and max."""
    out = {}
    for key in sorted({k for r in runs for k in r}):
        recs = [r[key] for r in runs if key in r]
        s = {"runs": len(recs)}
        for name in recs[0]:
            vals = [r[name] for r in recs]
            if name.endswith("_us"):
                s[name] = {"median": round(statistics.median(vals), 2), "min": min(vals), "max": max(vals)}
            elif name.endswith("bytes") or name.endswith("_calls"):
                s[name] = max(vals)
        for name in ("forward", "backward_both", "backward_flow", "backward_mask"):
            t = s[f"{name}_us"]["median"] * 1e-6
            rate = s[f"{name}_algorithmic_bytes"] / t
            s[f"{name}_bytes_per_s"] = round(rate, -9)
            s[f"{name}_hbm_roofline_share"] = round(rate / HBM_PEAK, 3)
        s["stock_over_ours_fwd_bwd"] = round(s["stock_fwd_bwd_us"]["median"] / s["ours_fwd_bwd_us"]["median"], 2)
        s["backward_over_forward_byte_rate"] = round(s["backward_both_bytes_per_s"] / s["forward_bytes_per_s"], 2)
        out[key] = s
    return out


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--batches", type=int, nargs="+", default=[4, 16])
    ap.add_argument("--steps", type=int, default=30)
    ap.add_argument("--warmup", type=int, default=5)
    ap.add_argument("--lib", default=None, help="another build of libecorr.so (tools/lab_build.py) for an A/B")
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "upsample_backward", "bench_upsample.json"))
    a = ap.parse_args()
    if a.steps < 20:
        raise SystemExit("bench_upsample_backward: --steps must be at least 20")
    if not torch.cuda.is_available():
        raise SystemExit("bench_upsample_backward: no HIP device (there is no CPU path)")
    torch.backends.cuda.matmul.allow_tf32 = False
    if a.lib:
        from eraft_amd import _lib
        _lib.LIB_PATH = os.path.abspath(a.lib)
    run = {f"B{B}": measure(B, a.steps, a.warmup) for B in a.batches}
    os.makedirs(os.path.dirname(a.out), exist_ok=True)
    doc = json.load(open(a.out)) if os.path.exists(a.out) else {}
    doc["shape"] = {"H": H, "W": W, "calls_for_peak": CALLS}
    doc["device"] = torch.cuda.get_device_name(0)
    if a.lib:
        doc["lib"] = os.path.relpath(a.lib, ROOT)
    doc.setdefault("runs", []).append(run)
    doc["summary"] = summarize(doc["runs"])
    json.dump(doc, open(a.out, "w"), indent=1, sort_keys=True)
    print(json.dumps(run))


if __name__ == "__main__":
    main()
