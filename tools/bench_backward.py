#!/usr/bin/env python3
"""Times of the CorrBlock backward at DSEC size (60 x 80, D = 256, 12 lookups) against the stock
alternative: oracle/torch_ref.py's op sequence (bmm, avg_pool2d, grid_sample) under autograd on the
same GPU.  A measurement tool, not a gate; writes profiles/backward/bench_backward.json
(--out to change), which DESIGN.md §3.9 quotes.

Per kernel (HIP events around each C-ABI call, warm-up, median of --steps):
  lookup_backward   one ecorr_lookup_backward call (median over the 12 lookups' calls and the steps)
  fold + GEMMs      ecorr_build_backward with both outputs; each GEMM alone as a 1-level call with
                    one output (no fold runs for one level); the fold as the difference between
                    the 4-level and the 1-level call with the same single output (`fold_est_us`)
Whole step: CorrBlock(differentiable=True) build, 12 lookups, loss, backward -- ours and stock.
Peak memory: torch.cuda.max_memory_allocated over one step of each.
Algorithmic bytes and FLOPs are computed here from the shapes.

Run each mode in its own process under a time limit, chained:
  timeout -k 10 300 python tools/bench_backward.py --mode ours && \\
  timeout -k 10 300 python tools/bench_backward.py --mode stock
(both append to the same JSON file).
"""
import argparse
import ctypes
import json
import os
import statistics
import sys

import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
for p in (ROOT, os.path.join(ROOT, "oracle"), os.path.join(ROOT, "tests")):
    sys.path.insert(0, p)

H, W, D, LEVELS, RADIUS, LOOKUPS = 60, 80, 256, 4, 4, 12


def inputs(B):
    g = torch.Generator(device="cuda").manual_seed(0)
    f1 = torch.randn((B, D, H, W), generator=g, device="cuda")
    f2 = torch.randn((B, D, H, W), generator=g, device="cuda")
    ys, xs = torch.meshgrid(torch.arange(H, device="cuda", dtype=torch.float32),
                            torch.arange(W, device="cuda", dtype=torch.float32), indexing="ij")
    base = torch.stack([xs, ys])[None].repeat(B, 1, 1, 1)
    smooth = torch.nn.functional.avg_pool2d(torch.randn((B, 2, H, W), generator=g, device="cuda") * 9.0, 5, 1, 2)
    coords = [(base + smooth + 0.5 * torch.randn((B, 2, H, W), generator=g, device="cuda")).contiguous()
              for _ in range(LOOKUPS)]
    C = LEVELS * (2 * RADIUS + 1) ** 2
    gos = [torch.randn((B, C, H, W), generator=g, device="cuda") for _ in range(2)]
    return f1, f2, coords, gos


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
    return ts


def med(ts):
    return round(statistics.median(ts), 2)


def step(cls, f1, f2, coords, gos, **kw):
    a, b = f1.detach().requires_grad_(True), f2.detach().requires_grad_(True)
    blk = cls(a, b, num_levels=LEVELS, radius=RADIUS, **kw)
    loss = 0.0
    for i, c in enumerate(coords):
        loss = loss + (blk(c) * gos[i & 1]).sum()
    loss.backward()
    return a.grad, b.grad


def peak_of(fn):
    torch.cuda.synchronize()
    torch.cuda.empty_cache()
    torch.cuda.reset_peak_memory_stats()
    base = torch.cuda.memory_allocated()
    fn()
    torch.cuda.synchronize()
    return torch.cuda.max_memory_allocated() - base


def run_ours(B, steps, warmup):
    import eraft_amd
    from eraft_amd import _lib
    f1, f2, coords, gos = inputs(B)
    L = _lib.lib()
    st = ctypes.c_void_p(torch.cuda.current_stream().cuda_stream)
    Q = H * W
    _, _, off = _lib.layout(B * Q, H, W, LEVELS)
    G = torch.zeros(off[-1], device="cuda")
    g1, g2 = torch.empty_like(f1), torch.empty_like(f2)

    def lookup_bw(i):
        _lib.check(L.ecorr_lookup_backward(gos[i & 1].data_ptr(), coords[i].data_ptr(), B, H, W, Q, LEVELS, RADIUS,
                                           G.data_ptr(), st), "lookup backward")

    def build_bw(a, b, levels=LEVELS):
        _lib.check(L.ecorr_build_backward(G.data_ptr(), f1.data_ptr(), f2.data_ptr(), B, D, H, W, Q, levels,
                                          None if a is None else a.data_ptr(), None if b is None else b.data_ptr(), st), "build backward")

    with torch.no_grad():
        blk = eraft_amd.CorrBlock(f1, f2, num_levels=LEVELS, radius=RADIUS)
        t_fw = []
        t_lk = []
        for i in range(LOOKUPS):
            t_fw += timed(lambda: blk(coords[i]), max(steps // 4, 5), 2)
            t_lk += timed(lambda: lookup_bw(i), max(steps // 4, 5), 2)
        # the GEMMs read level 0 only, so a 1-level call is the GEMMs without the fold (G's values do
        # not matter for the time; the fold rewrites level 0 in place, finite stays finite at 1/4 weights)
        G.zero_()
        lookup_bw(0)
        t_both = timed(lambda: build_bw(g1, g2), steps, warmup)
        t_g1 = timed(lambda: build_bw(g1, None, 1), steps, warmup)
        t_g2 = timed(lambda: build_bw(None, g2, 1), steps, warmup)
        t_fold1 = timed(lambda: build_bw(g1, None), steps, warmup)
        del blk
    t_step = timed(lambda: step(eraft_amd.CorrBlock, f1, f2, coords, gos, differentiable=True), steps, warmup)
    peak = peak_of(lambda: step(eraft_amd.CorrBlock, f1, f2, coords, gos, differentiable=True))
    rows = B * Q
    C = LEVELS * 81
    pyr_bytes = off[-1] * 4
    return {
        "B": B, "steps": steps,
        "lookup_forward_us": med(t_fw), "lookup_backward_us": med(t_lk),
        "build_backward_us": med(t_both), "gemm_grad_fmap1_us": med(t_g1), "gemm_grad_fmap2_us": med(t_g2),
        "fold_est_us": round(med(t_fold1) - med(t_g1), 2),
        "step_forward_backward_us": med(t_step), "step_peak_bytes": peak,
        "pyramid_bytes": pyr_bytes,
        # algorithmic traffic: upstream read once, (2r+2)^2 window cells read + written per query and level
        "lookup_backward_algorithmic_bytes": rows * (C * 4 + LEVELS * 100 * 8 + 8),
        "fold_algorithmic_bytes": pyr_bytes + rows * Q * 4,
        "gemm_flops_each": 2 * B * Q * Q * D,
        "gemm_algorithmic_bytes_each": rows * Q * 4 + 2 * B * D * Q * 4,
    }


def run_stock(B, steps, warmup):
    from torch_ref import TorchCpuCorrBlock
    f1, f2, coords, gos = inputs(B)
    t_step = timed(lambda: step(TorchCpuCorrBlock, f1, f2, coords, gos), steps, warmup)
    peak = peak_of(lambda: step(TorchCpuCorrBlock, f1, f2, coords, gos))
    return {"B": B, "steps": steps, "step_forward_backward_us": med(t_step), "step_peak_bytes": peak}


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--mode", choices=("ours", "stock"), required=True)
    ap.add_argument("--batch", type=int, default=4)
    ap.add_argument("--steps", type=int, default=20)
    ap.add_argument("--warmup", type=int, default=3)
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "backward", "bench_backward.json"))
    a = ap.parse_args()
    if not torch.cuda.is_available():
        raise SystemExit("bench_backward: no HIP device (there is no CPU path)")
    torch.backends.cuda.matmul.allow_tf32 = False
    rec = (run_ours if a.mode == "ours" else run_stock)(a.batch, a.steps, a.warmup)
    os.makedirs(os.path.dirname(a.out), exist_ok=True)
    doc = json.load(open(a.out)) if os.path.exists(a.out) else {}
    doc.setdefault("shape", {"H": H, "W": W, "D": D, "levels": LEVELS, "radius": RADIUS, "lookups": LOOKUPS})
    doc["device"] = torch.cuda.get_device_name(0)
    doc.setdefault(a.mode, {})[f"B{a.batch}"] = rec
    json.dump(doc, open(a.out, "w"), indent=1, sort_keys=True)
    print(json.dumps({a.mode: rec}))


if __name__ == "__main__":
    main()
