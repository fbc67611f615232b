#!/usr/bin/env python3
"""What training without the volume costs and saves: AlternateCorrBlock(trainable=True) against
CorrBlock(differentiable=True) from the same tree, at D = 256, 4 levels, radius 4 on DSEC's 60 x 80 map
(B = 1, 4, 16) and on a 92 x 160 map (B = 4): the shapes of tools/bench_alt_corr.py.  A measurement
tool, not a gate; writes profiles/alt_corr/bench_backward.json (--out to change), which DESIGN.md
§3.10.1 quotes.

Every measurement runs in a process of its own (one block, one shape), started one after the other by
this parent, which never touches the GPU: per shape the two blocks alternate (alt, volume, alt, volume,
...), --reps times each, and the summary is the median over a block's processes with their min and max.
Per process, HIP events around the Python calls, after a warm-up, medians of --steps:
  step_us          construction + 12 lookups + loss + backward: one training step's share of the block
  forward_us       construction + 12 lookups of that step (the backward is the difference)
  lookup_us        one forward corr_fn(coords) of the live block (the alt block's reads the same bytes
                   from L2 as its grad_f1 kernel: the floor to price that kernel against)
  step_peak_bytes  torch.cuda.max_memory_allocated over one step, above what was allocated before it
                   (fmaps, coords and the loss weights excluded)
  kernels          per kernel of one profiled step (torch.profiler): calls and mean device time
A child that fails ends the run: nothing more is started on the GPU after it.
"""
import argparse
import json
import os
import re
import statistics
import subprocess
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))

D, LEVELS, RADIUS, LOOKUPS = 256, 4, 4, 12
SHAPES = {"dsec_b1": (1, 60, 80), "dsec_b4": (4, 60, 80), "dsec_b16": (16, 60, 80), "hd_92x160_b4": (4, 92, 160)}
BLOCKS = ("alt", "volume")
KEYS = ("step_us", "forward_us", "lookup_us", "step_peak_bytes")


def child(block, shape, steps, warmup):
    import torch
    sys.path.insert(0, ROOT)
    import eraft_amd
    if not torch.cuda.is_available():
        raise SystemExit("bench_alt_backward: no HIP device (there is no CPU path)")
    B, H, W = SHAPES[shape]
    C = LEVELS * (2 * RADIUS + 1) ** 2
    g = torch.Generator(device="cuda").manual_seed(B * H)
    f1 = torch.randn((B, D, H, W), generator=g, device="cuda").requires_grad_(True)
    f2 = torch.randn((B, D, H, W), generator=g, device="cuda").requires_grad_(True)
    coords = [eraft_amd.coords_grid(B, H, W, device="cuda") + 2.0 * torch.randn((B, 2, H, W), generator=g, device="cuda")
              for _ in range(LOOKUPS)]
    go = torch.randn((B, C, H, W), generator=g, device="cuda")

    def make():
        if block == "alt":
            return eraft_amd.AlternateCorrBlock(f1, f2, num_levels=LEVELS, radius=RADIUS, trainable=True)
        return eraft_amd.CorrBlock(f1, f2, num_levels=LEVELS, radius=RADIUS, differentiable=True)

    def event():
        e = torch.cuda.Event(enable_timing=True)
        e.record()
        return e

    def step():
        """(forward us, whole step us)"""
        f1.grad = f2.grad = None
        e0 = event()
        fn = make()
        loss = 0.0
        for c in coords:
            loss = loss + (fn(c) * go).sum()
        e1 = event()
        loss.backward()
        e2 = event()
        e2.synchronize()
        return e0.elapsed_time(e1) * 1e3, e0.elapsed_time(e2) * 1e3

    for _ in range(warmup):
        step()
    fwd, whole, lookup = [], [], []
    for _ in range(steps):
        a, b = step()
        fwd.append(a)
        whole.append(b)
    fn = make()
    for _ in range(3 * steps):
        e0 = event()
        out = fn(coords[0])
        e1 = event()
        e1.synchronize()
        lookup.append(e0.elapsed_time(e1) * 1e3)
    del fn, out
    f1.grad = f2.grad = None
    torch.cuda.synchronize()
    torch.cuda.empty_cache()
    torch.cuda.reset_peak_memory_stats()
    base = torch.cuda.memory_allocated()
    step()
    torch.cuda.synchronize()
    peak = torch.cuda.max_memory_allocated() - base
    kernels, note = {}, None
    try:
        from torch.profiler import ProfilerActivity, profile
        with profile(activities=[ProfilerActivity.CUDA]) as prof:
            step()
            torch.cuda.synchronize()
        for ev in prof.key_averages():
            t = getattr(ev, "device_time_total", None)
            if t is None:
                t = getattr(ev, "cuda_time_total", 0.0)
            m = re.search(r"(\w+_kernel(?:<[^>]*>)?)", ev.key)
            if t and m and "ecorr" in ev.key:
                kernels[m.group(1)] = {"calls": ev.count, "mean_us": round(t / ev.count, 2), "total_us": round(t, 2)}
    except Exception as e:   # a measurement tool: the step times above stand without the per-kernel split
        note = f"no per-kernel times: {type(e).__name__}: {e}"
    print(json.dumps({"block": block, "shape": shape, "device": torch.cuda.get_device_name(0),
                      "step_us": round(statistics.median(whole), 2), "forward_us": round(statistics.median(fwd), 2),
                      "lookup_us": round(statistics.median(lookup), 2), "step_peak_bytes": int(peak),
                      "kernels": kernels, "kernels_note": note}))


def summarize(recs):
    """Per shape and block: median / min / max over the processes; then the alt / volume ratios of the medians."""
    out = {}
    for shape in SHAPES:
        s = {}
        for block in BLOCKS:
            rs = [r for r in recs if r["shape"] == shape and r["block"] == block]
            if not rs:
                continue
            s[block] = {"processes": len(rs), "kernels": rs[-1]["kernels"]}
            for k in KEYS:
                v = [r[k] for r in rs]
                s[block][k] = {"median": round(statistics.median(v), 2), "min": min(v), "max": max(v)}
        if len(s) == 2:
            for k in KEYS:
                s[f"alt_over_volume_{k}"] = round(s["alt"][k]["median"] / s["volume"][k]["median"], 4)
        if s:
            out[shape] = s
    return out


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--shapes", nargs="+", default=list(SHAPES), choices=list(SHAPES))
    ap.add_argument("--reps", type=int, default=2, help="processes per block and shape")
    ap.add_argument("--steps", type=int, default=5)
    ap.add_argument("--warmup", type=int, default=1)
    ap.add_argument("--child-timeout", type=float, default=240.0, help="seconds per child process")
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "alt_corr", "bench_backward.json"))
    ap.add_argument("--child", nargs=2, metavar=("BLOCK", "SHAPE"), help=argparse.SUPPRESS)
    a = ap.parse_args()
    if a.child:
        return child(a.child[0], a.child[1], a.steps, a.warmup)
    recs = []
    for shape in a.shapes:
        for _ in range(a.reps):
            for block in BLOCKS:   # alternating
                p = subprocess.run([sys.executable, os.path.abspath(__file__), "--child", block, shape, "--steps",
                                    str(a.steps), "--warmup", str(a.warmup)], capture_output=True, text=True,
                                   timeout=a.child_timeout)
                if p.returncode != 0:
                    raise SystemExit(f"bench_alt_backward: {block} / {shape} ended with {p.returncode}:\n{p.stderr[-2000:]}")
                recs.append(json.loads(p.stdout.strip().splitlines()[-1]))
                print(json.dumps(recs[-1]), flush=True)
    doc = {"config": {"D": D, "levels": LEVELS, "radius": RADIUS, "lookups_per_step": LOOKUPS, "steps": a.steps,
                      "shapes": {k: SHAPES[k] for k in a.shapes}},
           "device": recs[0]["device"], "processes": recs, "summary": summarize(recs)}
    os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
    json.dump(doc, open(a.out, "w"), indent=1, sort_keys=True)
    print(json.dumps(doc["summary"]))


if __name__ == "__main__":
    main()
