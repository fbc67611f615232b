#!/usr/bin/env python3
"""What the volume-free lookup costs and saves: AlternateCorrBlock against CorrBlock from the same tree,
at D = 256, 4 levels, radius 4 on DSEC's 60 x 80 map (B = 1, 4, 16) and on a 92 x 160 map (a 720p sensor,
B = 4).  A measurement tool, not a gate; writes profiles/alt_corr/bench.json (--out to change), which
DESIGN.md §3.10 and the README quote.

Every measurement runs in a process of its own (one block, one shape), started one after the other by
this parent, which never touches the GPU: per shape the two blocks alternate (alt, volume, alt, volume,
...), --reps times each, and the summary is the median over a block's processes with their min and max.
Per process, HIP events around the Python calls, after a warm-up, medians of --steps:
  construct_us   the constructor: AlternateCorrBlock's pack (transpose + pooled fmap2 levels), or
                 CorrBlock's build (operand pass + GEMM with the fused pyramid)
  lookup_us      one corr_fn(coords) call (sigma-2 flow on the grid)
  step_us        construction + 12 lookups: what one E-RAFT forward asks of the block
  step_peak_bytes  torch.cuda.max_memory_allocated over one step, above what was allocated before it
                 (fmaps and coords excluded, the block and one lookup output included)
A child that fails ends the run: nothing more is started on the GPU after it.
"""
import argparse
import json
import os
import statistics
import subprocess
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))

D, LEVELS, RADIUS, LOOKUPS = 256, 4, 4, 12
SHAPES = {"dsec_b1": (1, 60, 80), "dsec_b4": (4, 60, 80), "dsec_b16": (16, 60, 80), "hd_92x160_b4": (4, 92, 160)}
BLOCKS = ("alt", "volume")


def child(block, shape, steps, warmup):
    import torch
    sys.path.insert(0, ROOT)
    import eraft_amd
    if not torch.cuda.is_available():
        raise SystemExit("bench_alt_corr: no HIP device (there is no CPU path)")
    B, H, W = SHAPES[shape]
    cls = eraft_amd.AlternateCorrBlock if block == "alt" else eraft_amd.CorrBlock
    g = torch.Generator(device="cuda").manual_seed(B * H)
    f1 = torch.randn((B, D, H, W), generator=g, device="cuda")
    f2 = torch.randn((B, D, H, W), generator=g, device="cuda")
    coords = eraft_amd.coords_grid(B, H, W, device="cuda") + 2.0 * torch.randn((B, 2, H, W), generator=g, device="cuda")

    def timed(fn):
        e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        e0.record()
        r = fn()
        e1.record()
        e1.synchronize()
        return e0.elapsed_time(e1) * 1e3, r

    def step():
        fn = cls(f1, f2, num_levels=LEVELS, radius=RADIUS)
        for _ in range(LOOKUPS):
            out = fn(coords)
        return out

    with torch.no_grad():
        for _ in range(warmup):
            step()
        construct, lookup, whole = [], [], []
        for _ in range(steps):
            t, fn = timed(lambda: cls(f1, f2, num_levels=LEVELS, radius=RADIUS))
            construct.append(t)
            for _ in range(3):
                lookup.append(timed(lambda: fn(coords))[0])
            del fn
            whole.append(timed(step)[0])
        torch.cuda.synchronize()
        torch.cuda.empty_cache()
        torch.cuda.reset_peak_memory_stats()
        base = torch.cuda.memory_allocated()
        step()
        torch.cuda.synchronize()
        peak = torch.cuda.max_memory_allocated() - base
    print(json.dumps({"block": block, "shape": shape, "device": torch.cuda.get_device_name(0),
                      "construct_us": round(statistics.median(construct), 2),
                      "lookup_us": round(statistics.median(lookup), 2),
                      "step_us": round(statistics.median(whole), 2), "step_peak_bytes": int(peak)}))


def summarize(recs):
    """Per shape and block: median / min / max over the processes; then the alt / volume ratios of the medians."""
    out = {}
    for shape in SHAPES:
        s = {}
        for block in BLOCKS:
            rs = [r for r in recs if r["shape"] == shape and r["block"] == block]
            if not rs:
                continue
            s[block] = {"processes": len(rs)}
            for k in ("construct_us", "lookup_us", "step_us", "step_peak_bytes"):
                v = [r[k] for r in rs]
                s[block][k] = {"median": round(statistics.median(v), 2), "min": min(v), "max": max(v)}
        if len(s) == 2:
            for k in ("construct_us", "lookup_us", "step_us", "step_peak_bytes"):
                s[f"alt_over_volume_{k}"] = round(s["alt"][k]["median"] / s["volume"][k]["median"], 4)
        if s:
            out[shape] = s
    return out


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--shapes", nargs="+", default=list(SHAPES), choices=list(SHAPES))
    ap.add_argument("--reps", type=int, default=2, help="processes per block and shape")
    ap.add_argument("--steps", type=int, default=10)
    ap.add_argument("--warmup", type=int, default=2)
    ap.add_argument("--child-timeout", type=float, default=240.0, help="seconds per child process")
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "alt_corr", "bench.json"))
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
                    raise SystemExit(f"bench_alt_corr: {block} / {shape} ended with {p.returncode}:\n{p.stderr[-2000:]}")
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
