#!/usr/bin/env python3
"""What the hi-only split build (ECORR_BUILD_HI, ecorr_build_split_pack_hi_as / _gemm_hi) buys for 16-bit
fmaps at DSEC size (60 x 80, D = 256, 4 levels; B = 4 and B = 16; float16 and bfloat16).  A measurement
tool, not a gate; appends one record per process run to profiles/hi_build/bench_hi_build.json (--out to
change) and recomputes the summary over the runs, which DESIGN.md §3.1 / §3.2.1 quote and which decides
the switch's default (the rule is in `summarize`).

Arms, alternating step by step in the same process (off, on, flagged, off, on, ...):
  off      CorrBlock(f1, f2, fmap_dtype=dt) with the switch off: the plain entries, the yardstick
  on       ... with the switch on: flag 0, the one-term K loop
  flagged  ... with the switch on and one NaN pixel in fmap2: flag 1, the three-term K loop -- what the
           memset, the flag stores and the idle kernel launch cost when the one-term loop cannot run
Per arm: HIP events around the Python call (build_*_us), warm-up, median of --steps (>= 30); then, in a
second alternated pass, the operand pass and the GEMM apart from the block's own stage events
(pack_*_us: memset + pass; gemm_*_us: both kernels of the hi form).

One process run measures everything; run it three times, each under its own time limit, chained:
  timeout -k 10 300 python tools/bench_hi_build.py && \\
  timeout -k 10 300 python tools/bench_hi_build.py && \\
  timeout -k 10 300 python tools/bench_hi_build.py
"""
import argparse
import json
import os
import statistics
import sys

import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

H, W, D, LEVELS, RADIUS = 60, 80, 256, 4, 4
DTYPES = {"f16": torch.float16, "bf16": torch.bfloat16}
ARMS = ("off", "on", "flagged")


def measure(B, dt, steps, warmup):
    import eraft_amd
    from eraft_amd import _lib
    g = torch.Generator(device="cuda").manual_seed(B)
    f1 = torch.randn((B, D, H, W), generator=g, device="cuda").to(dt)
    f2 = torch.randn((B, D, H, W), generator=g, device="cuda").to(dt)
    f2_nan = f2.clone()
    f2_nan[0, 3, 5, 7] = float("nan")
    kw = dict(num_levels=LEVELS, radius=RADIUS, fmap_dtype=dt)
    arms = {"off": (False, f2), "on": (True, f2), "flagged": (True, f2_nan)}
    before = _lib.build_hi()

    def build(arm):
        on, tgt = arms[arm]
        _lib.set_build_hi(on)
        return eraft_amd.CorrBlock(f1, tgt, **kw)

    rec = {}
    try:
        with torch.no_grad():
            for _ in range(warmup):
                for arm in ARMS:
                    build(arm)
            whole = {arm: [] for arm in ARMS}
            for _ in range(steps):
                for arm in ARMS:
                    e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
                    e0.record()
                    build(arm)
                    e1.record()
                    e1.synchronize()
                    whole[arm].append(e0.elapsed_time(e1) * 1e3)
            stages = {arm: [] for arm in ARMS}
            _lib.stage_events, _lib.stage_event_start = [], True
            try:
                for _ in range(steps):
                    for arm in ARMS:
                        build(arm)
                torch.cuda.synchronize()
                for i, ev in enumerate(_lib.stage_events):
                    stages[ARMS[i % len(ARMS)]].append((ev[0].elapsed_time(ev[1]) * 1e3, ev[1].elapsed_time(ev[2]) * 1e3))
            finally:
                _lib.stage_events = None
    finally:
        _lib.set_build_hi(before)
    for arm in ARMS:
        rec[f"build_{arm}_us"] = round(statistics.median(whole[arm]), 2)
        rec[f"pack_{arm}_us"] = round(statistics.median(p for p, _ in stages[arm]), 2)
        rec[f"gemm_{arm}_us"] = round(statistics.median(m for _, m in stages[arm]), 2)
    return rec


def summarize(runs):
    """Per (batch, dtype) and timing: the median over the process runs' medians with their min and max.
    The default's rule, per dtype and over both: on by default for 16-bit fmaps if, in EVERY run, the
    B = 16 whole-build median with the switch on is below the off arm's by more than the off arm's own
    min-max spread over the runs, and at B = 4 it is not slower by more than that spread."""
    out = {}
    keys = sorted({k for r in runs for k in r})
    for key in keys:
        recs = [r[key] for r in runs if key in r]
        s = {"runs": len(recs)}
        for name in recs[0]:
            vals = [r[name] for r in recs]
            s[name] = {"median": round(statistics.median(vals), 2), "min": min(vals), "max": max(vals)}
        s["build_off_spread_us"] = round(s["build_off_us"]["max"] - s["build_off_us"]["min"], 2)
        s["build_on_over_off"] = round(s["build_on_us"]["median"] / s["build_off_us"]["median"], 3)
        s["build_flagged_over_off"] = round(s["build_flagged_us"]["median"] / s["build_off_us"]["median"], 3)
        s["gemm_on_over_off"] = round(s["gemm_on_us"]["median"] / s["gemm_off_us"]["median"], 3)
        spread = s["build_off_spread_us"]
        if key.startswith("B16_"):
            s["rule_met_in_every_run"] = all(r["build_on_us"] < r["build_off_us"] - spread for r in recs)
        elif key.startswith("B4_"):
            s["rule_met_in_every_run"] = all(r["build_on_us"] <= r["build_off_us"] + spread for r in recs)
        out[key] = s
    ruled = [out[k]["rule_met_in_every_run"] for k in keys if "rule_met_in_every_run" in out[k]]
    complete = all(f"B{b}_{t}" in out for b in (4, 16) for t in DTYPES) and min(out[k]["runs"] for k in keys) >= 3
    out["default_on"] = bool(complete and all(ruled))
    return out


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--batches", type=int, nargs="+", default=[4, 16])
    ap.add_argument("--steps", type=int, default=30)
    ap.add_argument("--warmup", type=int, default=5)
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "hi_build", "bench_hi_build.json"))
    a = ap.parse_args()
    if a.steps < 30:
        raise SystemExit("bench_hi_build: --steps must be at least 30")
    if not torch.cuda.is_available():
        raise SystemExit("bench_hi_build: no HIP device (there is no CPU path)")
    run = {f"B{B}_{tag}": measure(B, dt, a.steps, a.warmup) for B in a.batches for tag, dt in DTYPES.items()}
    os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
    doc = json.load(open(a.out)) if os.path.exists(a.out) else {}
    doc["shape"] = {"H": H, "W": W, "D": D, "levels": LEVELS}
    doc["device"] = torch.cuda.get_device_name(0)
    doc.setdefault("runs", []).append(run)
    doc["summary"] = summarize(doc["runs"])
    json.dump(doc, open(a.out, "w"), indent=1, sort_keys=True)
    print(json.dumps(run))


if __name__ == "__main__":
    main()
