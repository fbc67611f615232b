#!/usr/bin/env python3
"""Times of 16-bit fmaps in and a 16-bit convc1 output out (CorrBlock(..., fmap_dtype=...),
lookup_conv1x1_relu(..., out_dtype=...)) at DSEC size (60 x 80, D = 256, 4 levels, radius 4; B = 4 and
B = 16, smooth coordinates) against what ERAFT(mixed_precision=True) paid before them: two .float() casts
in front of the build, and an fp32 convc1 output that autocast casts in front of convc2.  A measurement
tool, not a gate; appends one record per process run to profiles/half_io/bench_half_io.json (--out to
change) and recomputes the summary over the runs, which DESIGN.md §3.2.1 quotes.

Per batch size and dtype, HIP events around each Python call, warm-up, median of --steps (>= 20); the
first arm of each row is the yardstick (the path without the feature, in the same run):
  (a) build_cast_<dt>_us         f1.float(); f2.float(); CorrBlock(...)           (16-bit fmaps given)
      build_native_<dt>_us       CorrBlock(f1, f2, fmap_dtype=dt)
  (b) pack_f32_us                the operand pass alone on fp32 fmaps (_lib.stage_events)
      pack_<dt>_us               ... on 16-bit fmaps
  (c) convc1_<mode>_cast_<dt>_us   lookup_conv1x1_relu(coords, w, b, mode).to(dt)
      convc1_<mode>_native_<dt>_us lookup_conv1x1_relu(coords, w, b, mode, out_dtype=dt)
  (d) convc2_<mode>_cast_<dt>_us / convc2_<mode>_native_<dt>_us: row (c) without the explicit cast,
      followed by relu(convc2(.)) under torch.autocast(dtype=dt) (which casts an fp32 input itself)
for mode in split, fused.

One process run measures everything; run it at least three times, each under its own time limit,
chained, for the spread between runs:
  timeout -k 10 300 python tools/bench_half_io.py && \\
  timeout -k 10 300 python tools/bench_half_io.py && \\
  timeout -k 10 300 python tools/bench_half_io.py
"""
import argparse
import json
import os
import statistics
import sys

import torch
import torch.nn.functional as F

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tests"))   # prng: the smooth coordinate field of bench.py

H, W, D, LEVELS, RADIUS = 60, 80, 256, 4, 4
C = LEVELS * (2 * RADIUS + 1) ** 2
DTYPES = {"f16": torch.float16, "bf16": torch.bfloat16}
MODES = ("split", "fused")


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


def timed_pack(make, steps, warmup):
    """The operand pass of the builds `make` runs, from the block's own stage events."""
    from eraft_amd import _lib
    for _ in range(warmup):
        make()
    _lib.stage_events, _lib.stage_event_start = [], True
    try:
        for _ in range(steps):
            make()
        torch.cuda.synchronize()
        ts = [ev[0].elapsed_time(ev[1]) * 1e3 for ev in _lib.stage_events]
    finally:
        _lib.stage_events = None
    return round(statistics.median(ts), 2)


def measure(B, steps, warmup):
    import eraft_amd
    import prng
    g = torch.Generator(device="cuda").manual_seed(B)
    f1 = torch.randn((B, D, H, W), generator=g, device="cuda")
    f2 = torch.randn((B, D, H, W), generator=g, device="cuda")
    coords = torch.from_numpy(prng.coords_smooth(7, B, H, W)).cuda()
    convc1 = torch.nn.Conv2d(C, 256, 1).cuda()
    convc2 = torch.nn.Conv2d(256, 192, 3, padding=1).cuda()
    w, b = convc1.weight.detach(), convc1.bias.detach()
    kw = dict(num_levels=LEVELS, radius=RADIUS)
    q = B * H * W
    rec = {"B": B, "steps": steps, "warmup": warmup,
           "fmap_cast_algorithmic_bytes": 2 * q * D * 6,                     # per pair: read 2, write 4 bytes per element
           "pack_f32_algorithmic_bytes": 2 * q * D * 8, "pack_half_algorithmic_bytes": 2 * q * D * 6,
           "convc1_out_cast_algorithmic_bytes": q * 256 * 6}                 # per iteration
    with torch.no_grad():
        rec["pack_f32_us"] = timed_pack(lambda: eraft_amd.CorrBlock(f1, f2, **kw), steps, warmup)
        corr_fn = eraft_amd.CorrBlock(f1, f2, **kw)
        for tag, dt in DTYPES.items():
            h1, h2 = f1.to(dt), f2.to(dt)
            rec[f"build_cast_{tag}_us"] = timed(lambda: eraft_amd.CorrBlock(h1.float(), h2.float(), **kw), steps, warmup)
            rec[f"build_native_{tag}_us"] = timed(lambda: eraft_amd.CorrBlock(h1, h2, fmap_dtype=dt, **kw), steps, warmup)
            rec[f"pack_{tag}_us"] = timed_pack(lambda: eraft_amd.CorrBlock(h1, h2, fmap_dtype=dt, **kw), steps, warmup)
            del h1, h2

            def c2(x):
                with torch.autocast("cuda", dtype=dt):
                    return F.relu(convc2(x))
            for m in MODES:
                rec[f"convc1_{m}_cast_{tag}_us"] = timed(
                    lambda: corr_fn.lookup_conv1x1_relu(coords, w, b, mode=m).to(dt), steps, warmup)
                rec[f"convc1_{m}_native_{tag}_us"] = timed(
                    lambda: corr_fn.lookup_conv1x1_relu(coords, w, b, mode=m, out_dtype=dt), steps, warmup)
                rec[f"convc2_{m}_cast_{tag}_us"] = timed(
                    lambda: c2(corr_fn.lookup_conv1x1_relu(coords, w, b, mode=m)), steps, warmup)
                rec[f"convc2_{m}_native_{tag}_us"] = timed(
                    lambda: c2(corr_fn.lookup_conv1x1_relu(coords, w, b, mode=m, out_dtype=dt)), steps, warmup)
    return rec


def summarize(runs):
    """Per batch size and timing: the median over the process runs' medians, with their min and max; per
    row the new arm over its yardstick (medians), and whether the new arm's slowest run is within the
    yardstick's fastest-to-slowest spread or faster."""
    out = {}
    for key in sorted({k for r in runs for k in r}):
        recs = [r[key] for r in runs if key in r]
        s = {"runs": len(recs)}
        for name in recs[0]:
            vals = [r[name] for r in recs]
            if name.endswith("_us"):
                s[name] = {"median": round(statistics.median(vals), 2), "min": min(vals), "max": max(vals)}
            elif name.endswith("bytes"):
                s[name] = max(vals)
        pairs = []
        for t in DTYPES:
            pairs += [(f"build_native_{t}_us", f"build_cast_{t}_us"), (f"pack_{t}_us", "pack_f32_us")]
            for m in MODES:
                pairs += [(f"convc1_{m}_native_{t}_us", f"convc1_{m}_cast_{t}_us"),
                          (f"convc2_{m}_native_{t}_us", f"convc2_{m}_cast_{t}_us")]
        for new, base in pairs:
            s[new[:-3] + "_over_" + base[:-3]] = round(s[new]["median"] / s[base]["median"], 3)
            s[new[:-3] + "_not_slower"] = bool(s[new]["median"] <= s[base]["max"])
        out[key] = s
    return out


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--batches", type=int, nargs="+", default=[4, 16])
    ap.add_argument("--steps", type=int, default=30)
    ap.add_argument("--warmup", type=int, default=5)
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "half_io", "bench_half_io.json"))
    a = ap.parse_args()
    if a.steps < 20:
        raise SystemExit("bench_half_io: --steps must be at least 20")
    if not torch.cuda.is_available():
        raise SystemExit("bench_half_io: no HIP device (there is no CPU path)")
    torch.backends.cuda.matmul.allow_tf32 = False
    torch.backends.cudnn.allow_tf32 = False
    run = {f"B{B}": measure(B, a.steps, a.warmup) for B in a.batches}
    os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
    doc = json.load(open(a.out)) if os.path.exists(a.out) else {}
    doc["shape"] = {"H": H, "W": W, "D": D, "levels": LEVELS, "radius": RADIUS, "coords": "prng.coords_smooth(7)"}
    doc["device"] = torch.cuda.get_device_name(0)
    doc.setdefault("runs", []).append(run)
    doc["summary"] = summarize(doc["runs"])
    json.dump(doc, open(a.out, "w"), indent=1, sort_keys=True)
    print(json.dumps(run))


if __name__ == "__main__":
    main()
