#!/usr/bin/env python3
"""Times of the 16-bit lookup output (ecorr_lookup_as, CorrBlock.__call__(coords, out_dtype=...)) at
DSEC size (60 x 80, D = 256, 4 levels, radius 4; B = 4 and B = 16, smooth coordinates) against what a
mixed-precision consumer pays without it: the fp32 lookup followed by an ATen cast.  A measurement
tool, not a gate; appends one record per process run to profiles/half_out/bench_lookup_half.json
(--out to change) and recomputes the summary over the runs, which DESIGN.md §3.2.1 quotes.

Per batch size, HIP events around each call, warm-up, median of --steps (>= 20):
  lookup_f32_us                 corr_fn(coords)
  lookup_f32_cast_<dt>_us       corr_fn(coords).to(dt): the lookup + the cast autocast makes for convc1
  lookup_<dt>_us                corr_fn(coords, out_dtype=dt)
  convc1_after_f32_<dt>_us      corr_fn(coords), then relu(convc1(.)) under torch.autocast(dtype=dt)
  convc1_after_<dt>_us          corr_fn(coords, out_dtype=dt), then the same convc1
Algorithmic bytes per lookup, from the shapes: the output (324 channels of 4 or 2 bytes per query), the
(2r+2)^2 window of every query and level (fp32) and the coordinates; the share of the HBM roofline is
those bytes at 8 TB/s over the measured time.
And ERAFT.forward at B = 1 (480 x 640 events, 15 bins, 12 iterations, default-initialised weights):
  eraft_fp32_us, eraft_mixed_cast_<dt>_us (_native_half_lookup=False), eraft_mixed_native_<dt>_us.

One process run measures everything; run it at least three times, each under its own time limit,
chained, for the spread between runs:
  timeout -k 10 400 python tools/bench_lookup_half.py && \\
  timeout -k 10 400 python tools/bench_lookup_half.py && \\
  timeout -k 10 400 python tools/bench_lookup_half.py
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
HBM_PEAK = 8.0e12   # bytes / s (spec)
DTYPES = {"f16": torch.float16, "bf16": torch.bfloat16}


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


def lookup_bytes(B, elem):
    q = B * H * W
    return q * (C * elem + LEVELS * (2 * RADIUS + 2) ** 2 * 4 + 8)


def measure_lookup(B, steps, warmup):
    import eraft_amd
    import prng
    g = torch.Generator(device="cuda").manual_seed(B)
    f1 = torch.randn((B, D, H, W), generator=g, device="cuda")
    f2 = torch.randn((B, D, H, W), generator=g, device="cuda")
    corr_fn = eraft_amd.CorrBlock(f1, f2, num_levels=LEVELS, radius=RADIUS)
    del f1, f2
    coords = torch.from_numpy(prng.coords_smooth(7, B, H, W)).cuda()
    convc1 = torch.nn.Conv2d(C, 256, 1).cuda()
    rec = {"B": B, "steps": steps, "warmup": warmup,
           "lookup_f32_algorithmic_bytes": lookup_bytes(B, 4), "lookup_half_algorithmic_bytes": lookup_bytes(B, 2),
           "cast_algorithmic_bytes": B * H * W * C * 6}
    with torch.no_grad():
        rec["lookup_f32_us"] = timed(lambda: corr_fn(coords), steps, warmup)
        for tag, dt in DTYPES.items():
            def conv(x):
                with torch.autocast("cuda", dtype=dt):
                    return F.relu(convc1(x))
            rec[f"lookup_f32_cast_{tag}_us"] = timed(lambda: corr_fn(coords).to(dt), steps, warmup)
            rec[f"lookup_{tag}_us"] = timed(lambda: corr_fn(coords, out_dtype=dt), steps, warmup)
            rec[f"convc1_after_f32_{tag}_us"] = timed(lambda: conv(corr_fn(coords)), steps, warmup)
            rec[f"convc1_after_{tag}_us"] = timed(lambda: conv(corr_fn(coords, out_dtype=dt)), steps, warmup)
    return rec


def measure_eraft(steps, warmup):
    from eraft_amd.network import ERAFT
    g = torch.Generator(device="cuda").manual_seed(1)
    im1 = torch.randn((1, 15, 480, 640), generator=g, device="cuda")
    im2 = torch.randn((1, 15, 480, 640), generator=g, device="cuda")
    rec = {"B": 1, "steps": steps, "warmup": warmup}

    def arm(**kw):
        torch.manual_seed(0)
        net = ERAFT({"subtype": "standard"}, n_first_channels=15, **kw).cuda().eval()
        with torch.no_grad():
            return timed(lambda: net(im1, im2, iters=12), steps, warmup)
    rec["eraft_fp32_us"] = arm()
    for tag, dt in DTYPES.items():
        rec[f"eraft_mixed_cast_{tag}_us"] = arm(mixed_precision=True, amp_dtype=dt, _native_half_lookup=False)
        rec[f"eraft_mixed_native_{tag}_us"] = arm(mixed_precision=True, amp_dtype=dt)
    return rec


def summarize(runs):
    """Per record and timing: the median over the process runs' medians, with their min and max."""
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
        if key.startswith("B"):
            for name, nbytes in [("lookup_f32", "lookup_f32_algorithmic_bytes")] + \
                                [(f"lookup_{t}", "lookup_half_algorithmic_bytes") for t in DTYPES]:
                rate = s[nbytes] / (s[f"{name}_us"]["median"] * 1e-6)
                s[f"{name}_bytes_per_s"] = round(rate, -9)
                s[f"{name}_hbm_roofline_share"] = round(rate / HBM_PEAK, 3)
            for t in DTYPES:
                s[f"lookup_{t}_over_f32"] = round(s[f"lookup_{t}_us"]["median"] / s["lookup_f32_us"]["median"], 3)
                s[f"lookup_{t}_over_f32_cast"] = round(
                    s[f"lookup_{t}_us"]["median"] / s[f"lookup_f32_cast_{t}_us"]["median"], 3)
                s[f"convc1_after_{t}_over_after_f32"] = round(
                    s[f"convc1_after_{t}_us"]["median"] / s[f"convc1_after_f32_{t}_us"]["median"], 3)
        else:
            for t in DTYPES:
                s[f"mixed_native_{t}_over_fp32"] = round(
                    s[f"eraft_mixed_native_{t}_us"]["median"] / s["eraft_fp32_us"]["median"], 3)
                s[f"mixed_native_{t}_over_mixed_cast"] = round(
                    s[f"eraft_mixed_native_{t}_us"]["median"] / s[f"eraft_mixed_cast_{t}_us"]["median"], 3)
        out[key] = s
    return out


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--batches", type=int, nargs="+", default=[4, 16])
    ap.add_argument("--steps", type=int, default=30)
    ap.add_argument("--warmup", type=int, default=5)
    ap.add_argument("--no-eraft", action="store_true", help="skip the ERAFT.forward arms")
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "half_out", "bench_lookup_half.json"))
    a = ap.parse_args()
    if a.steps < 20:
        raise SystemExit("bench_lookup_half: --steps must be at least 20")
    if not torch.cuda.is_available():
        raise SystemExit("bench_lookup_half: no HIP device (there is no CPU path)")
    torch.backends.cuda.matmul.allow_tf32 = False
    torch.backends.cudnn.allow_tf32 = False
    run = {f"B{B}": measure_lookup(B, a.steps, a.warmup) for B in a.batches}
    if not a.no_eraft:
        run["eraft_B1"] = measure_eraft(a.steps, a.warmup)
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
