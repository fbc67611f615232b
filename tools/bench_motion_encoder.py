#!/usr/bin/env python3
"""What the HIP motion encoder costs: eraft_amd.motion_encoder (csrc/motion_enc.hip, fp32 MFMA) against
network.BasicMotionEncoder.forward(flow, c1, corr_is_convc1=True) on MIOpen fp32 with TF32 off (the default path:
four convolutions and two torch.cat).  A measurement tool, not a gate; writes profiles/motion_encoder/bench.json
(--out to change), which DESIGN.md §3.12 and the README quote.  It fails without a HIP device: there is no
fallback.

Shapes: DSEC's 60 x 80 map at B = 1 and B = 16, MVSEC's 32 x 32 map at B = 64, a 92 x 160 map at B = 4.
Per shape the two arms alternate call by call in one process (miopen, hip, miopen, hip, ...): HIP events
around each call, --warmup (>= 5) unrecorded rounds, then the median of --steps (>= 20) with min and max
(the spread) per arm.  Derived per arm: ms per call, fp32-equivalent TFLOP/s at 1,637,888 flop per pixel
(2 x (192 x 256 x 9 + 128 x 2 x 49 + 64 x 128 x 9 + 126 x 256 x 9)), and for the hip arm the share of the
157.3 TFLOP/s fp32-MFMA roof, the instruction it runs on.  Inputs: c1 = relu(normal), flow = 3 * normal,
default-scale random weights.

End to end (--e2e-steps, default 5; 0 to skip): the ERAFT forward at DSEC 480 x 640, 15 bins, B = 16, 12
iterations with fuse_motion_corr, hip_upsample and hip_gru, with and without hip_motion_encoder, alternating,
the same --warmup rounds, median; its weights are the PRNG weights of tests/e2e_weights.py, as in bench.py's
end-to-end arm.

--trace-only runs ten motion_encoder calls at DSEC B = 16 and nothing else: the program of a
`rocprofv3 --kernel-trace --stats` run of its own (per-kernel times; profiles/motion_encoder/).
"""
import argparse
import json
import os
import statistics
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))

FLOP_PER_PIXEL = 2 * (192 * 256 * 9 + 128 * 2 * 49 + 64 * 128 * 9 + 126 * 256 * 9)   # 1,637,888
FP32_MFMA_TFLOPS = 157.3
SHAPES = {"dsec_b1": (1, 60, 80), "dsec_b16": (16, 60, 80), "mvsec_b64": (64, 32, 32), "hd_92x160_b4": (4, 92, 160)}


def timed(torch, fn):
    e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    e0.record()
    fn()
    e1.record()
    e1.synchronize()
    return e0.elapsed_time(e1)


def stats(ms, pixels):
    med = statistics.median(ms)
    return {"ms": round(med, 4), "ms_min": round(min(ms), 4), "ms_max": round(max(ms), 4), "calls": len(ms),
            "tflops_fp32_equiv": round(FLOP_PER_PIXEL * pixels / (med * 1e-3) / 1e12, 2)}


def make_encoder(torch, nw):
    torch.manual_seed(7)
    return nw.BasicMotionEncoder().cuda().eval().requires_grad_(False)


def make_inputs(torch, B, H, W):
    g = torch.Generator(device="cuda").manual_seed(B * H + W)
    c1 = torch.relu(torch.randn((B, 256, H, W), generator=g, device="cuda"))
    flow = 3 * torch.randn((B, 2, H, W), generator=g, device="cuda")
    return flow, c1


def bench_shape(torch, eraft_amd, enc, shape, steps, warmup):
    B, H, W = SHAPES[shape]
    flow, c1 = make_inputs(torch, B, H, W)
    arms = {"miopen": lambda: enc(flow, c1, corr_is_convc1=True), "hip": lambda: eraft_amd.motion_encoder(flow, c1, enc)}
    ms = {k: [] for k in arms}
    with torch.no_grad():
        for i in range(warmup + steps):
            for k, fn in arms.items():   # alternating
                t = timed(torch, fn)
                if i >= warmup:
                    ms[k].append(t)
        err = float((arms["hip"]() - arms["miopen"]()).abs().max())
    rec = {k: stats(v, B * H * W) for k, v in ms.items()}
    rec["hip"]["share_of_fp32_mfma_roof"] = round(rec["hip"]["tflops_fp32_equiv"] / FP32_MFMA_TFLOPS, 4)
    rec["hip_over_miopen_ms"] = round(rec["hip"]["ms"] / rec["miopen"]["ms"], 4)
    # the gap counts only where the two arms' ranges do not overlap
    rec["ranges_disjoint"] = bool(rec["hip"]["ms_max"] < rec["miopen"]["ms_min"] or
                                  rec["miopen"]["ms_max"] < rec["hip"]["ms_min"])
    rec["max_abs_difference"] = err
    rec["B_H_W"] = [B, H, W]
    return rec


def bench_e2e(torch, nw, steps, warmup, B=16):
    sys.path.insert(0, os.path.join(ROOT, "tests"))
    from e2e_weights import make_state_dict   # as bench.py's end-to-end arm: the PRNG weights, finite flows
    nets = {}
    for k, flag in (("miopen_encoder", False), ("hip_encoder", True)):
        net = nw.ERAFT({"subtype": "warm_start"}, n_first_channels=15, fuse_motion_corr=True, hip_upsample=True,
                       hip_gru=True, hip_motion_encoder=flag)
        net.load_state_dict(make_state_dict(net.state_dict()))
        nets[k] = net.cuda().eval()
    g = torch.Generator(device="cuda").manual_seed(3)
    im1 = torch.randn((B, 15, 480, 640), generator=g, device="cuda")
    im2 = torch.randn((B, 15, 480, 640), generator=g, device="cuda")
    ms = {k: [] for k in nets}
    with torch.no_grad():
        for i in range(steps + warmup):
            for k, net in nets.items():   # alternating
                t = timed(torch, lambda: net(im1, im2, iters=12))
                if i >= warmup:
                    ms[k].append(t)
    rec = {k: {"ms": round(statistics.median(v), 3), "ms_min": round(min(v), 3), "ms_max": round(max(v), 3),
               "calls": len(v)} for k, v in ms.items()}
    rec["config"] = (f"DSEC 480x640, 15 bins, batch {B}, 12 iterations, fuse_motion_corr + hip_upsample + hip_gru, "
                     "PRNG weights")
    rec["protocol"] = f"alternating arms, {warmup} warm-up rounds, median of {steps}, HIP events, TF32 off"
    rec["hip_over_miopen_ms"] = round(rec["hip_encoder"]["ms"] / rec["miopen_encoder"]["ms"], 4)
    rec["ranges_disjoint"] = bool(rec["hip_encoder"]["ms_max"] < rec["miopen_encoder"]["ms_min"] or
                                  rec["miopen_encoder"]["ms_max"] < rec["hip_encoder"]["ms_min"])
    return rec


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--shapes", nargs="+", default=list(SHAPES), choices=list(SHAPES))
    ap.add_argument("--steps", type=int, default=20)
    ap.add_argument("--warmup", type=int, default=5)
    ap.add_argument("--e2e-steps", type=int, default=5)
    ap.add_argument("--trace-only", action="store_true")
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "motion_encoder", "bench.json"))
    a = ap.parse_args()
    if a.steps < 20 or a.warmup < 5:
        raise SystemExit("bench_motion_encoder: --steps >= 20 and --warmup >= 5")
    import torch
    sys.path.insert(0, ROOT)
    import eraft_amd
    from eraft_amd import network as nw
    if not torch.cuda.is_available():
        raise SystemExit("bench_motion_encoder: no HIP device (there is no CPU path)")
    torch.backends.cuda.matmul.allow_tf32 = False
    torch.backends.cudnn.allow_tf32 = False
    enc = make_encoder(torch, nw)
    if a.trace_only:
        flow, c1 = make_inputs(torch, *SHAPES["dsec_b16"])
        with torch.no_grad():
            for _ in range(10):
                eraft_amd.motion_encoder(flow, c1, enc)
        torch.cuda.synchronize()
        return
    doc = {"device": torch.cuda.get_device_name(0), "flop_per_pixel": FLOP_PER_PIXEL,
           "roof": f"fp32 MFMA (v_mfma_f32_32x32x2_f32), {FP32_MFMA_TFLOPS} TFLOP/s",
           "protocol": f"alternating arms, {a.warmup} warm-up rounds, median of {a.steps}, HIP events, TF32 off",
           "source_digest": eraft_amd._lib.source_digest(), "shapes": {}}
    for shape in a.shapes:
        doc["shapes"][shape] = bench_shape(torch, eraft_amd, enc, shape, a.steps, a.warmup)
        print(shape, json.dumps(doc["shapes"][shape]), flush=True)
    if a.e2e_steps > 0:
        doc["e2e_dsec_b16"] = bench_e2e(torch, nw, a.e2e_steps, a.warmup)
        print("e2e", json.dumps(doc["e2e_dsec_b16"]), flush=True)
    os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
    json.dump(doc, open(a.out, "w"), indent=1, sort_keys=True)


if __name__ == "__main__":
    main()
