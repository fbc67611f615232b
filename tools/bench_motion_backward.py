#!/usr/bin/env python3
"""Times and memory of training through lookup + convc1 + ReLU at DSEC size (60 x 80, D = 256, 12
iterations), the new path against the one training had before.  A measurement tool, not a gate;
appends to profiles/motion_backward/bench.json (--out to change), which DESIGN.md §3.3.1 quotes.

Step = CorrBlock build + 12 x (lookup + convc1 + ReLU) + loss + backward, on a differentiable block:
  ours    blk.lookup_conv1x1_relu(coords, w, b)                (ecorr_conv1x1_relu_backward in the backward)
  today   F.relu(F.conv2d(blk(coords), w, b)) under autograd   (MIOpen fp32 convs, TF32 off; corr saved)
HIP events, warm-up, the median of --steps steps; torch.cuda.max_memory_allocated over one step.
Mode `parts` times single C-ABI calls: ecorr_conv1x1_relu_backward with one output each (every call
runs the mask pass, so grad_bias alone = the mask pass + its tiny reduce, and `*_less_mask_us` is a
difference of medians, an estimate), all three, the recompute lookup, ecorr_lookup_backward, and
the forward pair for scale.  FLOPs and algorithmic bytes are computed here from the shapes; the share
of peak is min-time / time with min-time = max(flop / peak rate, bytes / peak bandwidth) against
157.3 TFLOP/s (fp32 MFMA), 3 x as many f16 MFMA flops against 2516 TFLOP/s (dense f16) and 8 TB/s.

One mode per process, each under its own time limit, chained; run the line twice for the spread
(--tag run1 / run2):
  timeout -k 10 300 python tools/bench_motion_backward.py --mode ours --tag run1 && \\
  timeout -k 10 300 python tools/bench_motion_backward.py --mode today --tag run1 && \\
  timeout -k 10 300 python tools/bench_motion_backward.py --mode parts --tag run1
"""
import argparse
import ctypes
import json
import os
import statistics
import sys

import torch
import torch.nn.functional as F

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

H, W, D, LEVELS, RADIUS, ITERS, O = 60, 80, 256, 4, 4, 12, 256
C = LEVELS * (2 * RADIUS + 1) ** 2
PEAK_F32, PEAK_F16, PEAK_BW = 157.3e12, 2516e12, 8.0e12


def inputs(B):
    g = torch.Generator(device="cuda").manual_seed(0)
    f1 = torch.randn((B, D, H, W), generator=g, device="cuda")
    f2 = torch.randn((B, D, H, W), generator=g, device="cuda")
    ys, xs = torch.meshgrid(torch.arange(H, device="cuda", dtype=torch.float32),
                            torch.arange(W, device="cuda", dtype=torch.float32), indexing="ij")
    base = torch.stack([xs, ys])[None].repeat(B, 1, 1, 1)
    smooth = F.avg_pool2d(torch.randn((B, 2, H, W), generator=g, device="cuda") * 9.0, 5, 1, 2)
    coords = [(base + smooth + 0.5 * torch.randn((B, 2, H, W), generator=g, device="cuda")).contiguous()
              for _ in range(ITERS)]
    w = torch.randn((O, C, 1, 1), generator=g, device="cuda") * 0.05
    b = torch.randn((O,), generator=g, device="cuda") * 0.1
    gos = [torch.randn((B, O, H, W), generator=g, device="cuda") for _ in range(2)]
    return f1, f2, coords, w, b, gos


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


def peak_of(fn):
    torch.cuda.synchronize()
    torch.cuda.empty_cache()
    torch.cuda.reset_peak_memory_stats()
    base = torch.cuda.memory_allocated()
    fn()
    torch.cuda.synchronize()
    return torch.cuda.max_memory_allocated() - base


def step(ours, f1, f2, coords, w, b, gos):
    import eraft_amd
    f1, f2, w, b = (t.detach().requires_grad_(True) for t in (f1, f2, w, b))
    blk = eraft_amd.CorrBlock(f1, f2, num_levels=LEVELS, radius=RADIUS, differentiable=True)
    loss = 0.0
    for i, c in enumerate(coords):
        y = blk.lookup_conv1x1_relu(c, w, b) if ours else F.relu(F.conv2d(blk(c), w, b))
        loss = loss + (y * gos[i & 1]).sum()
    loss.backward()
    return f1.grad, f2.grad, w.grad, b.grad


def run_step(ours, B, steps, warmup):
    args = inputs(B)
    ts = timed(lambda: step(ours, *args), steps, warmup)
    peak = peak_of(lambda: step(ours, *args))
    return {"B": B, "steps": steps, "step_us": med(ts), "step_min_us": round(min(ts), 2),
            "step_max_us": round(max(ts), 2), "step_peak_bytes": peak}


def share(us, flop, peak_rate, nbytes):
    t_flop, t_bw = flop / peak_rate * 1e6, nbytes / PEAK_BW * 1e6
    return {"min_us": round(max(t_flop, t_bw), 2), "bound": "compute" if t_flop >= t_bw else "bandwidth",
            "share_of_peak": round(max(t_flop, t_bw) / us, 3)}


def run_parts(B, steps, warmup):
    import eraft_amd
    from eraft_amd import _lib
    f1, f2, coords, w, b, gos = inputs(B)
    L = _lib.lib()
    Q = H * W
    st = ctypes.c_void_p(torch.cuda.current_stream().cuda_stream)
    with torch.no_grad():
        blk = eraft_amd.CorrBlock(f1, f2, num_levels=LEVELS, radius=RADIUS)
        out = blk.lookup_conv1x1_relu(coords[0], w, b, mode="split")
        corr = blk(coords[0])
        n = ctypes.c_int64()
        _lib.check(L.ecorr_conv1x1_relu_backward_workspace_size(B, C, Q, O, ctypes.byref(n)), "size")
        ws = torch.empty(n.value, dtype=torch.uint8, device="cuda")
        pk = _lib.packed_conv1x1_weight(w, O, C, "split_t", st, {})
        gi = torch.empty_like(corr)
        gw, gb = torch.empty((O, C), device="cuda"), torch.empty(O, device="cuda")
        _, _, off = _lib.layout(B * Q, H, W, LEVELS)
        G = torch.zeros(off[-1], device="cuda")
        go = gos[0]

        def bw(a, c, d):
            _lib.check(L.ecorr_conv1x1_relu_backward(
                go.data_ptr(), out.data_ptr(), corr.data_ptr(), pk.data_ptr(), B, C, Q, O,
                None if a is None else a.data_ptr(), None if c is None else c.data_ptr(),
                None if d is None else d.data_ptr(), ws.data_ptr(), st), "conv backward")

        def lookup_bw():
            _lib.check(L.ecorr_lookup_backward(gi.data_ptr(), coords[0].data_ptr(), B, H, W, Q, LEVELS, RADIUS,
                                               G.data_ptr(), st), "lookup backward")
        t_b = med(timed(lambda: bw(None, None, gb), steps, warmup))
        t_i = med(timed(lambda: bw(gi, None, None), steps, warmup))
        t_w = med(timed(lambda: bw(None, gw, None), steps, warmup))
        t_all = med(timed(lambda: bw(gi, gw, gb), steps, warmup))
        t_lk = med(timed(lambda: blk(coords[0]), steps, warmup))
        t_lb = med(timed(lookup_bw, steps, warmup))
        t_fw = med(timed(lambda: blk.lookup_conv1x1_relu(coords[0], w, b, mode="split"), steps, warmup))
    flop = 2 * B * Q * O * C
    act = B * O * Q * 4            # grad_out, out, gm: one [B][O][Q] fp32 tensor each
    cin = B * C * Q * 4            # corr / grad_corr
    def cdiv(a, d):
        return -(-a // d)
    cap = 1024                     # slabs per batch item: conv_grad.hip's conv_grad_layout rule
    while cap > 256 and B * cdiv(Q, cap) * cdiv(O, 256) * cdiv(C, 64) < 480:
        cap //= 2
    slab = cdiv(cdiv(Q, cdiv(Q, cap)), 32) * 32
    nsl = cdiv(Q, slab)
    part = B * nsl * O * C * 4     # weight slab partials, written then read
    return {
        "B": B, "steps": steps, "workspace_bytes": n.value, "slab_queries": slab, "slabs_per_item": nsl,
        "mask_pass_and_bias_us": t_b, "grad_in_incl_mask_us": t_i, "grad_weight_incl_mask_us": t_w,
        "grad_in_less_mask_us": round(t_i - t_b, 2), "grad_weight_and_reduce_less_mask_us": round(t_w - t_b, 2),
        "all_three_us": t_all, "recompute_lookup_us": t_lk, "lookup_backward_us": t_lb,
        "forward_lookup_qmax_plus_split_conv_us": t_fw,
        "flop_each_gemm": flop,
        "mask_pass": dict(algorithmic_bytes=3 * act, **share(t_b, 0, PEAK_F32, 3 * act)),
        "grad_in": dict(algorithmic_bytes=act + cin, f16_mfma_flop=3 * flop,
                        **share(max(t_i - t_b, 1e-3), 3 * flop, PEAK_F16, act + cin)),
        "grad_weight": dict(algorithmic_bytes=act + cin + 2 * part,
                            **share(max(t_w - t_b, 1e-3), flop, PEAK_F32, act + cin + 2 * part)),
    }


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--mode", choices=("ours", "today", "parts"), required=True)
    ap.add_argument("--batch", type=int, default=4)
    ap.add_argument("--steps", type=int, default=20)
    ap.add_argument("--warmup", type=int, default=3)
    ap.add_argument("--tag", default="run1")
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "motion_backward", "bench.json"))
    a = ap.parse_args()
    if not torch.cuda.is_available():
        raise SystemExit("bench_motion_backward: no HIP device (there is no CPU path)")
    torch.backends.cuda.matmul.allow_tf32 = False
    torch.backends.cudnn.allow_tf32 = False
    if a.mode == "parts":
        rec = run_parts(a.batch, a.steps, a.warmup)
    else:
        rec = run_step(a.mode == "ours", a.batch, a.steps, a.warmup)
    os.makedirs(os.path.dirname(a.out), exist_ok=True)
    doc = json.load(open(a.out)) if os.path.exists(a.out) else {}
    doc.setdefault("shape", {"H": H, "W": W, "D": D, "levels": LEVELS, "radius": RADIUS, "iters": ITERS, "O": O})
    doc["device"] = torch.cuda.get_device_name(0)
    doc.setdefault(a.mode, {}).setdefault(f"B{a.batch}", {})[a.tag] = rec
    json.dump(doc, open(a.out, "w"), indent=1, sort_keys=True)
    print(json.dumps({a.mode: {a.tag: rec}}))


if __name__ == "__main__":
    main()
