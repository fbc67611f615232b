#!/usr/bin/env python3
"""Interleaved A/B of the warm-start splat (ecorr_forward_interpolate, splat.hip) between the tree's
libecorr.so and AB_ALT_LIB lab builds (name=path,...) in one process, on the three 60 x 80 maps of
tools/prof_splat_overflow.py: a smooth DSEC field (B = 16, the list path), the collision map (B = 3,
sub-ranges) and the one-target map (B = 2, the walk).  Reports whether each library's output is
bitwise the tree's, and per map the median, fastest and slowest device time of 10 calls per round
over rotated rounds (HIP events on the call's stream; the C call alone, no Python wrapper).  The
overflow paths are serial loops of a few instructions, and their time moves by several percent with
where the loop falls in the code (profiles/event_kernels/timing.txt): compare builds of one tree
through this tool, not figures across trees."""
import ctypes
import json
import os
import statistics
import sys

import numpy as np
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
import eraft_amd  # noqa: E402,F401
from eraft_amd import _lib  # noqa: E402

LIBS = {"tree": _lib.lib()}
for item in filter(None, os.environ.get("AB_ALT_LIB", "").split(",")):
    name, _, path = item.rpartition("=")
    L = ctypes.CDLL(os.path.join(ROOT, path))
    for sym, (res, args) in _lib.SYMBOLS.items():
        if hasattr(L, sym):
            getattr(L, sym).restype = res
            getattr(L, sym).argtypes = args
    LIBS[name] = L

h, w = 60, 80
yy, xx = np.mgrid[0:h, 0:w].astype(np.float32)
maps = {
    "smooth_b16": (np.random.default_rng(0).standard_normal((16, 2, h, w)) * 1.5).astype(np.float32),
    "collisions_b3": np.repeat(np.stack([(40.25 - xx) * 0.99, (30.5 - yy) * 0.99])[None], 3, axis=0),
    "one_target_b2": np.repeat(np.stack([40.0 - xx, 30.0 - yy])[None], 2, axis=0),
}
res = {}
names = list(LIBS)
with torch.no_grad():
    for mname, m in maps.items():
        flow = torch.from_numpy(np.ascontiguousarray(m, dtype=np.float32)).cuda()
        B = flow.shape[0]
        out = torch.empty_like(flow)
        st = _lib.stream_of(flow)

        def run(nm):
            _lib.check(LIBS[nm].ecorr_forward_interpolate(flow.data_ptr(), B, h, w, out.data_ptr(), None, st), nm)

        run("tree")
        torch.cuda.synchronize()
        base = out.clone()
        times = {nm: [] for nm in names}
        same = {}
        for nm in names:
            out.fill_(float("nan"))
            run(nm)
            torch.cuda.synchronize()
            same[nm] = bool(torch.equal(out.view(torch.int32), base.view(torch.int32)))
        for rnd in range(4):
            for nm in names[rnd % len(names):] + names[:rnd % len(names)]:
                for _ in range(3):
                    run(nm)
                ev = [torch.cuda.Event(enable_timing=True) for _ in range(11)]
                ev[0].record()
                for i in range(10):
                    run(nm)
                    ev[i + 1].record()
                torch.cuda.synchronize()
                times[nm] += [ev[i].elapsed_time(ev[i + 1]) * 1e3 for i in range(10)]
        res[mname] = {nm: {"bitwise": same[nm], "us_median": round(statistics.median(ts), 1), "us_min": round(min(ts), 1),
                           "us_max": round(max(ts), 1)} for nm, ts in times.items()}
print(json.dumps({"probe": "ab_splat forward_interpolate 60x80, C call", "maps": res}))
