"""Cases of the splat's dispatch tests (csrc/splat.hip) and a plain Python mirror of its dispatch: test
infrastructure, numpy only.  Shared by tests/test_dispatch_mirrors.py (on the CPU: the mirror's
constants against the source, every branch covered) and tests/test_splat_dispatch_gpu.py.

launch_splat takes the banded kernel (splat_band_kernel, G bands of targets per item, one workgroup
each) for n <= kBandMaxN points per item, else splat_kernel, one workgroup per item with its
keys -- and, past kLdsTargets targets, its counts -- in the caller's workspace.  The banded kernel
stages an item's points in LDS while they fit kBandPts floats (16-byte loads where the item's pointer
is 16-byte aligned, else scalar ones), serves a band whose contributions fit kBandCap from its LDS
list, and otherwise walks sub-ranges of targets (re-evaluating every point per sub-range), a single
target past kBandCap folded by one wave walking all contributions (fold_walk).
"""
import numpy as np

import prng

# csrc/splat.hip (tests/test_dispatch_mirrors.py holds these to the source)
kBandMaxN = 65536
kBandPts = 10240
kBandCap = 6144
kBandTargets = 2048
kLdsTargets = 16384

BRANCHES = (
    "large.flow", "large.points", "large.batch", "large.counts_ws", "large.counts_lds",
    "band.flow.n_max", "large.flow.n_min", "band.points.n_max", "large.points.n_min",
    "band.list", "band.subrange.valid", "band.walk.valid",
    "band.staged.aligned", "band.staged.scalar", "band.staged.last", "band.unstaged",
    "points.n0", "points.n1",
)


# ---- the mirror -------------------------------------------------------------------------------------

def kernel(n):
    """band_mode"""
    return "band" if n <= kBandMaxN else "large"


def workspace_needed(n):
    """splat_workspace_bytes > 0: the large-map kernel's keys."""
    return kernel(n) == "large"


def counts(hw):
    """splat_kernel: cnt = hw <= kLdsTargets ? pool : ws_count"""
    return "lds" if hw <= kLdsTargets else "ws"


def staged(flow, n):
    """splat_band_kernel: NP * n <= kBandPts"""
    return (2 if flow else 3) * n <= kBandPts


def staging(flow, n, b):
    """The staging arm of item b (the batch's pointer 16-byte aligned): its pointer's own alignment."""
    return "aligned" if (b * (2 if flow else 3) * n * 4) % 16 == 0 else "scalar"


def band_count(B, hw):
    need = (hw + kBandTargets - 1) // kBandTargets
    g = max(256 // B, need)
    return max(1, min(g, hw))


def positions(flow, data, h, w):
    """(x, y) float32 [B, n] as point<FLOW> makes them."""
    data = np.asarray(data, dtype=np.float32)
    if not flow:
        return data[0][None], data[1][None]
    B = data.shape[0]
    yy, xx = np.mgrid[0:h, 0:w].astype(np.float32)
    return (xx[None] + data[:, 0]).reshape(B, -1), (yy[None] + data[:, 1]).reshape(B, -1)


def target_counts(x, y, h, w):
    """Contributions per target of one item: target_of over the four passes."""
    cnt = np.zeros(h * w, dtype=np.int64)
    with np.errstate(invalid="ignore"):
        for xv in (np.floor(x), np.ceil(x)):
            for yv in (np.floor(y), np.ceil(y)):
                ok = (xv < np.float32(w)) & (xv >= 0) & (yv < np.float32(h)) & (yv >= 0)
                t = (xv[ok] + np.float32(w) * yv[ok]).astype(np.int64)
                np.add.at(cnt, t, 1)
    return cnt


def band_paths(flow, data, h, w):
    """Which of the banded kernel's fold paths the data takes: {"list", "subrange", "walk"}."""
    x, y = positions(flow, data, h, w)
    B, hw = x.shape[0], h * w
    G = band_count(B, hw)
    out = set()
    for b in range(B):
        cnt = target_counts(x[b], y[b], h, w)
        for band in range(G):
            c = cnt[band * hw // G:(band + 1) * hw // G]
            if c.sum() <= kBandCap:
                out.add("list")
                continue
            a = 0   # the overflow path's greedy sub-ranges
            while a < c.size:
                e = a + 1
                while e < c.size and c[a:e + 1].sum() <= kBandCap:
                    e += 1
                if c[a:e].sum() > kBandCap:
                    out.add("walk")
                elif c[a:e].sum() > 0:
                    out.add("subrange")
                a = e
    return out


def tags(name):
    """The branches of BRANCHES the mirror says the case takes."""
    c = CASES[name]
    flow, B, n, h, w = c["mode"] == "flow", c["B"], c["n"], c["h"], c["w"]
    out = set()
    if kernel(n) == "large":
        out |= {"large.flow" if flow else "large.points", "large.counts_" + counts(h * w)}
        if B > 1:
            out.add("large.batch")
        if n == kBandMaxN + 1 or (flow and n - w < kBandMaxN + 1):   # flow: the first whole map past the switch
            out.add("large.flow.n_min" if flow else "large.points.n_min")
        return out
    if n == kBandMaxN:
        out.add("band.flow.n_max" if flow else "band.points.n_max")
    if n == 0:
        return out | {"points.n0"}
    if n == 1 and not flow:
        out.add("points.n1")
    if staged(flow, n):
        out |= {"band.staged." + staging(flow, n, b) for b in range(B)}
        if (2 if flow else 3) * n == kBandPts:
            out.add("band.staged.last")
    else:
        out.add("band.unstaged")
    paths = band_paths(flow, inputs(name), h, w)
    out |= {"band.list"} & {"band." + p for p in paths}
    if not flow:   # points mode stores `valid`
        out |= {"band." + p + ".valid" for p in paths - {"list"}}
    return out


# ---- the cases --------------------------------------------------------------------------------------

def _flow(seed, B, h, w, sigma):
    return dict(mode="flow", B=B, n=h * w, h=h, w=w, make=lambda: prng.normal(seed, (B, 2, h, w), sigma))


def _many(n, h, w):
    """Coordinates as test_grid_sample_values_many_points_vs_oracle: over the map and one pixel beyond."""
    pts = prng.uniform(7, (3, n), -2.0, 1.0).astype(np.float32)
    pts[0] = (pts[0] + 2.0) / 3.0 * (w + 1) - 1.0
    pts[1] = (pts[1] + 2.0) / 3.0 * (h + 1) - 1.0
    return pts


def _one_target(n):
    return np.stack([np.full(n, 40.0, np.float32), np.full(n, 30.0, np.float32), prng.normal(41, (n,))])


def _cluster(n):
    return np.stack([np.float32(40.25) + prng.uniform(42, (n,), -1.5, 1.5),
                     np.float32(30.5) + prng.uniform(43, (n,), -1.5, 1.5), prng.normal(44, (n,))]).astype(np.float32)


def _cluster_edges(n, h, w):
    """The cluster with every 50th point (2 %) given an edge value in x (even hits) or y (odd hits)."""
    pts = _cluster(n)
    for i, s in enumerate(range(0, n, 50)):
        lim = (w, h)[i & 1]
        special = (np.nan, np.inf, -np.inf, lim - 1.0, float(lim), -1.0, -1e-7)
        pts[i & 1, s] = np.float32(special[(i >> 1) % len(special)])
    return pts


def _points(n, h, w, make):
    return dict(mode="points", B=1, n=n, h=h, w=w, make=make)


CASES = {
    # large-map kernel, counts and keys in the workspace, strided by batch item
    "flow_b2_264x300": dict(_flow(801, 2, 264, 300, 3.0), expect={"large.flow", "large.batch", "large.counts_ws"},
                            alone=1),
    # large-map kernel, counts in LDS (15,000 targets), keys in the workspace
    "points_70000_100x150": dict(_points(70_000, 100, 150, lambda: _many(70_000, 100, 150)),
                                 expect={"large.points", "large.counts_lds"}),
    # the kernel switch in points mode: the first is a prefix of the second
    "points_65536_120x150": dict(_points(65_536, 120, 150, lambda: _many(65_537, 120, 150)[:, :65_536]),
                                 expect={"band.points.n_max", "band.unstaged"}),
    "points_65537_120x150": dict(_points(65_537, 120, 150, lambda: _many(65_537, 120, 150)),
                                 expect={"large.points.n_min", "large.counts_ws"}),
    # the same switch in flow mode
    "flow_256x256": dict(_flow(802, 1, 256, 256, 3.0), expect={"band.flow.n_max", "band.unstaged", "band.list"}),
    "flow_257x256": dict(_flow(803, 1, 257, 256, 3.0), expect={"large.flow.n_min", "large.counts_ws"}),
    # one target with 80,000 contributions: fold_walk with `valid`
    "points_one_target": dict(_points(20_000, 60, 80, lambda: _one_target(20_000)), expect={"band.walk.valid"}),
    # bands past kBandCap: the sub-range path with `valid`
    "points_cluster": dict(_points(20_000, 60, 80, lambda: _cluster(20_000)), expect={"band.subrange.valid"}),
    # in-bounds edges of target_of, in the overflow paths
    "points_cluster_edges": dict(_points(20_000, 60, 80, lambda: _cluster_edges(20_000, 60, 80)),
                                 expect={"band.subrange.valid", "band.walk.valid"}),
    "points_n0": dict(_points(0, 5, 7, lambda: np.zeros((3, 0), np.float32)), expect={"points.n0"}),
    "points_n1": dict(_points(1, 5, 7, lambda: np.array([[2.25], [3.5], [1.75]], np.float32)),
                      expect={"points.n1", "band.list"}),
    # items 1 and 2: one item pointer unaligned (scalar staging), one aligned
    "flow_b3_7x9": dict(_flow(804, 3, 7, 9, 1.5), expect={"band.staged.scalar", "band.staged.aligned"}),
    # last staged size; first unstaged size of the pair (the 16-point gather rounds), odd n
    "flow_b2_64x80": dict(_flow(805, 2, 64, 80, 2.0), expect={"band.staged.last", "band.staged.aligned"}),
    "flow_b2_65x79": dict(_flow(806, 2, 65, 79, 2.0), expect={"band.unstaged"}),
}

_inputs = {}


def inputs(name):
    """The case's input, float32, read-only and made once: flow [B, 2, h, w] or points [3, n]."""
    if name not in _inputs:
        a = np.ascontiguousarray(CASES[name]["make"](), dtype=np.float32)
        c = CASES[name]
        assert a.shape == ((c["B"], 2, c["h"], c["w"]) if c["mode"] == "flow" else (3, c["n"]))
        a.setflags(write=False)
        _inputs[name] = a
    return _inputs[name]


def describe(name):
    c = CASES[name]
    return f"{c['mode']} B={c['B']} n={c['n']} {c['h']}x{c['w']}: " + " ".join(sorted(c["expect"]))
