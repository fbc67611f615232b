"""Cases of the voxel grid's dispatch tests (csrc/voxel.hip) and a plain Python mirror of its dispatch:
test infrastructure, numpy only.  Shared by tests/test_dispatch_mirrors.py (on the CPU: the mirror's
constants against the source, every branch covered) and tests/test_voxel_dispatch_gpu.py.

launch_voxel sends DSEC events to the tiled pipeline (vb_*: tiles of VB_TY x VB_TX cells, a window of
events per tile, sorted in LDS up to VB_CAP events and read where it lies in HBM past that) while
vtile_geom holds: at most VB_MAXNB tiles (vb_count's LDS histogram) and (C + 1) * VB_WK <= VB_MAXRUN
runs per window.  Everything else -- MVSEC always -- takes the key-range pipeline, whose gather runs
min(kGatherBlocks, C * H) blocks over contiguous ranges of the C * H grid rows.
"""
import numpy as np

import prng
import voxel_cases

# csrc/voxel.hip (tests/test_dispatch_mirrors.py holds these to the source)
VB_TY, VB_TX = 4, 16
VB_MAXNB = 12288
VB_MAXRUN = 2048
VB_CAP = 512
VB_EPB = 8192
kGatherBlocks = 2048
VB_WK = (VB_TY + 1) * (VB_TX + 1)   # base cells of a window, per time bin

BRANCHES = (
    "tiled.nb_max", "tiled.lds", "tiled.arena", "tiled.count_blocks", "tiled.copies_max",
    "key_range.nb", "key_range.C", "key_range.mvsec", "key_range.gather_wrap", "key_range.scan_sums_wrap",
    "n1", "n2",
)


# ---- the mirror -------------------------------------------------------------------------------------

def tiles(H, W):
    """vtile_geom: (gy, gx, nb)"""
    gy, gx = (H + VB_TY - 1) // VB_TY, (W + VB_TX - 1) // VB_TX
    return gy, gx, gy * gx


def path(dsec, n, C, H, W):
    """("tiled", None), or ("key_range", why): launch_voxel / vtile_geom."""
    if not dsec:
        return "key_range", "mvsec"
    if tiles(H, W)[2] > VB_MAXNB:
        return "key_range", "nb"
    if (C + 1) * VB_WK > VB_MAXRUN:
        return "key_range", "C"
    assert 4 * n < 1 << 31 and W < 65535 and H < 65535   # vtile_geom's other limits: no case is near them
    return "tiled", None


def gather_blocks(C, H):
    """(blocks, grid rows per block) of the key-range gather."""
    blocks = min(kGatherBlocks, C * H)
    return blocks, (C * H + blocks - 1) // blocks


def key_range(dsec, C, H, W):
    return (C + 1) * (H + 1) * (W + 1) if dsec else C * H * W


def window_counts(t, x, y, C, H, W):
    """Events per window of the tiled path (vb_count): an event is copied to every tile whose window
    -- its cells' base cells and the +1 halo -- holds its base cell."""
    with np.errstate(invalid="ignore", divide="ignore"):
        tn = np.float32(C - 1) * (t - t[0]) / (t[-1] - t[0])
        fin = np.isfinite(x) & np.isfinite(y) & np.isfinite(tn)
        x0, y0, ti = (np.where(fin, np.trunc(v), -9).astype(np.int64) for v in (x, y, tn))
    ok = (x0 >= -1) & (x0 < W) & (y0 >= -1) & (y0 < H) & (ti >= -1) & (ti < C)
    ey, ex = y0[ok] + 1, x0[ok] + 1
    gy, gx, nb = tiles(H, W)
    cnt = np.zeros(nb, dtype=np.int64)
    for dy in (0, 1):
        for dx in (0, 1):
            ty, tx = ey // VB_TY - dy, ex // VB_TX - dx
            m = (ty >= 0) & (ty < gy) & (tx >= 0) & (tx < gx)
            if dy:
                m &= ey % VB_TY == 0
            if dx:
                m &= ex % VB_TX == 0
            np.add.at(cnt, (ty * gx + tx)[m], 1)
    return cnt


def tags(name):
    """The branches of BRANCHES the mirror says the case takes."""
    dsec, n, C, H, W = CASES[name]["shape"]
    out = set()
    which, why = path(dsec, n, C, H, W)
    if which == "tiled":
        _, t, x, y = events(name)
        cnt = window_counts(t, x, y, C, H, W)
        if tiles(H, W)[2] == VB_MAXNB:
            out.add("tiled.nb_max")
        if ((cnt > 0) & (cnt <= VB_CAP)).any():
            out.add("tiled.lds")
        if (cnt > VB_CAP).any():
            out.add("tiled.arena")
        if n > VB_EPB:
            out.add("tiled.count_blocks")
        # every event in four windows and the last window in the arena: the copies, and the arena's run
        # order behind them, reach the last element plan_tiled sizes (4n copies), the workspace's end
        if cnt.sum() == 4 * n and cnt[-1] > VB_CAP and (16 * n) % 256 == 0:
            out.add("tiled.copies_max")
    else:
        out.add("key_range." + why)
        if gather_blocks(C, H)[1] > 1:
            out.add("key_range.gather_wrap")
        if (key_range(dsec, C, H, W) + 1 + 4095) // 4096 > 256:   # scan_sums: more tile sums than one block pass
            out.add("key_range.scan_sums_wrap")
    if n <= 2:
        out.add("n%d" % n)
    return out


# ---- the cases --------------------------------------------------------------------------------------

def _hot_pixel():
    p, t, x, y = prng.dsec_events(730, 20_000, 16, 64)
    hot = prng.uniform(731, (20_000,)) < 0.6
    x[hot] = np.float32(10.3)
    y[hot] = np.float32(5.7)
    return p, t, x, y


def _corner():
    """Every event on the base cell shared by the four tiles of an 8 x 32 grid (extended cell (4, 16))."""
    p, t, x, y = prng.dsec_events(910, 1_024, 8, 32)
    x[:] = np.float32(15.0) + prng.uniform(911, (1_024,), 0.0, 0.999)
    y[:] = np.float32(3.0) + prng.uniform(912, (1_024,), 0.0, 0.999)
    return p, t, x, y


def _dsec(seed, n, C, H, W, expect, make=None):
    return dict(shape=(True, n, C, H, W), expect=expect, make=make or (lambda: prng.dsec_events(seed, n, H, W)))


def _golden(dsec, k):
    n, C, H, W, seed = (voxel_cases.DSEC_VOXEL if dsec else voxel_cases.MVSEC_VOXEL)[k]
    make = (lambda: voxel_cases.dsec_case(k, n, H, W, seed)) if dsec else (lambda: voxel_cases.mvsec_case(k, n, H, W, seed))
    return dict(shape=(dsec, n, C, H, W), expect={"n%d" % n}, make=make)


CASES = {
    "nb_12288": _dsec(900, 40_000, 2, 384, 2048, {"tiled.nb_max", "tiled.count_blocks"}),   # vb_count's histogram full
    "nb_12416": _dsec(901, 40_000, 2, 385, 2048, {"key_range.nb"}),
    # the project's large-frame size: K = 6 * 721 * 1281 keys
    "sensor_720p": _dsec(902, 100_000, 5, 720, 1280, {"key_range.nb", "key_range.scan_sums_wrap"}),
    "c24_wrap": _dsec(903, 30_000, 24, 100, 37, {"key_range.C", "key_range.gather_wrap"}),
    "mvsec_wrap": dict(shape=(False, 300_000, 15, 260, 346), expect={"key_range.mvsec", "key_range.gather_wrap"},
                       make=lambda: prng.mvsec_events(710, 300_000, 260, 346)),
    # test_voxel_dsec_tiled_paths_vs_oracle's sparse_ragged and hot_pixel events
    "tiled_lds": _dsec(750, 3_000, 5, 21, 70, {"tiled.lds"}),
    "tiled_arena": _dsec(730, 20_000, 3, 16, 64, {"tiled.arena", "tiled.count_blocks"}, _hot_pixel),
    # the workspace used to its last byte: 4n copies, the last window's run order in the arena
    "tiled_corner": _dsec(910, 1_024, 3, 8, 32, {"tiled.copies_max", "tiled.arena"}, _corner),
    "n1_dsec": _golden(True, "vd_n1"),
    "n2_dsec": _golden(True, "vd_n2"),
    "n2_dsec_equal_t": _golden(True, "vd_n2_equal_t"),
    "n1_mvsec": _golden(False, "vm_n1"),
    "n2_mvsec": _golden(False, "vm_n2"),
    "n2_mvsec_equal_t": _golden(False, "vm_n2_equal_t"),
}

_events = {}


def events(name):
    """The case's events, read-only and made once: DSEC (p, t, x, y) float32, MVSEC [n, 4] float64."""
    if name not in _events:
        ev = CASES[name]["make"]()
        for a in (ev if isinstance(ev, tuple) else (ev,)):
            a.setflags(write=False)
        _events[name] = ev
    return _events[name]


def describe(name):
    dsec, n, C, H, W = CASES[name]["shape"]
    which, why = path(dsec, n, C, H, W)
    blocks, per = gather_blocks(C, H)
    how = "tiled, %d tiles" % tiles(H, W)[2] if which == "tiled" else \
        "key-range (%s), gather %d blocks x %d rows" % (why, blocks, per)
    return f"{'DSEC' if dsec else 'MVSEC'} n={n} C={C} {H}x{W}: {how}; " + " ".join(sorted(CASES[name]["expect"]))
