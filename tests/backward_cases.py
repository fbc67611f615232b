"""Cases and inputs of the CorrBlock backward fixtures (test infrastructure, tests/prng.py only).

Shared by tests/golden/make_golden_backward.py (the reference's gradients) and tests/test_grad_gpu.py
(ours), so both differentiate the same loss:
    loss = sum_i (corr_fn(coords_i) * go_i).sum(),   go_i = prng.normal(seed + 200 + i, out.shape)
over the lookups of `lookups(case)`, in that order.
"""
import numpy as np

import prng

# name: (B, D, H, W, levels, radius, seed); every level is at least 2 x 2
CASES = {
    "t16x24": (1, 256, 16, 24, 4, 4, 110),      # the E-RAFT configuration, 384 rows
    "b2_17x20": (2, 256, 17, 20, 4, 4, 120),    # odd levels 17x20 -> 8x10 -> 4x5 -> 2x2, 680 rows, 2 items
    "l3r2_d64": (1, 64, 12, 16, 3, 2, 130),
    "d100_l2r3": (1, 100, 16, 16, 2, 3, 140),   # D no multiple of any tile
    "d3_l3r1": (2, 3, 8, 8, 3, 1, 150),         # D below one MFMA k step; levels 8, 4, 2
}
# the fixtures of these also hold the fp32 per-level pyramid gradients
PYRAMID_CASES = ("d3_l3r1", "l3r2_d64")
# this case adds the integer and near-integer coordinate sets (floor flips) to its lookups
EDGE_CASE = "d3_l3r1"


def fmaps(case):
    B, D, H, W, _, _, seed = CASES[case]
    return prng.normal(seed, (B, D, H, W)), prng.normal(seed + 1, (B, D, H, W))


def coord_sets(case):
    """As tests/golden/make_golden.py coord_sets (seed + 100): flow sigma 0.5 / 6 / 40 px, the integer
    grid, and integers nudged by a few ulps-worth (the unnormalize round trip flips floor() there)."""
    B, _, H, W, _, _, seed = CASES[case]
    s = seed + 100
    sets = {"s0p5": prng.coords_with_flow(s, B, H, W, 0.5),
            "s6": prng.coords_with_flow(s + 1, B, H, W, 6.0),
            "s40": prng.coords_with_flow(s + 2, B, H, W, 40.0),
            "int": prng.coords_with_flow(0, B, H, W, 0.0)}
    pick = prng.uniform(s + 3, (B, 2, H, W), 0.0, 8.0).astype(np.int64)
    eps = np.array([0.0, 1e-6, -1e-6, 2e-6, -2e-6, 5e-7, -5e-7, 0.5], dtype=np.float32)
    sets["nearint"] = (sets["int"] + eps[pick]).astype(np.float32)
    return sets


def lookups(case):
    """[(set name, coords, upstream seed)] in loss order."""
    names = ["s0p5", "s6", "s40"] + (["int", "nearint"] if case == EDGE_CASE else [])
    sets = coord_sets(case)
    seed = CASES[case][6]
    return [(n, sets[n], seed + 200 + i) for i, n in enumerate(names)]


def upstream(case, seed):
    B, _, H, W, L, r, _ = CASES[case]
    return prng.normal(seed, (B, L * (2 * r + 1) ** 2, H, W))
