"""Cases and inputs of the radius-4 lookup's three consumer forms (test infrastructure, numpy only).

CorrBlock.lookup_conv1x1_relu never runs the plain lookup: it runs ecorr_lookup_qmax (mode "split"),
ecorr_lookup_presplit (mode "presplit") or ecorr_lookup_conv1x1_relu[_packed] (mode "fused"), each
with stores and control flow of its own (csrc/lookup_kernels.h lookup_cols_reg<4, 64, PAIR, QMAX /
PRESPLIT>, csrc/motion.hip lookup_conv_kernel).  tests/test_lookup_consumers_gpu.py runs the three on
the cases below and the nine coordinate sets of tests/lookup_radius_cases.py; radius 4 and D = 8
feature channels throughout.  (lookup_radius_cases' own table and kernel_of do not describe radius 4.)
"""
import zlib

import numpy as np

import grad_ref
import prng
from lookup_radius_cases import L6_FORMATS, SETS  # noqa: F401  (SETS, L6_FORMATS: for the tests)

D = 8
R = 4
KK = (2 * R + 1) ** 2   # 81 channels per level

# name: (B, H, W, levels, q_begin, q_count); q_count < H * W: a slab of query rows (C ABI only)
CASES = {
    "pair_18x16": (2, 18, 16, 4, 0, 288),                  # PAIR, 4.5 blocks of 64 / 9 of 32
    "odd_17x21": (2, 17, 21, 4, 0, 357),                   # !PAIR, odd Q, tail block
    "slab_17x20": (2, 17, 20, 4, 60, 100),                 # !PAIR slab inside an interleave group, ragged 64 and 32
    "l3_23x40": (1, 23, 40, 3, 0, 920),                    # L = 3: 33 of 34 presplit groups, C = 243
    "l2_16x24": (2, 16, 24, 2, 0, 384),                    # L = 2: C = 162
    "l1_20x20": (1, 20, 20, 1, 0, 400),                    # L = 1: 11 of 12 presplit groups, C = 81
    "pair_slab_64x64_l5": (1, 64, 64, 5, 30 * 64 + 20, 200),   # qmax only: PAIR with a level 4
    "slab_64x120_l6": (2, 64, 120, 6, 32 * 120, 120),      # qmax only: tiled level 4, compact level 5
    "h1_8x32": (1, 8, 32, 4, 0, 256),                      # qmax only: level 3 is 1 x 4, all NaN
}
# what each case exists for (asserted below)
PAIR = {"pair_18x16": True, "odd_17x21": False, "slab_17x20": False, "l3_23x40": True, "l2_16x24": True,
        "l1_20x20": True, "pair_slab_64x64_l5": True, "slab_64x120_l6": False, "h1_8x32": True}
QMAX_ONLY = ("pair_slab_64x64_l5", "slab_64x120_l6", "h1_8x32")
# the presplit and fused forms take at most 4 levels; of those, h1_8x32 is the qmax form's
CONV_CASES = tuple(n for n in CASES if n not in QMAX_ONLY)


def level_widths(name):
    _, _, W, L, _, _ = CASES[name]
    return [W >> i for i in range(L)]


def is_pair(name):
    """Column-pair staging (lookup_takes_cols / launch_lookup_conv): every level width even.  Its other
    condition, every level 8-byte aligned, is asserted where the pyramid exists."""
    return all(w % 2 == 0 for w in level_widths(name))


def channels(name):
    return CASES[name][3] * KK


def is_slab(name):
    _, H, W, _, _, q = CASES[name]
    return q != H * W


def h1_level(name):
    """The level whose height is 1 (the reference divides by h - 1 = 0 there: all NaN), or None."""
    _, H, _, L, _, _ = CASES[name]
    one = [i for i in range(L) if H >> i == 1]
    return one[0] if one else None


# if a case changes, say so instead of silently covering less
assert sorted(PAIR) == sorted(CASES)
for _n in CASES:
    assert is_pair(_n) == PAIR[_n], f"{_n}: level widths {level_widths(_n)} are {'' if is_pair(_n) else 'not '}all even"
assert all(H * W >= 256 and q_begin + q <= H * W for _, H, W, _, q_begin, q in CASES.values())   # special_coords' need
assert all(CASES[n][3] <= 4 for n in CONV_CASES) and len(CONV_CASES) == 6
assert {CASES[n][3] for n in CONV_CASES} == {1, 2, 3, 4}
assert any(PAIR[n] for n in CONV_CASES if CASES[n][3] == 4) and any(not PAIR[n] for n in CONV_CASES if CASES[n][3] == 4)
assert CASES["pair_18x16"][5] % 64 == 32                                               # 4.5 blocks of 64, 9 of 32
assert all(CASES[n][5] % 64 and CASES[n][5] % 32 for n in ("odd_17x21", "slab_17x20"))   # ragged at 64 and at 32
assert CASES["slab_17x20"][4] % 64 != 0 and CASES["pair_slab_64x64_l5"][4] % 64 != 0   # inside an interleave group
assert CASES["pair_slab_64x64_l5"][3] > 4 and CASES["slab_64x120_l6"][3] == 6
assert h1_level("h1_8x32") == 3 and all(h1_level(n) is None for n in CASES if n != "h1_8x32")
assert all(channels(n) * CASES[n][5] * 4 < 0x7fffffff for n in CASES)


def assert_l6_formats():
    """slab_64x120_l6 reaches a tiled level 4 and a compact level 5 only while the library's format
    rule says so (asks libecorr.so, a host call: no GPU)."""
    from eraft_amd.layout import formats
    ntx = formats(64, 120, 6)
    for lv, n in L6_FORMATS.items():
        assert ntx[lv] == n, f"level {lv} of 64 x 120 has format {ntx[lv]}, slab_64x120_l6 was written for {n}"


def seed_of(name):
    """The case's first seed, from its name: adding a case leaves the others' inputs as they were."""
    return 5000 + 10 * (zlib.crc32(name.encode()) % 100000)


def fmaps(name):
    """(fmap1, fmap2) [B, D, H, W] of the whole map."""
    B, H, W, _, _, _ = CASES[name]
    s = seed_of(name)
    return prng.normal(s, (B, D, H, W)), prng.normal(s + 1, (B, D, H, W))


def coord_sets(name):
    """{set: [B, 2, H, W] float32} of the whole map, in the order of SETS (the nine sets of
    lookup_radius_cases.coord_sets, with its remedy for slabs that begin past the special queries)."""
    B, H, W, _, q_begin, q = CASES[name]
    s = seed_of(name)
    grid = prng.coords_with_flow(0, B, H, W, 0.0)
    f32 = np.float32
    sets = {
        "smooth": prng.coords_with_flow(s + 2, B, H, W, 2.0),
        "iid_large": prng.coords_with_flow(s + 3, B, H, W, 40.0),
        "special": grad_ref.special_coords(s + 4, B, H, W),      # NaN, +-inf, huge: the direct-gather mode
        "edge": grad_ref.edge_coords(B, H, W),                   # windows over all four borders
        "int": grid,
        "half": grid + f32(0.5),
        "up": np.nextafter(grid, f32(np.inf)),
        "down": np.nextafter(grid, f32(-np.inf)),
        "p1e-4": grid + f32(1e-4),
    }
    assert tuple(sets) == SETS
    if q_begin >= 256:
        # special_coords puts its blocks of special queries into the field's first 256 queries: a slab
        # that begins past those takes the coordinates of the field's first q_count queries
        sp = sets["special"].reshape(B, 2, H * W)
        sp[:, :, q_begin:q_begin + q] = sp[:, :, :q].copy()
    return {k: np.ascontiguousarray(v, dtype=np.float32) for k, v in sets.items()}


def slab(a, name):
    """[B, C, H, W] (or [B, C, H * W]) of the whole map -> the case's query rows [B, C, q_count]."""
    B, H, W, _, q_begin, q = CASES[name]
    return np.ascontiguousarray(a.reshape(B, a.shape[1], H * W)[:, :, q_begin:q_begin + q])
