"""Cases and inputs of the forward lookup at every radius (test infrastructure, numpy only).

Shared by tests/test_lookup_radius_ref.py (the oracle pinned against ATen on the CPU) and
tests/test_lookup_radius_gpu.py (the kernels against the oracle), so both look up the same fields.
Which kernel serves a plain lookup depends on the radius (launch_lookup_plain, csrc/lookup_kernels.h):
    4        lookup_cols_reg<4, PAIR / !PAIR>    (tests/test_corr_gpu.py)
    1        lookup_cols_reg<1, PAIR / !PAIR>    PAIR: every level width even (and every level 8-byte aligned)
    0, 2, 3  lookup_staged<0 / 2 / 3>
    5 .. 32  lookup_direct                       one thread per output, grid-stride over 8192 x 256 threads
KERNEL lists the cases of every instantiation and is asserted against kernel_of(), which restates the
dispatch from the radius and the level widths.  D = 8 feature channels throughout.
"""
import zlib

import numpy as np

import grad_ref
import prng
from gpu_guard import GRID_STRIDE_THREADS, mismatch  # noqa: F401  (mismatch: for the tests' messages)

D = 8

# name: (radius, B, H, W, levels, q_begin, q_count); q_count < H * W: a slab of query rows (C ABI only)
CASES = {
    "r0_17x21": (0, 2, 17, 21, 4, 0, 357),               # lookup_staged<0>, Q odd, tail block
    "r1_pair_18x16": (1, 2, 18, 16, 4, 0, 288),          # lookup_cols_reg<1, PAIR>, 4.5 query blocks
    "r1_17x21": (1, 2, 17, 21, 4, 0, 357),               # lookup_cols_reg<1, !PAIR>
    "r1_slab_17x20": (1, 2, 17, 20, 4, 60, 100),         # !PAIR (widths 20 / 10 / 5 / 2) on a slab starting inside an interleave group
    "r1_pair_slab_64x64_l5": (1, 1, 64, 64, 5, 30 * 64 + 20, 200),   # PAIR (64 / 32 / 16 / 8 / 4) on such a slab, with a level 4
    "r1_23x40": (1, 1, 23, 40, 4, 0, 920),               # widths 40 / 20 / 10 / 5: other w - 1 round trips
    "r2_17x21": (2, 2, 17, 21, 4, 0, 357),               # lookup_staged<2>
    "r3_17x21": (3, 2, 17, 21, 4, 0, 357),               # lookup_staged<3>
    "r3_slab_17x20": (3, 2, 17, 20, 4, 60, 100),         # lookup_staged<3> on a slab
    "r3_23x40": (3, 1, 23, 40, 4, 0, 920),
    "r3_64x64_l5": (3, 1, 64, 64, 5, 0, 4096),           # a level >= 4
    "r5_17x21": (5, 2, 17, 21, 4, 0, 357),               # lookup_direct
    "r5_slab_17x20": (5, 2, 17, 20, 4, 60, 100),         # lookup_direct on a slab
    "r8_16x16": (8, 1, 16, 16, 2, 0, 256),               # the window wider than the image
    "r32_16x16": (32, 1, 16, 16, 2, 0, 256),             # 2 x 65^2 x 256 outputs: the grid-stride loop wraps
    "r0_8x32_h1": (0, 1, 8, 32, 4, 0, 256),              # level 3 is 1 x 4: h - 1 = 0, the whole level NaN
    "r1_8x32_h1": (1, 1, 8, 32, 4, 0, 256),
    "r2_8x32_h1": (2, 1, 8, 32, 4, 0, 256),
    "r3_8x32_h1": (3, 1, 8, 32, 4, 0, 256),
    "r5_8x32_h1": (5, 1, 8, 32, 4, 0, 256),
    "r1_slab_64x120_l6": (1, 2, 64, 120, 6, 32 * 120, 120),   # !PAIR (120 / 60 / 30 / 15 / 7 / 3); a tiled level 4, a compact level 5
    "r5_slab_64x120_l6": (5, 2, 64, 120, 6, 32 * 120, 120),
}
SETS = ("smooth", "iid_large", "special", "edge", "int", "half", "up", "down", "p1e-4")
# the formats the _l6 cases were written for (layout.formats(64, 120, 6)): level 4 tiled with one
# tile per tile row, level 5 compact
L6_FORMATS = {4: 1, 5: 0}

# the cases of each kernel instantiation (asserted below against kernel_of)
KERNEL = {
    "lookup_cols_reg<1, PAIR>": ("r1_pair_18x16", "r1_8x32_h1", "r1_pair_slab_64x64_l5"),
    "lookup_cols_reg<1, !PAIR>": ("r1_17x21", "r1_slab_17x20", "r1_23x40", "r1_slab_64x120_l6"),
    "lookup_staged<0>": ("r0_17x21", "r0_8x32_h1"),
    "lookup_staged<2>": ("r2_17x21", "r2_8x32_h1"),
    "lookup_staged<3>": ("r3_17x21", "r3_slab_17x20", "r3_23x40", "r3_64x64_l5", "r3_8x32_h1"),
    "lookup_direct": ("r5_17x21", "r5_slab_17x20", "r5_8x32_h1", "r5_slab_64x120_l6", "r8_16x16", "r32_16x16"),
}


def level_widths(name):
    _, _, _, W, L, _, _ = CASES[name]
    return [W >> i for i in range(L)]


def kernel_of(name):
    """launch_lookup_plain / lookup_takes_cols (csrc/lookup_kernels.h) for the case: by the radius, and
    at radius 1 by whether every level width is even (the levels' 8-byte alignment, PAIR's other
    condition, is asserted where the pyramid exists: tests/test_lookup_radius_gpu.py).  Every case's
    output is far below the 2^31 bytes per batch item past which radius 1 leaves lookup_cols_reg."""
    r = CASES[name][0]
    if r > 4:
        return "lookup_direct"
    if r == 1:
        return "lookup_cols_reg<1, %sPAIR>" % ("" if all(w % 2 == 0 for w in level_widths(name)) else "!")
    return "lookup_staged<%d>" % r


def channels(name):
    r, _, _, _, L, _, _ = CASES[name]
    return L * (2 * r + 1) ** 2


def outputs(name):
    _, B, _, _, _, _, q = CASES[name]
    return B * channels(name) * q


def is_slab(name):
    _, _, H, W, _, _, q = CASES[name]
    return q != H * W


def h1_level(name):
    """The level whose height is 1 (the reference divides by h - 1 = 0 there), or None."""
    _, _, H, _, L, _, _ = CASES[name]
    one = [i for i in range(L) if H >> i == 1]
    return one[0] if one else None


# if a case changes, say so instead of silently covering less
assert sorted(n for ns in KERNEL.values() for n in ns) == sorted(CASES), "KERNEL does not list every case once"
for _k, _ns in KERNEL.items():
    for _n in _ns:
        assert kernel_of(_n) == _k, f"{_n} runs {kernel_of(_n)}, KERNEL lists it under {_k}"
assert all(channels(n) * CASES[n][6] * 4 < 0x7fffffff for n in CASES)
assert outputs("r32_16x16") == 2 * 65 * 65 * 256 > GRID_STRIDE_THREADS, "r32_16x16 no longer wraps lookup_direct's loop"
assert all(outputs(n) <= GRID_STRIDE_THREADS for n in CASES if n != "r32_16x16")
assert all(H * W >= 256 and q_begin + q <= H * W for _, _, H, W, _, q_begin, q in CASES.values())   # special_coords' need
assert all((h1_level(n) is not None) == n.endswith("_h1") for n in CASES)
assert all(h1_level(n) == 3 for n in CASES if n.endswith("_h1"))


def assert_l6_formats():
    """The _l6 cases reach a tiled level 4 and a compact level 5 only while the library's format
    rule says so (asks libecorr.so, a host call: no GPU)."""
    from eraft_amd.layout import formats
    ntx = formats(64, 120, 6)
    for lv, n in L6_FORMATS.items():
        assert ntx[lv] == n, f"level {lv} of 64 x 120 has format {ntx[lv]}, the _l6 cases were written for {n}"


def seed_of(name):
    """The case's first seed, from its name: adding a case leaves the others' inputs as they were."""
    return 1000 + 10 * (zlib.crc32(name.encode()) % 100000)


def fmaps(name):
    """(fmap1, fmap2) [B, D, H, W] of the whole map."""
    _, B, H, W, _, _, _ = CASES[name]
    s = seed_of(name)
    return prng.normal(s, (B, D, H, W)), prng.normal(s + 1, (B, D, H, W))


def coord_sets(name):
    """{set: [B, 2, H, W] float32} of the whole map, in the order of SETS."""
    _, B, H, W, _, _, _ = CASES[name]
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
        # one ulp off the integers: the floor flips that the window's slack row and column exist for
        "up": np.nextafter(grid, f32(np.inf)),
        "down": np.nextafter(grid, f32(-np.inf)),
        "p1e-4": grid + f32(1e-4),
    }
    assert tuple(sets) == SETS
    _, _, _, _, _, q_begin, q = CASES[name]
    if q_begin >= 256:
        # special_coords puts its blocks of special queries into the field's first 256 queries and
        # scatters single ones through fewer than 1000 more: a slab that begins past those (the _l6
        # cases) would hold none, so its queries take the coordinates of the field's first q_count
        sp = sets["special"].reshape(B, 2, H * W)
        sp[:, :, q_begin:q_begin + q] = sp[:, :, :q].copy()
    return {k: np.ascontiguousarray(v, dtype=np.float32) for k, v in sets.items()}


def slab(a, name):
    """[B, C, H, W] (or [B, C, H * W]) of the whole map -> the case's query rows [B, C, q_count]."""
    _, B, H, W, _, q_begin, q = CASES[name]
    return np.ascontiguousarray(a.reshape(B, a.shape[1], H * W)[:, :, q_begin:q_begin + q])
