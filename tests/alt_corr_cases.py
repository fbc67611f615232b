"""Cases and inputs of the volume-free lookup (AlternateCorrBlock, csrc/alt.hip): test infrastructure,
numpy only.  Shared by tests/test_alt_corr_ref.py (the fp64 reference, on the CPU) and
tests/test_alt_corr_gpu.py (the kernels against it), so both look up the same fields.

Radii <= 4 run alt_window_kernel<r>, larger ones alt_generic_kernel; queries whose window does not fit
(the `special` set's NaN / inf / huge coordinates, every query of a 1-pixel-tall level) take the generic
sample inside the window kernel.  The nine coordinate sets are those of lookup_radius_cases.coord_sets,
rebuilt for these shapes.
"""
import zlib

import numpy as np

import grad_ref
import prng

# name: (radius, B, D, H, W, levels)
CASES = {
    "a4_17x21_d37": (4, 2, 37, 17, 21, 4),    # odd sides drop pooled rows / columns; D pads to Dp = 40; batch stride
    "a4_16x24_d256": (4, 1, 256, 16, 24, 4),  # one float4 per lane
    "a4_8x32_h1_d8": (4, 1, 8, 8, 32, 4),     # level 3 is 1 x 4: NaN throughout
    "a4_16x16_d320": (4, 1, 320, 16, 16, 2),  # D above one wave pass (two 256-channel chunks)
    "a1_17x21_d8": (1, 2, 8, 17, 21, 4),      # small windows: 25 taps, one batch
    "a0_17x21_d8": (0, 2, 8, 17, 21, 4),      # 9 taps
    "a5_17x21_d8": (5, 2, 8, 17, 21, 4),      # generic kernel
    "a8_16x16_d8": (8, 1, 8, 16, 16, 2),      # generic kernel, the window wider than the image
}
SETS = ("smooth", "iid_large", "special", "edge", "int", "half", "up", "down", "p1e-4")
WINDOW_MAX_RADIUS = 4   # (2r+3)^2 <= 128 taps: two batches of 64

assert all(H * W >= 256 for _, _, _, H, W, _ in CASES.values())   # special_coords' need


def kernel_of(name):
    return "alt_window_kernel<%d>" % CASES[name][0] if CASES[name][0] <= WINDOW_MAX_RADIUS else "alt_generic_kernel"


def channels(name):
    r, _, _, _, _, L = CASES[name]
    return L * (2 * r + 1) ** 2


def level_sizes(name):
    _, _, _, H, W, L = CASES[name]
    return [(H >> i, W >> i) for i in range(L)]


def h1_level(name):
    """The level whose height is 1 (the reference divides by h - 1 = 0 there), or None."""
    one = [i for i, (h, _) in enumerate(level_sizes(name)) if h == 1]
    return one[0] if one else None


assert [n for n in CASES if h1_level(n) is not None] == ["a4_8x32_h1_d8"] and h1_level("a4_8x32_h1_d8") == 3


def seed_of(name):
    """The case's first seed, from its name: adding a case leaves the others' inputs as they were."""
    return 5000 + 10 * (zlib.crc32(name.encode()) % 100000)


def fmaps(name):
    """(fmap1, fmap2) [B, D, H, W] float32."""
    _, B, D, H, W, _ = CASES[name]
    s = seed_of(name)
    return prng.normal(s, (B, D, H, W)), prng.normal(s + 1, (B, D, H, W))


def coord_sets(name):
    """{set: [B, 2, H, W] float32}, in the order of SETS."""
    _, B, _, H, W, _ = CASES[name]
    s = seed_of(name)
    grid = prng.coords_with_flow(0, B, H, W, 0.0)
    f32 = np.float32
    sets = {
        "smooth": prng.coords_with_flow(s + 2, B, H, W, 2.0),
        "iid_large": prng.coords_with_flow(s + 3, B, H, W, 40.0),
        "special": grad_ref.special_coords(s + 4, B, H, W),      # NaN, +-inf, huge: windows that do not fit
        "edge": grad_ref.edge_coords(B, H, W),                   # windows over all four borders
        "int": grid,
        "half": grid + f32(0.5),
        # one ulp off the integers: the floor flips that the window's slack row and column exist for
        "up": np.nextafter(grid, f32(np.inf)),
        "down": np.nextafter(grid, f32(-np.inf)),
        "p1e-4": grid + f32(1e-4),
    }
    assert tuple(sets) == SETS
    return {k: np.ascontiguousarray(v, dtype=np.float32) for k, v in sets.items()}
