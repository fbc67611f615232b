"""Inputs of the generic bilinear_sampler / coords_grid checks (test infrastructure, numpy only).

Shared by tests/test_lookup_radius_ref.py (the oracle against the ATen expression on the CPU) and
tests/test_sampler_gpu.py (the kernels against the oracle).
"""
import numpy as np

import prng
from gpu_guard import GRID_STRIDE_THREADS

# (N, C, h, w, Hg, Wg): a general image, images 1 pixel tall / wide / both (the reference divides by
# size - 1 = 0), the smallest image with an interior, and a grid past one pass of the grid-stride loop;
# then the 1-pixel images again with 16 x 16 grids, which hold all 252 special points (an 8 x 8 grid
# holds the first 64: three y values)
CASES = [(2, 3, 7, 9, 16, 20), (1, 2, 1, 9, 8, 8), (1, 2, 7, 1, 8, 8), (1, 1, 1, 1, 4, 4), (3, 1, 2, 2, 8, 8),
         (1, 1, 5, 7, 1500, 1400), (1, 2, 1, 9, 16, 16), (1, 2, 7, 1, 16, 16), (1, 1, 1, 1, 16, 16)]
WRAPS = (1, 1, 5, 7, 1500, 1400)
assert WRAPS in CASES and WRAPS[0] * WRAPS[4] * WRAPS[5] > GRID_STRIDE_THREADS, "the sampler's loop no longer wraps"
assert all(c[0] * c[4] * c[5] <= GRID_STRIDE_THREADS for c in CASES if c != WRAPS)

# coords_grid (B, H, W): 3 x 2 x 600 x 601 elements wrap its loop
GRID_CASES = [(3, 600, 601), (1, 1, 1), (2, 1, 300)]
assert 3 * 2 * 600 * 601 > GRID_STRIDE_THREADS


def case_id(c):
    return "n%d_c%d_%dx%d_g%dx%d" % c


def special_values(h, w):
    """Coordinates where the mask's strict inequalities and the zero padding decide: exactly on and
    one ulp inside the borders, one pixel outside, signed zero, a small negative, non-finite, huge."""
    f = np.float32
    return np.array([0.0, -0.0, w - 1, h - 1, -1.0, w, h, 0.5, w - 1.5, 2.0, 2.9999998,
                     np.nextafter(f(0.0), f(1.0)), np.nextafter(f(w - 1), f(0.0)), -1e-7,
                     np.nan, np.inf, -np.inf, 1e9, -7e5, 3e7, 1e38], dtype=np.float32)


def inputs(case, seed=700):
    """(img [N, C, h, w], grid [N, Hg, Wg, 2] of (x, y) pixel coordinates): uniform coordinates in
    [-3, max(h, w) + 2], the leading points of every item overwritten by the cross product of the
    special values (x) and the first 12 of them (y), as far as the grid holds them; item n starts
    64 n points into the product."""
    N, C, h, w, Hg, Wg = case
    img = prng.normal(seed, (N, C, h, w))
    grid = prng.uniform(seed + 1, (N, Hg * Wg, 2), -3.0, max(h, w) + 2.0)
    tab = special_values(h, w)
    pts = np.array([(x, y) for y in tab[:12] for x in tab], dtype=np.float32)
    assert len(pts) == 252
    k = min(len(pts), Hg * Wg)
    for n in range(N):
        grid[n, :k] = np.roll(pts, -64 * n, axis=0)[:k]
    return img, np.ascontiguousarray(grid.reshape(N, Hg, Wg, 2))
