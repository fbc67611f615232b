"""Voxel-grid test cases shared by tests/golden/make_golden_next.py and the parity tests:
name -> (n events, C, H, W, seed) plus the edge-case edits each case applies to its events."""
import numpy as np

import prng

DSEC_VOXEL = {"vd_small": (3000, 5, 20, 30, 500), "vd_mid": (50000, 15, 48, 64, 510),
              "vd_const_t": (400, 3, 10, 12, 520), "vd_nan": (2000, 4, 16, 16, 530), "vd_hot": (5000, 5, 8, 8, 540),
              # one and two events: t[-1] - t[0] = 0 when it is the only datum (t_norm NaN: an empty grid)
              "vd_n1": (1, 3, 5, 7, 550), "vd_n2": (2, 3, 5, 7, 560), "vd_n2_equal_t": (2, 3, 5, 7, 570)}
MVSEC_VOXEL = {"vm_small": (3000, 5, 26, 34, 600), "vm_mid": (50000, 15, 48, 64, 610),
               "vm_const_t": (300, 5, 6, 7, 620), "vm_hot": (4000, 15, 4, 5, 630), "vm_bad": (100, 5, 6, 7, 640),
               # one and two events: deltaT == 0 -> 1 (transformers.py:74-75) puts them in bin 0
               "vm_n1": (1, 3, 5, 7, 650), "vm_n2": (2, 3, 5, 7, 660), "vm_n2_equal_t": (2, 3, 5, 7, 670)}


def dsec_case(k, n, H, W, seed):
    p, t, x, y = prng.dsec_events(seed, n, H, W)
    if k == "vd_const_t":
        t[:] = 5.0
    if k == "vd_nan":
        x[::97] = np.nan
        y[5::89] = np.inf
    if k == "vd_hot":
        x[:] = 3.25
        y[:] = 4.75
    if k in ("vd_n1", "vd_n2", "vd_n2_equal_t"):   # inside the grid, whatever the seed draws
        x[:] = np.float32([2.25, 4.5][:n])
        y[:] = np.float32([1.75, 3.25][:n])
    if k == "vd_n2_equal_t":
        t[:] = 5.0
    return p, t, x, y


def mvsec_case(k, n, H, W, seed):
    ev = prng.mvsec_events(seed, n, H, W)
    if k == "vm_const_t":
        ev[:, 0] = 7.0
    if k == "vm_hot":
        ev[:, 1] = 2.0
        ev[:, 2] = 3.0
    if k == "vm_n2_equal_t":
        ev[:, 0] = 7.0
    if k == "vm_bad":
        ev[17, 1] = W * H * 99.0
    return ev
