"""The reference of the volume-free lookup (test infrastructure, numpy on the CPU).

The function AlternateCorrBlock computes is CorrBlock's: sample the pyramid of the all-pairs volume.
The reference does exactly that with the volume in fp64: f1^T f2 / sqrt(D) in fp64, pooled in fp64 (the
floor-halving 2 x 2 mean), every level rounded ONCE to fp32, then oracle.lookup -- the path
tests/test_lookup_radius_ref.py pins to ATen's grid_sample bit for bit.  So sample positions, NaN
samples and exact zeros are the reference lookup's, and the values carry one fp32 rounding per level
element plus the blend's.

The bound scale S of the elementwise check is the same computation on |f1| and |f2|: the blend weights
are non-negative, so S = sum of weight * sum_d |f1_d| |pool f2_d| / sqrt(D) bounds the magnitude every
rounding error of a sample is relative to.
"""
import numpy as np

import alt_corr_cases as ac
import oracle


def pool64(x):
    """Floor-halving 2 x 2 mean over the last two axes (an odd last row / column is dropped), fp64."""
    h, w = x.shape[-2] // 2, x.shape[-1] // 2
    x = x[..., :2 * h, :2 * w]
    return 0.25 * (x[..., 0::2, 0::2] + x[..., 0::2, 1::2] + x[..., 1::2, 0::2] + x[..., 1::2, 1::2])


def volume_levels64(f1, f2, L):
    """Correlate, then pool: levels [B Q, h_i, w_i] of f1^T f2 / sqrt(D), fp64."""
    f1, f2 = np.asarray(f1, np.float64), np.asarray(f2, np.float64)
    B, D, H, W = f1.shape
    lv = np.einsum("bdq,bdhw->bqhw", f1.reshape(B, D, H * W), f2).reshape(B * H * W, H, W) / np.sqrt(np.float64(D))
    out = [lv]
    for _ in range(L - 1):
        out.append(pool64(out[-1]))
    return out


def pooled_feature_levels64(f1, f2, L):
    """Pool, then correlate (what the kernels do): f1^T pool^i(f2) / sqrt(D), fp64."""
    f1, f2 = np.asarray(f1, np.float64), np.asarray(f2, np.float64)
    B, D, H, W = f1.shape
    out = []
    for i in range(L):
        if i:
            f2 = pool64(f2)
        h, w = f2.shape[-2:]
        out.append(np.einsum("bdq,bdhw->bqhw", f1.reshape(B, D, H * W), f2).reshape(B * H * W, h, w)
                   / np.sqrt(np.float64(D)))
    return out


def levels32(f1, f2, L):
    """The fp64 volume pyramid, each level rounded once to fp32."""
    return [np.ascontiguousarray(lv, dtype=np.float32) for lv in volume_levels64(f1, f2, L)]


_cache = {}


def reference(name):
    """case -> {set: (coords [B, 2, H, W], ref [B, C, H, W], S [B, C, H, W])}: computed once, shared by the
    tests, never written."""
    if name not in _cache:
        r, B, D, H, W, L = ac.CASES[name]
        f1, f2 = ac.fmaps(name)
        lv = levels32(f1, f2, L)
        la = levels32(np.abs(f1), np.abs(f2), L)
        runs = {}
        for s, c in ac.coord_sets(name).items():
            ref, S = oracle.lookup(lv, c, r), oracle.lookup(la, c, r)
            for a in (c, ref, S):
                a.setflags(write=False)
            runs[s] = (c, ref, S)
        _cache[name] = runs
    return _cache[name]


def level_channels(name, i):
    """The channel slice of level i in a lookup output."""
    KK = (2 * ac.CASES[name][0] + 1) ** 2
    return slice(i * KK, (i + 1) * KK)
