"""Cases, inputs and comparisons of the forward build sweep (test infrastructure, numpy only).

Shared by tests/test_build_cases_ref.py (the oracle pinned on integers, the comparisons shown to
reject corrupted references, on the CPU) and tests/test_build_sweep_gpu.py (every GEMM kernel of
csrc/build.hip against the oracle), so both build the same fields.

Which kernels serve a build (launch_build, csrc/build.hip), with dc = ceil(D / 16) K chunks:
    split mode (ecorr_build_split)
        build_split16_kernel   dc == 16, i.e. D = 241 .. 256 -- not D == 256 alone
        build_split_kernel     every other D
        <MUL>                  sqrtf(D) a power of two (the scale is then a multiply, else __fdiv_rn);
                               among D = 241 .. 256 only 256, so build_split16_kernel<!MUL> serves
                               exactly D = 241 .. 255
        operand pass           pack_both_kernel keeps a thread's values in registers for dc <= 16
                               and reads them a second time for dc > 16 (D > 256)
    fp32 mode (ecorr_build)
        build_f32_kernel       D == 256, W % 4 == 0, fmap2 16-byte aligned, both operands of a batch
                               item below 0x7fff0000 bytes.  D == 256 implies MUL, so
                               build_f32_kernel<false> is unreachable.  The alignment of fmap1 does
                               not enter: the kernel loads fmap1 as dwords, so a misaligned fmap1 at
                               D = 256 stays on this kernel (case f32_d256_mis1_8x8).
        build_kernel<vec, glds>   vec  = W % 4 == 0, q_count % 4 == 0, both fmaps 16-byte aligned
                                  glds = vec and both operands below 0x7fff0000 bytes
KERNEL-wise, REQUIRED lists what the table must reach of every kernel: D classes, the scale form,
tile geometry (tile_counts), query slabs, levels and batch sizes; coverage() is asserted at import,
so a case deleted from the table fails the CPU suite instead of silently covering less.

Two input sets per case, both from tests/prng.py:
    exact    integers in [-7, 7]; in every batch item one all-zero pixel and one pixel of all +-7
             per map (the same sign pattern in both maps: their dot product is 49 D, the largest
             sum there is).  Every product and partial sum is an integer below 2^24 under any
             summation order and any per-pixel power-of-two scale, the f16 lo halves are 0 and the
             kernels end in __fdiv_rn or an exact multiply: level 0 must equal the oracle bit for
             bit, the pooled levels the oracle's pools of it.
    normal   PRNG normals: level 0 within GEMM_TOL normwise of the fp64 oracle, the pooled levels
             bit-exact from the level 0 the kernel wrote.
"""
import functools
import zlib

import numpy as np

import oracle
import prng
from gpu_guard import mismatch

GEMM_TOL = 1e-5           # the project's bar for level 0 (tests/test_build_modes_gpu.py)
OPERAND_LIMIT = 0x7fff0000
SETS = ("exact", "normal")

# name: (mode, B, D, H, W, levels, q_begin, q_count, misalign); q_count < H * W: a slab of queries
# [q_begin, q_begin + q_count) of fmap1; misalign: 0, or 1 / 2 = fmap1 / fmap2 handed over as a
# view that starts 4 bytes into its buffer
CASES = {
    # ---- split mode, build_split_kernel: D = 1, 5, 16, 17, 64, 240 (dc = 15), 257 (dc = 17), 513
    "s_d1_1x1": ("split", 1, 1, 1, 1, 1, 0, 1, 0),
    "s_d5_2x3_l2": ("split", 2, 5, 2, 3, 2, 0, 6, 0),
    "s_d5_7x5_b1": ("split", 1, 5, 7, 5, 2, 0, 35, 0),             # odd batch stride (D * H * W = 175)
    "s_d5_7x5_b2": ("split", 2, 5, 7, 5, 3, 0, 35, 0),
    "s_d5_7x5_b3": ("split", 3, 5, 7, 5, 3, 0, 35, 0),
    "s_d16_8x8_l3": ("split", 2, 16, 8, 8, 3, 0, 64, 0),           # one K chunk exactly, one n-tile
    "s_d17_9x32_l4": ("split", 1, 17, 9, 32, 4, 0, 288, 0),        # band of 1 row, 2 n-tile columns
    "s_d64_12x40_l4": ("split", 2, 64, 12, 40, 4, 0, 480, 0),      # MUL; band of 4 rows, W % 32 != 0, 3 columns
    "s_d240_13x8_l2": ("split", 1, 240, 13, 8, 2, 0, 104, 0),      # padded tile row (5 of 8)
    "s_d257_15x32_l4": ("split", 1, 257, 15, 32, 4, 0, 480, 0),    # re-read operand pass; padded (7 of 8)
    "s_d513_8x40_l3": ("split", 1, 513, 8, 40, 3, 0, 320, 0),      # 3 n-tile columns: an odd pair tail
    "s_d17_slab_12x40": ("split", 2, 17, 12, 40, 3, 70, 148, 0),   # slab: starts mid-group, ends mid-row
    "s_d257_slab37_9x32": ("split", 1, 257, 9, 32, 2, 100, 37, 0),
    "s_d513_slab_12x40_l1": ("split", 2, 513, 12, 40, 1, 70, 148, 0),
    # ---- split mode, build_split16_kernel: D = 241, 250, 255 (<!MUL>) and 256 (<MUL>)
    "s16_d241_1x1": ("split", 1, 241, 1, 1, 1, 0, 1, 0),
    "s16_d241_2x3_l2": ("split", 2, 241, 2, 3, 2, 0, 6, 0),
    "s16_d241_7x5_b1": ("split", 1, 241, 7, 5, 2, 0, 35, 0),
    "s16_d241_7x5_b2": ("split", 2, 241, 7, 5, 3, 0, 35, 0),
    "s16_d241_7x5_b3": ("split", 3, 241, 7, 5, 3, 0, 35, 0),
    "s16_d250_8x8_l3": ("split", 2, 250, 8, 8, 3, 0, 64, 0),
    "s16_d250_9x32_l4": ("split", 1, 250, 9, 32, 4, 0, 288, 0),
    "s16_d255_12x40_l4": ("split", 1, 255, 12, 40, 4, 0, 480, 0),
    "s16_d255_13x8_l2": ("split", 1, 255, 13, 8, 2, 0, 104, 0),
    "s16_d256_15x32_l4": ("split", 1, 256, 15, 32, 4, 0, 480, 0),
    "s16_d256_8x40_l1": ("split", 1, 256, 8, 40, 1, 0, 320, 0),
    "s16_d241_slab_12x40": ("split", 2, 241, 12, 40, 3, 70, 148, 0),
    "s16_d256_slab37_9x32": ("split", 1, 256, 9, 32, 2, 100, 37, 0),
    # ---- fp32 mode, build_kernel<true, true>: D = 1, 17, 64, 255, 257, 513
    "f_tt_d1_8x8_l3": ("fp32", 2, 1, 8, 8, 3, 0, 64, 0),
    "f_tt_d17_9x32_l4": ("fp32", 1, 17, 9, 32, 4, 0, 288, 0),
    "f_tt_d64_12x40_l4": ("fp32", 2, 64, 12, 40, 4, 0, 480, 0),
    "f_tt_d255_13x8_l2": ("fp32", 1, 255, 13, 8, 2, 0, 104, 0),
    "f_tt_d257_15x32_l4": ("fp32", 1, 257, 15, 32, 4, 0, 480, 0),
    "f_tt_d513_8x40_l1": ("fp32", 1, 513, 8, 40, 1, 0, 320, 0),
    "f_tt_d17_slab_12x40": ("fp32", 2, 17, 12, 40, 3, 72, 148, 0),   # q_count % 4 == 0, yet no whole rows
    # ---- fp32 mode, build_kernel<false, false>: D = 5, 100, 256, 300, by each of its conditions
    "f_ff_d5_1x1": ("fp32", 1, 5, 1, 1, 1, 0, 1, 0),                 # W % 4 != 0
    "f_ff_d100_2x3_l2": ("fp32", 2, 100, 2, 3, 2, 0, 6, 0),
    "f_ff_d5_7x5_b1": ("fp32", 1, 5, 7, 5, 2, 0, 35, 0),
    "f_ff_d5_7x5_b2": ("fp32", 2, 5, 7, 5, 3, 0, 35, 0),
    "f_ff_d5_7x5_b3": ("fp32", 3, 5, 7, 5, 3, 0, 35, 0),
    "f_ff_d5_8x7_l3": ("fp32", 2, 5, 8, 7, 3, 0, 56, 0),
    "f_ff_d100_9x30_l4": ("fp32", 1, 100, 9, 30, 4, 0, 270, 0),
    "f_ff_d300_12x39_l4": ("fp32", 1, 300, 12, 39, 4, 0, 468, 0),
    "f_ff_d256_13x7_l2": ("fp32", 1, 256, 13, 7, 2, 0, 91, 0),
    "f_ff_d256_15x30_l4": ("fp32", 1, 256, 15, 30, 4, 0, 450, 0),
    "f_ff_d300_slab_12x39": ("fp32", 2, 300, 12, 39, 3, 70, 149, 0),
    "f_ff_d100_slab37_9x32": ("fp32", 1, 100, 9, 32, 2, 100, 37, 0),     # q_count % 4 != 0 alone
    "f_ff_d300_slab37_12x40_l1": ("fp32", 2, 300, 12, 40, 1, 70, 37, 0),
    "f_ff_d100_mis1_8x8": ("fp32", 2, 100, 8, 8, 3, 0, 64, 1),           # a misaligned fmap1 alone
    "f_ff_d256_mis2_8x8": ("fp32", 2, 256, 8, 8, 3, 0, 64, 2),           # a misaligned fmap2 alone, off build_f32_kernel
    # ---- fp32 mode, build_f32_kernel (D = 256): whole maps and slabs
    "f32_d256_8x8_l3": ("fp32", 2, 256, 8, 8, 3, 0, 64, 0),
    "f32_d256_9x32_l4": ("fp32", 1, 256, 9, 32, 4, 0, 288, 0),
    "f32_d256_12x40_l4": ("fp32", 1, 256, 12, 40, 4, 0, 480, 0),
    "f32_d256_13x8_l2": ("fp32", 1, 256, 13, 8, 2, 0, 104, 0),
    "f32_d256_15x32_l4": ("fp32", 1, 256, 15, 32, 4, 0, 480, 0),
    "f32_d256_8x40_l1": ("fp32", 1, 256, 8, 40, 1, 0, 320, 0),
    "f32_d256_slab37_9x32": ("fp32", 1, 256, 9, 32, 2, 100, 37, 0),
    "f32_d256_slab_12x40": ("fp32", 2, 256, 12, 40, 3, 70, 148, 0),
    "f32_d256_mis1_8x8": ("fp32", 2, 256, 8, 8, 3, 0, 64, 1),            # fmap1's alignment does not move it
    # ---- operands of 2 GiB per batch item (inputs made on the device): build_kernel<true, false>,
    #      and the same geometry through the split build
    "opsize_fp32": ("fp32", 1, 2048, 512, 512, 1, 0, 4, 0),
    "opsize_split": ("split", 1, 2048, 512, 512, 1, 0, 4, 0),
}
ON_DEVICE = ("opsize_fp32", "opsize_split")       # no host copy of their inputs
HOST_CASES = tuple(n for n in CASES if n not in ON_DEVICE)


def dc_of(D):
    return (D + 15) // 16


def scale_is_mul(D):
    """sqrtf(D) is a power of two (build_common, csrc/abi.hip: frexpf's mantissa is 0.5)."""
    mant, _ = np.frexp(np.sqrt(np.float32(D)))
    return bool(mant == np.float32(0.5))


def family_of(name):
    """The kernel of the case without its scale form: launch_build's rule from the case's numbers."""
    mode, B, D, H, W, L, q_begin, q, mis = CASES[name]
    if mode == "split":
        return "build_split16_kernel" if dc_of(D) == 16 else "build_split_kernel"
    small = D * H * W * 4 < OPERAND_LIMIT and D * q * 4 < OPERAND_LIMIT
    if D == 256 and W % 4 == 0 and mis != 2 and small:
        return "build_f32_kernel"
    vec = W % 4 == 0 and q % 4 == 0 and mis == 0
    return "build_kernel<%s, %s>" % ("true" if vec else "false", "true" if vec and small else "false")


def kernel_of(name):
    """The kernel instantiation launch_build picks for the case."""
    fam, D = family_of(name), CASES[name][2]
    if fam.startswith("build_kernel"):
        return fam        # one body: the scale form is a branch inside
    return "%s<%sMUL>" % (fam, "" if scale_is_mul(D) else "!")


def pack_path(name):
    """The operand pass's path (pack_body): None in fp32 mode."""
    mode, D = CASES[name][0], CASES[name][2]
    if mode != "split":
        return None
    return "register" if dc_of(D) <= 16 else "re-read"


def describe(name):
    """The text that names a failing case's code path."""
    p = pack_path(name)
    return kernel_of(name) + (f", operand pass: {p} path" if p else "")


def tags_of(name):
    """What of tile_counts' geometry, the query slab, the levels and the batch the case exercises."""
    mode, B, D, H, W, L, q_begin, q, mis = CASES[name]
    t = {"D=%d" % D, "L%d" % L, "MUL" if scale_is_mul(D) else "!MUL"}
    rem = H % 8
    band = 0 < rem <= 4
    if (H, W) == (1, 1):
        t.add("1x1")
    elif (H, W) == (2, 3):
        t.add("2x3")
    else:
        t.add("h%8=0" if rem == 0 else ("band%d" if band else "pad%d") % rem)
        t.add("ntx%d" % ((W + 15) // 16))          # n-tile columns
        if band and W % 32 != 0:
            t.add("band,w%32")
    if q < 128:
        t.add("q<128")
    if 128 < q < 256:
        t.add("128<q<256")
    if q > 256 and q % 128 != 0:
        t.add("q>256,q%128")
    if q != H * W:
        t.add("slab")
        if q_begin % 64 != 0:
            t.add("q_begin%64")
        if q_begin % W != 0 or q % W != 0:
            t.add("part_rows")
        if q == 37:
            t.add("slab37")
    if D % 2 == 1 and (H * W) % 2 == 1 and q % 2 == 1:
        t.add("B%d,odd_stride" % B)
    if W % 4 != 0:
        t.add("w%4")
    if q % 4 != 0:
        t.add("q%4")
    if mis:
        t.add("mis_f%d" % mis)
    if pack_path(name):
        t.add("pack:" + pack_path(name))
    return t


_GEOMETRY = ("h%8=0", "band1", "band4", "pad5", "pad7", "ntx1", "ntx2", "ntx3", "band,w%32")
_QUERIES = ("q<128", "128<q<256", "q>256,q%128", "q_begin%64", "part_rows")
_LEVELS = ("L1", "L2", "L3", "L4")
_BATCH = ("B1,odd_stride", "B2,odd_stride", "B3,odd_stride")
_SMALL_MAPS = ("1x1", "2x3")
# kernel family: the tags some case of that family must carry.  1 x 1 and 2 x 3 maps and odd batch
# strides need W % 4 != 0, so build_f32_kernel and build_kernel<true, true> cannot see them.
REQUIRED = {
    "build_split_kernel": ("D=1", "D=5", "D=16", "D=17", "D=64", "D=240", "D=257", "D=513", "D=2048", "MUL", "!MUL",
                           "pack:register", "pack:re-read") + _GEOMETRY + _QUERIES + _LEVELS + _BATCH + _SMALL_MAPS,
    "build_split16_kernel": ("D=241", "D=250", "D=255", "D=256", "MUL", "!MUL") + _GEOMETRY + _QUERIES + _LEVELS
                            + _BATCH + _SMALL_MAPS,
    "build_kernel<true, true>": ("D=1", "D=17", "D=64", "D=255", "D=257", "D=513") + _GEOMETRY + _QUERIES + _LEVELS,
    "build_kernel<false, false>": ("D=5", "D=100", "D=256", "D=300", "w%4", "slab37", "mis_f1", "mis_f2") + _GEOMETRY
                                  + _QUERIES + _LEVELS + _BATCH + _SMALL_MAPS,
    "build_f32_kernel": ("D=256", "slab37", "mis_f1") + _GEOMETRY + _QUERIES + _LEVELS,
    "build_kernel<true, false>": ("D=2048",),
}


def coverage():
    """{(family, tag): the cases that reach it} for every cell of REQUIRED."""
    fam = {n: family_of(n) for n in CASES}
    tags = {n: tags_of(n) for n in CASES}
    return {(k, t): tuple(n for n in CASES if fam[n] == k and t in tags[n]) for k, ts in REQUIRED.items() for t in ts}


def assert_coverage():
    missing = [cell for cell, names in coverage().items() if not names]
    assert not missing, f"no build case reaches {missing}"
    assert set(family_of(n) for n in CASES) == set(REQUIRED), "a case runs a kernel REQUIRED does not list"
    # the conditions that choose build_kernel<false, false> each act alone in some case
    alone = {"w%4": False, "q%4": False, "mis_f1": False, "mis_f2": False}
    for n in CASES:
        if family_of(n) == "build_kernel<false, false>":
            hit = [c for c in alone if c in tags_of(n)]
            if len(hit) == 1:
                alone[hit[0]] = True
    assert all(alone.values()), f"build_kernel<false, false> is never chosen by one condition alone: {alone}"
    # alignment alone moves D = 256 off build_f32_kernel
    assert kernel_of("f_ff_d256_mis2_8x8") == "build_kernel<false, false>"
    assert kernel_of("f32_d256_mis1_8x8") == "build_f32_kernel<MUL>"
    assert kernel_of("opsize_fp32") == "build_kernel<true, false>"
    assert (kernel_of("opsize_split"), pack_path("opsize_split")) == ("build_split_kernel<!MUL>", "re-read")
    # build_split16_kernel<!MUL> is exactly D = 241 .. 255; build_f32_kernel<!MUL> does not exist
    assert all(dc_of(D) == 16 and not scale_is_mul(D) for D in range(241, 256)) and scale_is_mul(256)
    assert dc_of(240) == 15 and dc_of(257) == 17
    assert not any(kernel_of(n) == "build_f32_kernel<!MUL>" for n in CASES)


for _n, (_mode, _B, _D, _H, _W, _L, _qb, _q, _mis) in CASES.items():
    assert _mode in ("split", "fp32") and 0 < _q and _qb + _q <= _H * _W, _n
    assert (_H >> (_L - 1)) >= 1 and (_W >> (_L - 1)) >= 1, f"{_n}: level {_L - 1} is empty"
    assert 49 * _D < 2 ** 24, f"{_n}: the exact set's sums no longer fit 24 bits"
    if _n not in ON_DEVICE:   # small maps: each case well under a second on the device
        assert _H <= 40 and _W <= 40 and _B <= 3, _n
        assert _B * _q * _H * _W * _D <= 2.5e8, f"{_n}: too much work for a sweep case"
assert_coverage()


# ---- inputs ----------------------------------------------------------------------------------

def seed_of(name):
    """The case's first seed, from its name: adding a case leaves the others' inputs as they were."""
    return 5000 + 10 * (zlib.crc32(name.encode()) % 100000)


def planted(name):
    """(query zero pixel, query +-7 pixel, target zero pixel, target +-7 pixel) as flat pixel indices
    of the whole map; the zero pixel is None where the slab / the map has one pixel only.  The
    target pair are neighbours in one row (the +-7 pixel to the right) wherever W >= 2."""
    _, _, _, H, W, _, q_begin, q, _ = CASES[name]
    t0 = (H // 2) * W + max(0, W // 2 - 1)
    qz, q7 = (q_begin, q_begin + 1) if q >= 2 else (None, q_begin)
    tz, t7 = (t0, t0 + 1) if H * W >= 2 else (None, 0)
    return qz, q7, tz, t7


def signs7(name):
    """The +-7 pattern of the planted pixels, [D] float32."""
    D = CASES[name][2]
    return np.where(prng.splitmix64(seed_of(name) + 2, D) & np.uint64(1), 7.0, -7.0).astype(np.float32)


def _freeze(*arrays):
    for a in arrays:
        a.setflags(write=False)
    return arrays


@functools.lru_cache(maxsize=4)
def fmaps(name, kind):
    """(fmap1, fmap2) [B, D, H, W] float32 of the whole map for the input set `kind`; read-only (shared)."""
    assert name not in ON_DEVICE and kind in SETS
    _, B, D, H, W, _, _, _, _ = CASES[name]
    s = seed_of(name)
    if kind == "normal":
        return _freeze(prng.normal(s + 5, (B, D, H, W)), prng.normal(s + 6, (B, D, H, W)))
    n = B * D * H * W
    maps = [((prng.splitmix64(s + i, n) % np.uint64(15)).astype(np.int64) - 7).astype(np.float32).reshape(B, D, H * W)
            for i in (0, 1)]
    qz, q7, tz, t7 = planted(name)
    for m, z, p in ((maps[0], qz, q7), (maps[1], tz, t7)):
        if z is not None:
            m[:, :, z] = 0.0
        m[:, :, p] = signs7(name)[None, :]
    return _freeze(*(m.reshape(B, D, H, W) for m in maps))


def slab(a, name):
    """[B, C, H, W] of the whole map -> the case's queries [B, C, q_count], contiguous."""
    _, B, _, H, W, _, q_begin, q, _ = CASES[name]
    return np.ascontiguousarray(a.reshape(B, a.shape[1], H * W)[:, :, q_begin:q_begin + q])


# ---- references and comparisons --------------------------------------------------------------

def reference_levels(name, f1, f2):
    """The oracle's pyramid of the case's queries: [B * q_count, h_i, w_i] per level (fp64 sums,
    one rounding, / sqrtf(D); 2 x 2 pools in the reference's order)."""
    _, _, _, _, _, L, q_begin, q, _ = CASES[name]
    return oracle.pyramid_from_level0(oracle.corr_level0(f1, f2, q_begin, q), L)


@functools.lru_cache(maxsize=4)
def reference(name, kind):
    """reference_levels of the case's own inputs, computed once and shared (read-only)."""
    return _freeze(*reference_levels(name, *fmaps(name, kind)))


def check_exact(levels, ref_levels):
    """The comparison of the exact set: None when every level equals the reference bit for bit,
    else a text naming the first level that differs and its first element (row, y, x)."""
    if len(levels) != len(ref_levels):
        return f"{len(levels)} levels, expected {len(ref_levels)}"
    for i, (got, want) in enumerate(zip(levels, ref_levels)):
        m = mismatch(got, want)
        if m is not None:
            return f"level {i} (elements are (query row, y, x)): {m}"
    return None


def check_normal(levels, truth0):
    """The comparison of the normal set -> (normwise error of level 0 against the fp64 oracle's
    level 0, None or the text of what failed): the error within GEMM_TOL, and every pooled level
    bit for bit the oracle's pool of the level 0 given."""
    err = oracle.normwise_err(levels[0], truth0)
    if not err <= GEMM_TOL:
        return err, f"level 0: normwise error {err:.3e} against fp64 exceeds {GEMM_TOL:g}"
    bad = check_exact(levels, oracle.pyramid_from_level0(levels[0], len(levels)))
    if bad is not None:
        return err, "against the pools of the level 0 written: " + bad
    return err, None


# ---- corrupted references (tests/test_build_cases_ref.py) ---------------------------------------

CORRUPTIONS = ("channel_dropped", "pixel_from_neighbour", "chunk_twice")


def corrupted_levels(name, kind, how):
    """The pyramid a subtly wrong build would write, or None where the case has no such error (a
    one-pixel map has no neighbour):
        channel_dropped       channel D - 1 missing from every sum
        pixel_from_neighbour  one target pixel's column (all queries) taken from the next pixel
        chunk_twice           the last K chunk, channels 16 (dc - 1) and up, summed twice
    On the exact set each changes the element (+-7 query, +-7 target), whose terms are all 49: the
    dropped channel by 49, the doubled chunk by 49 (D - 16 (dc - 1)); the moved column replaces the
    all-zero target pixel's zeros by its neighbour's, the +-7 pixel's, 49 D at the +-7 query."""
    _, B, D, H, W, L, q_begin, q, _ = CASES[name]
    f1, f2 = fmaps(name, kind)
    if how == "pixel_from_neighbour":
        _, _, tz, t7 = planted(name)
        if tz is None:
            return None
        lv0 = reference(name, kind)[0].reshape(B * q, H * W).copy()
        lv0[:, tz] = lv0[:, t7]
        return oracle.pyramid_from_level0(lv0.reshape(B * q, H, W), L)
    g1 = f1.copy()
    if how == "channel_dropped":
        g1[:, D - 1] = 0.0
    else:
        assert how == "chunk_twice"
        g1[:, 16 * (dc_of(D) - 1):] *= np.float32(2.0)
    return reference_levels(name, g1, f2)
