"""The premise of the hi-only split build (include/ecorr.h, ecorr_build_split_*_hi): the split's lo half
of a float16 / bfloat16 element is +-0 exactly when the element is finite.

A numpy restatement, on bit patterns, of split_exponent and split_f16 (e-raft_amd/csrc/split_f16.h):
    e  = clamp(15 - E, -126, 126) for a pixel maximum m = f 2^E, f in [0.5, 1), finite and > 0; else 0
    xs = x * 2^e (fp32), hi = f16(xs), lo = f16(xs - hi)
For EVERY finite 16-bit pattern x and EVERY exponent e that a pixel maximum m >= |x| of the same dtype
can produce (m ranges over the dtype's finite values from |x| up; the operand pass takes the maximum
with fmaxf, which ignores NaNs), lo has no magnitude bit.  For +-inf (whose pixel maximum is inf: e = 0)
and for NaN (any e) lo is a NaN.  So for 16-bit fmaps "a lo half has a magnitude bit" and "an element is
not finite" are the same statement, which is what the operand pass's flag records.

Both fp32 multiply modes are covered: subnormal products kept (the HIP default on gfx950) and flushed."""
import numpy as np
import pytest

F16_MAX_E = 16      # frexp exponent of the largest finite float16 (65504 = 0.9995 * 2^16)
BF16_MAX_E = 128    # ... bfloat16


def _values(kind):
    """(patterns uint16[65536], their fp32 values)."""
    bits = np.arange(65536, dtype=np.uint32).astype(np.uint16)
    if kind == "f16":
        return bits, bits.view(np.float16).astype(np.float32)
    return bits, (bits.astype(np.uint32) << 16).view(np.float32)


def split_exponent(m):
    """split_f16.h: m >= 0 fp32 array -> e."""
    _, E = np.frexp(m)
    ok = (m > 0) & (m <= np.float32(3.4028235e38))
    e = np.where(ok, 15 - E, 0)
    return np.clip(e, -126, 126)


def exp2i(e):
    return ((np.asarray(e, dtype=np.int32) + 127) << 23).view(np.float32)


def split_lo_bits(x, e, flush):
    """Magnitude bits (uint16) of lo for fp32 values x at exponents e (arrays of one shape)."""
    with np.errstate(over="ignore", invalid="ignore", under="ignore"):
        xs = (x * exp2i(e)).astype(np.float32)
        if flush:
            tiny = np.abs(xs) < np.float32(2.0 ** -126)
            xs = np.where(tiny, np.copysign(np.float32(0), xs), xs)
        hi = xs.astype(np.float16)
        lo = (xs - hi.astype(np.float32)).astype(np.float16)
    return lo.view(np.uint16) & np.uint16(0x7fff), lo


def test_restated_exponent_rule():
    m = np.array([0.0, 1.0, 0.75, 65504.0, 2.0 ** -24, 2.0 ** -133, 3.3e38, np.inf, np.nan], dtype=np.float32)
    with np.errstate(invalid="ignore"):
        e = split_exponent(m)
    assert list(e) == [0, 14, 15, -1, 38, 126, -113, 0, 0]
    for mm, ee in zip(m[1:7], e[1:7]):
        if -126 < ee < 126:   # unclamped: the scaled maximum lies in [2^14, 2^15)
            assert 2.0 ** 14 <= float(mm) * 2.0 ** int(ee) < 2.0 ** 15


@pytest.mark.parametrize("flush", [False, True], ids=["denormals", "flushed"])
@pytest.mark.parametrize("kind,max_e", [("f16", F16_MAX_E), ("bf16", BF16_MAX_E)])
def test_lo_is_zero_for_every_finite_pattern_and_reachable_exponent(kind, max_e, flush):
    bits, x = _values(kind)
    finite = np.isfinite(x)
    x = x[finite]
    ax = np.abs(x)
    _, Ex = np.frexp(ax)                 # the smallest E a maximum >= |x| can have (x = 0: every E)
    min_e = int(np.frexp(ax[ax > 0].min())[1])
    Ex = np.where(ax > 0, Ex, min_e)
    checked = 0
    for E in range(min_e, max_e + 1):    # the pixel maximum's frexp exponent
        sel = Ex <= E
        # the rule on an actual maximum with that exponent, not a re-derivation: m = 0.5 * 2^E
        e = int(split_exponent(np.array([np.ldexp(np.float32(0.5), E)], dtype=np.float32))[0])
        mag, _ = split_lo_bits(x[sel], np.full(int(sel.sum()), e, dtype=np.int32), flush)
        bad = np.flatnonzero(mag)
        assert bad.size == 0, (kind, E, e, [hex(int(v)) for v in bits[finite][sel][bad[:4]]])
        checked += int(sel.sum())
    # an all-zero pixel: m = 0, e = 0
    mag, _ = split_lo_bits(np.array([0.0, -0.0], dtype=np.float32), np.zeros(2, dtype=np.int32), flush)
    assert not mag.any()
    assert int(sel.sum()) == x.size and checked > x.size   # the largest maxima admit every finite pattern


@pytest.mark.parametrize("kind,max_e", [("f16", F16_MAX_E), ("bf16", BF16_MAX_E)])
def test_lo_is_nan_for_inf_and_nan(kind, max_e):
    bits, x = _values(kind)
    inf = x[np.isinf(x)]
    assert inf.size == 2
    mag, lo = split_lo_bits(inf, np.zeros(2, dtype=np.int32), False)   # the pixel maximum is inf: e = 0
    assert np.isnan(lo).all() and mag.all()
    nan = x[np.isnan(x)]
    assert nan.size > 0
    min_e = -23 if kind == "f16" else -132
    for E in range(min_e, max_e + 1):   # fmaxf ignores the NaN: the maximum is any finite value of the pixel
        e = int(split_exponent(np.array([np.ldexp(np.float32(0.5), E)], dtype=np.float32))[0])
        mag, lo = split_lo_bits(nan, np.full(nan.size, e, dtype=np.int32), False)
        assert np.isnan(lo).all() and mag.all()


def test_full_significand_fp32_has_a_lo():
    """The contrast: an fp32 value with more than 11 significant bits keeps a non-zero lo."""
    x = np.array([1.0 + 2.0 ** -12, 3.14159274], dtype=np.float32)
    mag, _ = split_lo_bits(x, split_exponent(np.abs(x)), False)
    assert mag.all()
