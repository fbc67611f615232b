"""tests/presplit_ref.py on the CPU: the position map against its own statement (injective, inverse,
the 7 L zero positions, whole groups per wave) and the hi / lo split against its contract (22 bits,
NaN and signed zeros) -- what tests/test_lookup_consumers_gpu.py then holds the kernel to.
"""
import numpy as np
import pytest

import presplit_ref as pr
import prng

LEVELS = (1, 2, 3, 4)


@pytest.mark.parametrize("L", LEVELS)
def test_pos_is_injective_and_chan_its_inverse(L):
    ch = np.arange(81 * L)
    at = pr.pos(ch, L)
    assert at.min() >= 0 and at.max() < 88 * L
    assert np.unique(at).size == 81 * L
    assert np.array_equal(pr.chan(at, L), ch)
    for c in (0, 23, 24, 26, 27, 80, 81 * L - 1):   # scalars too
        assert int(pr.chan(pr.pos(c, L), L)) == c


@pytest.mark.parametrize("L", LEVELS)
def test_zero_positions_are_9_to_15_of_each_leftover_pair(L):
    ch = pr.chan(np.arange(88 * L), L)
    zero = np.flatnonzero(ch < 0)
    assert zero.size == 7 * L
    want = np.concatenate([72 * L + 16 * lv + np.arange(9, 16) for lv in range(L)])
    assert np.array_equal(zero, want)
    # and the leftover pair of level lv holds that level's channels 24 .. 26 of parts 0, 1, 2
    for lv in range(L):
        got = ch[72 * L + 16 * lv:72 * L + 16 * lv + 9]
        assert np.array_equal(got, [81 * lv + 27 * part + 24 + i for part in range(3) for i in range(3)])
    assert np.array_equal(pr.padding(L).reshape(-1), ch < 0)


@pytest.mark.parametrize("L", LEVELS)
def test_groups_below_72L_belong_to_one_level_and_part(L):
    ch = pr.chan(np.arange(72 * L), L).reshape(9 * L, 8)
    assert (ch >= 0).all()
    lv, part = ch // 81, ch % 81 // 27
    assert (lv == lv[:, :1]).all() and (part == part[:, :1]).all()
    assert np.array_equal(lv[:, 0] * 3 + part[:, 0], np.arange(9 * L) // 3)   # group 9 lv + 3 part + j
    assert (np.diff(ch, axis=1) == 1).all()                                  # k = 8 j .. 8 j + 7 in order


def test_group_and_byte_counts():
    assert [pr.groups(L) for L in LEVELS] == [12, 22, 34, 44]
    assert [int(pr.written(L).sum()) for L in LEVELS] == [11, 22, 33, 44]
    assert pr.bytes_per_item(3, 920) == 34 * 2 * 920 * 16


@pytest.mark.parametrize("L", LEVELS)
def test_decode_of_encode_carries_22_bits(L):
    B, Q = 2, 37
    x = prng.normal(700 + L, (B, 81 * L, Q)) * np.float32(3.0)
    # y = |x| 2^s in [2^-4, 2^15): hi is a normal half, |y - hi| <= 2^-11 y; lo = half(y - hi) errs by
    # 2^-11 of that (2^-22 y) while it is a normal half and by at most half the subnormal spacing,
    # 2^-25 <= 2^-21 * 2^-4, once it is not -- the samples below 2^-4 are left out of the bound
    m = np.abs(x).max(axis=1)
    s = (14 - np.ceil(np.log2(m))).astype(np.int32) - (np.arange(Q, dtype=np.int32) % 5)[None, :]
    y = np.abs(x.astype(np.float64)) * np.exp2(s)[:, None, :]
    keep = y >= 2.0 ** -4
    assert y.max() < 2.0 ** 15 and keep.mean() > 0.9
    buf = pr.encode(x, s, poison=0x7E7E)
    assert buf.shape == (B, pr.groups(L), 2, Q, 8) and buf.dtype == np.uint16
    assert buf.nbytes == B * pr.bytes_per_item(L, Q)
    back = pr.decode(buf, s)
    assert back.dtype == np.float64 and back.shape == x.shape
    err = np.abs(back - x.astype(np.float64))
    assert (err[keep] <= 2.0 ** -21 * np.abs(x.astype(np.float64))[keep]).all()
    # the padding is zero, the groups from 11 L on keep the poison
    pad = pr.padding(L)
    assert (buf[:, :11 * L].transpose(0, 2, 3, 1, 4)[..., pad] == 0).all()
    assert (buf[:, 11 * L:] == 0x7E7E).all()
    assert not (buf[:, :11 * L] == 0x7E7E).any()


def test_encode_of_nan_and_signed_zero():
    L, Q = 1, 4
    x = np.ones((1, 81, Q), dtype=np.float32)
    x[0, 5, 0] = np.nan       # a whole-group channel
    x[0, 26, 0] = np.nan      # a leftover channel
    x[0, 7, 1] = 0.0
    x[0, 8, 1] = -0.0
    x[0, 9, 2] = np.inf       # hi = inf, lo = inf - inf
    s = np.array([[3, -2, 0, 5]], dtype=np.int32)
    buf = pr.encode(x, s).view(np.float16)
    for c, q in ((5, 0), (26, 0)):
        g, e = divmod(int(pr.pos(c, L)), 8)
        assert np.isnan(buf[0, g, 0, q, e]) and np.isnan(buf[0, g, 1, q, e])
    raw = buf.view(np.uint16)
    g, e = divmod(int(pr.pos(7, L)), 8)
    assert raw[0, g, 0, 1, e] == 0 and raw[0, g, 1, 1, e] == 0
    g, e = divmod(int(pr.pos(8, L)), 8)
    assert raw[0, g, 0, 1, e] == 0x8000 and raw[0, g, 1, 1, e] == 0   # hi = -0, lo = -0 - -0 = +0
    g, e = divmod(int(pr.pos(9, L)), 8)
    assert np.isinf(buf[0, g, 0, 2, e]) and np.isnan(buf[0, g, 1, 2, e])
    # everything else of query 3 is 1 * 2^5 exactly: hi = 32, lo = 0
    d = pr.decode(raw, s)
    assert (d[0, :, 3] == 1.0).all()
    assert np.isnan(d[0, 5, 0]) and np.isnan(d[0, 26, 0]) and d[0, 7, 1] == 0.0 and d[0, 8, 1] == 0.0
