"""Plain numpy reference of the presplit corr (test infrastructure, no GPU).

Written from the layout comment of e-raft_amd/csrc/ecorr_internal.h and the ABI text of
include/ecorr.h (ecorr_lookup_presplit), not from the kernel:

  radius 4, L <= 4 levels, C = 81 L channels at K = 88 L positions.  Channel ch = 81 lv + 27 part + k
  (k < 27) sits at position
      72 lv + 24 part + k                 for k < 24
      72 L + 16 lv + 3 part + (k - 24)    for k >= 24   (a level's 9 last channels in 2 groups of 8:
                                                         positions 9 .. 15 of those 16 hold zeros)
  One batch item is [group][hi | lo][query][8 halves] with groups(L) = 2 ceil(88 L / 16) groups of 8
  positions, 16 bytes per (group, hi | lo, query); the groups from 11 L on are never written.
  A sample x of query p is stored as the binary16 pair
      y = float32(x) * float32(2^s_p),  hi = half(y),  lo = half(float32(y) - float32(hi))
  both converts round to nearest even and keep subnormals (numpy's float32 -> float16 cast does).

tests/test_presplit_ref.py checks this file on the CPU; tests/test_lookup_consumers_gpu.py holds the
kernel's buffer against encode() bit for bit.
"""
import numpy as np

POISON = 0x7E7E   # a binary16 NaN no convert produces: what a test fills the buffer with


def positions(L):
    return 88 * L


def groups(L):
    return 2 * ((88 * L + 15) // 16)


def bytes_per_item(L, Q):
    return groups(L) * 2 * Q * 16


def pos(ch, L):
    """Position of channel ch (int or integer array) among the 88 L positions."""
    ch = np.asarray(ch)
    lv, r = ch // 81, ch % 81
    part, k = r // 27, r % 27
    return np.where(k < 24, 72 * lv + 24 * part + k, 72 * L + 16 * lv + 3 * part + (k - 24))


def chan(p, L):
    """The inverse: the channel at position p (int or integer array), -1 for a zero position."""
    p = np.asarray(p)
    lv, r = p // 72, p % 72
    body = 81 * lv + 27 * (r // 24) + r % 24
    j = p - 72 * L
    lvl, rl = j // 16, j % 16
    left = np.where((lvl < L) & (rl < 9), 81 * lvl + 27 * (rl // 3) + 24 + rl % 3, -1)
    return np.where(p < 72 * L, body, left)


def split(x, scale):
    """x [B, C, Q] float32, scale [B, Q] int32 -> (hi, lo) [B, C, Q] float16."""
    x = np.asarray(x, dtype=np.float32)
    scale = np.asarray(scale, dtype=np.int32)
    assert scale.min() >= -126 and scale.max() <= 127, "2^s must be a normal float32"
    with np.errstate(all="ignore"):
        y = x * np.ldexp(np.float32(1.0), scale)[:, None, :].astype(np.float32)
        assert y.dtype == np.float32
        hi = y.astype(np.float16)
        lo = (y - hi.astype(np.float32)).astype(np.float16)
    return hi, lo


def encode(x, scale, poison=POISON):
    """x [B, 81 L, Q] float32, scale [B, Q] int32 -> uint16 [B, groups(L), 2, Q, 8]: the buffer
    ecorr_lookup_presplit leaves in memory that held `poison` everywhere."""
    x = np.asarray(x, dtype=np.float32)
    B, C, Q = x.shape
    L = C // 81
    assert C == 81 * L and 1 <= L <= 4
    hi, lo = split(x, scale)
    P = positions(L)
    ch = chan(np.arange(P), L)
    src = np.where(ch >= 0, ch, 0)
    buf = np.full((B, groups(L), 2, Q, 8), poison, dtype=np.uint16)
    for half, v in enumerate((hi, lo)):
        at = v.view(np.uint16)[:, src, :]                 # [B, P, Q] in position order
        at[:, ch < 0, :] = 0                              # the padding positions
        buf[:, :P // 8, half] = at.reshape(B, P // 8, 8, Q).transpose(0, 1, 3, 2)
    return buf


def written(L):
    """[groups(L)] bool: the groups ecorr_lookup_presplit writes (the first 11 L)."""
    return np.arange(groups(L)) < 11 * L


def padding(L):
    """[11 L, 8] bool: the zero positions inside the written groups."""
    return chan(np.arange(88 * L), L).reshape(11 * L, 8) < 0


def decode(buf, scale):
    """uint16 [B, groups(L), 2, Q, 8] -> (hi + lo) * 2^-s as float64 [B, 81 L, Q], in channel order."""
    buf = np.asarray(buf, dtype=np.uint16)
    B, G, _, Q, _ = buf.shape
    L = [l for l in range(1, 5) if groups(l) == G][0]
    P = positions(L)
    v = buf[:, :P // 8].view(np.float16).astype(np.float64)           # [B, 11 L, 2, Q, 8]
    s = (v[:, :, 0] + v[:, :, 1]).transpose(0, 1, 3, 2).reshape(B, P, Q)   # position order
    at = pos(np.arange(81 * L), L)
    return s[:, at, :] * np.ldexp(1.0, -np.asarray(scale, dtype=np.int64))[:, None, :]
