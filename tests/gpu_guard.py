"""Shared helpers of the bit-exact kernel tests (test infrastructure; torch only inside guarded()).

guarded / check_guarded: an output handed to a kernel lies in the middle of a buffer filled with one
bit pattern, GUARD floats of it on each side: a store outside the output changes a guard band, an
element the kernel never wrote keeps the pattern.
guarded_u8 / check_guarded_u8: the same for a byte output (the splat's valid mask), BYTE_FILL = 0x7b being
neither 0 nor 1.
guarded_u16 / check_guarded_u16: a uint16 output in the middle of a guarded_u8 buffer (the PNG codec's).
Workspace: a kernel's byte scratch of exactly the size its size entry reports, WS_GUARD bytes of guard
on each side, everything prefilled with a byte the caller chooses; a zero-byte one is passed as NULL.
mismatch: the text of a failed bitwise comparison.
GRID_STRIDE_THREADS: the threads of one pass of the generic kernels' grid-stride loops.
"""
import numpy as np

GUARD = 64            # floats on each side of an output (256 bytes: the output keeps its alignment)
FILL = 0x7b7b7b7b     # 1.3e36 as a float: finite, not NaN, and nothing the kernels under test compute
BYTE_FILL = 0x7b      # one byte of FILL
WS_GUARD = 4096       # bytes on each side of a workspace (a multiple of 256: the middle keeps its alignment);
                      # an overrun of a few hundred bytes still lands in the guard, not beyond it
GRID_STRIDE_THREADS = 8192 * 256   # grid_for() (csrc/lookup_kernels.h): at most 8192 blocks of NT = 256 threads


def guarded(n, device="cuda"):
    """(the whole int32 buffer, its middle n elements as float32), FILL everywhere."""
    import torch
    buf = torch.full((n + 2 * GUARD,), FILL, dtype=torch.int32, device=device)
    return buf, buf[GUARD:GUARD + n].view(torch.float32)


def check_guarded(buf, what):
    """Asserts the guards untouched and no element of the middle left unwritten -> the middle as
    numpy float32."""
    host = buf.cpu().numpy()
    assert (host[:GUARD] == FILL).all() and (host[-GUARD:] == FILL).all(), f"{what}: a guard band was written"
    mid = host[GUARD:-GUARD]
    left = int((mid == FILL).sum())
    assert left == 0, f"{what}: {left} of {mid.size} elements were never written"
    return mid.view(np.float32)


def guarded_u8(n, device="cuda"):
    """(the whole uint8 buffer, its middle n bytes), BYTE_FILL everywhere."""
    import torch
    buf = torch.full((n + 2 * 4 * GUARD,), BYTE_FILL, dtype=torch.uint8, device=device)
    return buf, buf[4 * GUARD:4 * GUARD + n]


def check_guarded_u8(buf, what):
    """As check_guarded for a guarded_u8 buffer -> the middle as numpy uint8."""
    host = buf.cpu().numpy()
    G = 4 * GUARD
    assert (host[:G] == BYTE_FILL).all() and (host[-G:] == BYTE_FILL).all(), f"{what}: a guard band was written"
    mid = host[G:-G]
    left = int((mid == BYTE_FILL).sum())
    assert left == 0, f"{what}: {left} of {mid.size} bytes were never written"
    return mid


def guarded_u16(n, device="cuda"):
    """(the whole uint8 buffer of guarded_u8(2 n), its middle as n uint16), BYTE_FILL everywhere."""
    import torch
    buf, mid = guarded_u8(2 * n, device)
    return buf, mid.view(torch.uint16)


def check_guarded_u16(buf, what):
    """Asserts the guards of a guarded_u16 buffer untouched -> the middle as numpy uint16.  A written
    element may be 0x7b7b itself (the DSEC codec's channels span the whole range), so what was never
    written shows in the caller's comparison of every element, not here."""
    host = buf.cpu().numpy()
    G = 4 * GUARD
    assert (host[:G] == BYTE_FILL).all() and (host[-G:] == BYTE_FILL).all(), f"{what}: a guard band was written"
    return host[G:-G].view(np.uint16)


class Workspace:
    """nbytes of scratch between two WS_GUARD-byte guards, everything the byte `fill`.  ptr: the
    middle's address (256-byte aligned), or None (NULL, as _lib.ptr(None)) for a zero-byte workspace."""

    def __init__(self, nbytes, fill, device="cuda"):
        import torch
        self.nbytes, self.fill = int(nbytes), fill
        self.buf = torch.full((self.nbytes + 2 * WS_GUARD,), fill, dtype=torch.uint8, device=device)
        middle = self.buf.data_ptr() + WS_GUARD
        assert middle % 256 == 0
        self.ptr = middle if self.nbytes else None

    def check(self, what):
        """Asserts both guards untouched."""
        lo, hi = self.buf[:WS_GUARD], self.buf[WS_GUARD + self.nbytes:]
        assert bool((lo == self.fill).all()) and bool((hi == self.fill).all()), \
            f"{what}: a workspace guard was written (workspace of {self.nbytes} bytes)"


def mismatch(got, want):
    """None when got and want ([B, C, ...] float32) are the same bits up to NaN payloads
    (oracle.same_bits), else a text: the count of differing elements and the first one's
    (b, channel, query) with both values."""
    got, want = np.asarray(got, dtype=np.float32), np.asarray(want, dtype=np.float32)
    if got.shape != want.shape:
        return f"shape {got.shape} != {want.shape}"
    ng, nw = np.isnan(got), np.isnan(want)
    bad = (ng != nw) | (~ng & ~nw & (got.view(np.uint32) != want.view(np.uint32)))
    n = int(bad.sum())
    if n == 0:
        return None
    B, C = got.shape[:2]
    b, c, q = np.argwhere(bad.reshape(B, C, -1))[0]
    g, w = got.reshape(B, C, -1)[b, c, q], want.reshape(B, C, -1)[b, c, q]
    return (f"{n} of {bad.size} elements differ; first at (b, channel, query) = ({b}, {c}, {q}): got {g!r} "
            f"({g.view(np.uint32):#010x}), expected {w!r} ({w.view(np.uint32):#010x})")
