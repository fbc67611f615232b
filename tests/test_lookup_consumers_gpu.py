"""The radius-4 lookup's three consumer forms against the oracle, bit for bit, on the GPU.

CorrBlock.lookup_conv1x1_relu runs none of the plain lookup kernels (tests/test_lookup_radius_gpu.py,
test_corr_gpu.py) but one of three siblings with stores and control flow of their own:
    ecorr_lookup_qmax at r = 4            lookup_cols_reg<4, 64, PAIR, QMAX>        (mode "split")
    ecorr_lookup_presplit                 lookup_cols_reg<4, 64, PAIR, false, PRESPLIT>   ("presplit")
    ecorr_lookup_conv1x1_relu[_packed]    lookup_conv_kernel (csrc/motion.hip)       ("fused")
Each runs here through the C ABI on the cases of tests/consumer_cases.py -- PAIR and !PAIR staging,
ragged 64- and 32-query blocks, a slab that starts inside an interleave group, 1 to 4 levels, and for
qmax a level 4, a tiled level 4 with a compact level 5, and an h = 1 level -- with the nine coordinate
sets of tests/lookup_radius_cases.py: smooth and sigma = 40 flows, whole blocks of NaN / +-inf / huge
coordinates, windows over all four borders, the integer grid, half pixels and the integers moved by
one ulp and by 1e-4.  The pyramid is built once per case and the reference, oracle.lookup on the
levels read back from it, once per (case, set).

Every output lies between two 4096-byte guards in a buffer prefilled with a NaN no kernel computes
(0x7FC0DEAD, halves 0x7E7E) and is compared as integers:
    qmax      out is the oracle; every qmax[b][3 lv + part][p] is the maximum of |out| over exactly
              that wave's 27 channels (0 where they are all NaN); the split conv fed these maxima is
              bitwise the conv that finds them itself (G = 18 at six levels: its second qmax loop).
    presplit  the buffer is tests/presplit_ref.py's encode() of the oracle under scales the test
              chooses (neighbouring queries differ): hi and lo halves, the zero padding, and the group
              past 11 L (L = 1, 3) still poison; the presplit conv on that buffer stays finite and
              within 1e-5 normwise of the fp64 conv, so it never consumes the unwritten group.
    fused     one-hot weights whose pick maps cover all C channels, O = 64 / 192 / 320 (a wave past O,
              a second 256-channel pass), with and without bias, packed and unpacked weight (the
              straddling 4-channel piece at C % 4 != 0): relu(oracle[pick] + bias) bit for bit, every
              output of a query with a non-finite sample NaN (0 x NaN enters the sum); dense weights
              within 1e-5 normwise of the fp64 conv at O = 320.
-s prints one line per (case, form): the elements compared, the NaN ones, the poison words left and
the guard words changed.
"""
import ctypes

import numpy as np
import pytest
import torch

import consumer_cases as cc
import oracle
import presplit_ref as pr
import prng
from gpu_guard import mismatch

pytestmark = pytest.mark.gpu

DEV = "cuda"
GUARD_WORDS = 4096 // 4     # 4096 bytes on each side of an output
POISON_F32 = 0x7FC0DEAD     # a float NaN (np.float32 view: payload 0xDEAD) no kernel computes
POISON_F16 = 0x7E7E         # a binary16 NaN no convert produces


@pytest.fixture(scope="module")
def ea():
    if not torch.cuda.is_available():
        pytest.fail("no HIP device visible")
    import eraft_amd
    eraft_amd.lib()
    return eraft_amd


class _Case:
    """One case's pyramid on the device, its coordinate sets and the oracle lookup of each."""

    def __init__(self, name):
        from eraft_amd import _lib
        from eraft_amd.layout import levels_of
        B, H, W, L, q_begin, q = cc.CASES[name]
        if name.endswith("_l6"):
            cc.assert_l6_formats()
        f1, f2 = cc.fmaps(name)
        d1 = torch.from_numpy(cc.slab(f1, name)).to(DEV)
        d2 = torch.from_numpy(f2).to(DEV)
        _, _, off = _lib.layout(B * q, H, W, L)
        self.pyr = _lib.build_pyramid(d1, d2, B, cc.D, H, W, q, L, off, "test build")
        # PAIR's other condition (lookup_takes_cols, launch_lookup_conv): every level 8-byte aligned
        aligned = self.pyr.data_ptr() % 8 == 0 and all(o % 2 == 0 for o in off[:L])
        assert aligned or not cc.PAIR[name], f"{name}: levels at {off}: the case no longer stages column pairs"
        torch.cuda.synchronize()
        levels = [lv[:, 0].cpu().numpy() for lv in levels_of(self.pyr, B * q, H, W, L)]
        self.coords = {s: cc.slab(c, name).reshape(B, 2, 1, q) for s, c in cc.coord_sets(name).items()}
        self.want = {}   # set -> [B, C, q] float32, computed once, never written
        for s, cs in self.coords.items():
            w = oracle.lookup(levels, cs, cc.R).reshape(B, cc.channels(name), q)
            w.setflags(write=False)
            self.want[s] = w
        h1 = cc.h1_level(name)
        if h1 is not None:   # what the case exists for: the reference makes the whole level NaN
            assert all(np.isnan(w[:, cc.KK * h1:cc.KK * (h1 + 1)]).all() for w in self.want.values())
        assert np.isnan(self.want["special"]).any() and np.isfinite(self.want["smooth"][:, :cc.KK]).all()


@pytest.fixture(scope="module")
def cases(ea):
    """name -> _Case, built once per module (the largest pyramid is 8 MB)."""
    cache = {}

    def get(name):
        if name not in cache:
            cache[name] = _Case(name)
        return cache[name]
    return get


def _guarded(nbytes, word):
    """(the whole int32 buffer, its middle nbytes as int32), `word` everywhere; 4096 bytes of guard on
    each side, so the middle keeps the allocation's alignment."""
    assert nbytes % 4 == 0
    n = nbytes // 4
    buf = torch.full((n + 2 * GUARD_WORDS,), word, dtype=torch.int32, device=DEV)
    return buf, buf[GUARD_WORDS:GUARD_WORDS + n]


class _Tally:
    """The figures of one (case, form): printed, then asserted."""

    def __init__(self, what):
        self.what, self.compared, self.nan, self.poison, self.guard, self.bad = what, 0, 0, 0, 0, []

    def read(self, buf, word, what):
        """The middle of a guarded buffer as numpy int32; counts the guard words changed."""
        host = buf.cpu().numpy()
        g = int((host[:GUARD_WORDS] != word).sum() + (host[-GUARD_WORDS:] != word).sum())
        if g:
            self.guard += g
            self.bad.append(f"{what}: {g} guard words changed")
        return host[GUARD_WORDS:-GUARD_WORDS]

    def floats(self, buf, what):
        """The middle of a float output: no 0x7FC0DEAD left -> numpy float32."""
        mid = self.read(buf, POISON_F32, what)
        left = int((mid == POISON_F32).sum())
        if left:
            self.poison += left
            self.bad.append(f"{what}: {left} of {mid.size} elements were never written")
        return mid.view(np.float32)

    def same(self, got, want, what):
        """got and want [B, C, q] float32: the same bits up to NaN payloads."""
        self.compared += want.size
        self.nan += int(np.isnan(want).sum())
        m = mismatch(got, want)
        if m:
            self.bad.append(f"{what}: {m}")

    def done(self):
        print(f"\n{self.what}: {self.compared} elements compared, {self.nan} of them NaN, "
              f"{self.poison} poison words left, {self.guard} guard words changed")
        assert not self.bad, "; ".join(self.bad[:12])
        assert self.poison == 0 and self.guard == 0 and self.compared > 0


def _stream():
    return ctypes.c_void_p(torch.cuda.current_stream().cuda_stream)


def _weight(seed, O, C):
    return torch.from_numpy(prng.normal(seed, (O, C)) * np.float32(0.05)).to(DEV)


def _conv_ref(want, w, bias):
    """relu(w . want + bias) in float64: [B, O, q]."""
    r = np.einsum("oc,bcq->boq", w.double().cpu().numpy(), want.astype(np.float64))
    if bias is not None:
        r = r + bias.double().cpu().numpy()[None, :, None]
    return np.maximum(r, 0.0)


def _normwise(got, ref):
    return float(np.max(np.abs(got.astype(np.float64) - ref)) / np.sqrt(np.mean(ref * ref)))


# ---- ecorr_lookup_qmax at radius 4

def qmax_ref(want, L):
    """[B, 81 L, q] -> [B, 3 L, q]: row 3 lv + part = max(0, max |want| over the 27 channels
    81 lv + 27 part + k) with NaN ignored (fmaxf from 0)."""
    B, C, q = want.shape
    a = np.abs(want).reshape(B, 3 * L, 27, q)
    return np.fmax.reduce(a, axis=2, initial=np.float32(0.0))


@pytest.mark.parametrize("name", list(cc.CASES))
def test_qmax_lookup_and_every_partial_maximum(ea, cases, name):
    from eraft_amd import _lib
    B, H, W, L, _, q = cc.CASES[name]
    C, G, O = cc.channels(name), 3 * L, 96
    case = cases(name)
    lib = _lib.lib()
    w = _weight(cc.seed_of(name) + 5, O, C)
    pk = _lib.packed_conv1x1_weight(w, O, C, "split", _lib.stream_of(w), {})
    t = _Tally(f"{name} / qmax")
    for s in cc.SETS:
        what = f"{name} / {s}"
        c = torch.from_numpy(case.coords[s]).to(DEV)
        obuf, out = _guarded(B * C * q * 4, POISON_F32)
        qbuf, qm = _guarded(B * G * q * 4, POISON_F32)
        _lib.check(lib.ecorr_lookup_qmax(case.pyr.data_ptr(), c.data_ptr(), B, H, W, q, L, cc.R, out.data_ptr(),
                                         qm.data_ptr(), _stream()), "qmax lookup")
        torch.cuda.synchronize()
        want = case.want[s]
        t.same(t.floats(obuf, what + " out").reshape(B, C, q), want, what + " out")
        got = t.floats(qbuf, what + " qmax").reshape(B, G, q)
        ref = qmax_ref(want, L)
        assert not np.isnan(ref).any()
        t.compared += ref.size
        if np.isnan(got).any() or not np.array_equal(got.view(np.uint32), ref.view(np.uint32)):
            t.bad.append(f"{what} qmax (b, 3 lv + part, query): {mismatch(got, ref)}")
        h1 = cc.h1_level(name)
        if h1 is not None and (got[:, 3 * h1:3 * h1 + 3].view(np.uint32) != 0).any():
            t.bad.append(f"{what}: the maxima of the all-NaN level {h1} are not 0")
        # the split conv with these maxima is bitwise the conv that finds them itself
        a = torch.empty((B, O, q), dtype=torch.float32, device=DEV)
        b = torch.empty((B, O, q), dtype=torch.float32, device=DEV)
        for dst, qp in ((a, qm.data_ptr()), (b, None)):
            _lib.check(lib.ecorr_conv1x1_relu_split(out.data_ptr(), B, C, q, qp, G, pk.data_ptr(), None, O,
                                                    dst.data_ptr(), _stream()), "split conv")
        torch.cuda.synchronize()
        if not torch.equal(a.view(torch.int32), b.view(torch.int32)):
            t.bad.append(f"{what}: the split conv with qmax differs from the conv with qmax = NULL: "
                         f"{mismatch(a.cpu().numpy(), b.cpu().numpy())}")
    t.done()


# ---- ecorr_lookup_presplit

def presplit_scale(want):
    """[B, C, q] -> int32 [B, q]: s = 14 - ceil(log2(max |finite sample|)) - (p % 5), so |x| 2^s < 2^15
    and neighbouring queries differ; 0 for a query with no finite nonzero sample."""
    a = np.where(np.isfinite(want), np.abs(want.astype(np.float64)), 0.0).max(axis=1)
    some = a > 0.0
    s = 14 - np.ceil(np.log2(np.where(some, a, 1.0))).astype(np.int64) - (np.arange(want.shape[2]) % 5)[None, :]
    s = np.where(some, s, 0).astype(np.int32)
    assert (a * np.exp2(s) < 2.0 ** 15).all() and np.abs(s).max() <= 126
    return s


@pytest.mark.parametrize("name", cc.CONV_CASES)
def test_presplit_buffer_is_the_encoded_oracle(ea, cases, name):
    from eraft_amd import _lib
    B, H, W, L, _, q = cc.CASES[name]
    C = cc.channels(name)
    case = cases(name)
    lib = _lib.lib()
    n = ctypes.c_int64()
    _lib.check(lib.ecorr_presplit_size(B, L, q, ctypes.byref(n)), "presplit size")
    assert n.value == B * pr.bytes_per_item(L, q)
    G = pr.groups(L)
    pad = pr.padding(L)
    t = _Tally(f"{name} / presplit")
    for s in cc.SETS:
        what = f"{name} / {s}"
        want = case.want[s]
        scale_np = presplit_scale(want)
        if s == "smooth":
            assert len(np.unique(scale_np)) >= 5
        scale = torch.from_numpy(scale_np).to(DEV)
        c = torch.from_numpy(case.coords[s]).to(DEV)
        pbuf, pre = _guarded(n.value, POISON_F16 * 0x10001)
        _lib.check(lib.ecorr_lookup_presplit(case.pyr.data_ptr(), c.data_ptr(), B, H, W, q, L, cc.R,
                                             scale.data_ptr(), pre.data_ptr(), _stream()), "presplit lookup")
        torch.cuda.synchronize()
        got = t.read(pbuf, POISON_F16 * 0x10001, what).view(np.uint16).reshape(B, G, 2, q, 8)
        ref = pr.encode(want, scale_np, POISON_F16)
        gw, rw = got[:, :11 * L], ref[:, :11 * L]
        gn, rn = np.isnan(gw.view(np.float16)), np.isnan(rw.view(np.float16))
        bad = (gn != rn) | (~rn & (gw != rw))
        t.compared += rw.size
        t.nan += int(rn.sum())
        if bad.any():
            b, g, hl, p, e = np.argwhere(bad)[0]
            t.bad.append(f"{what}: {int(bad.sum())} of {bad.size} halves differ; first at (b, group, hi|lo, query, "
                         f"half) = ({b}, {g}, {hl}, {p}, {e}), channel {int(pr.chan(8 * g + e, L))}: got "
                         f"{gw[b, g, hl, p, e]:#06x}, expected {rw[b, g, hl, p, e]:#06x}, scale {scale_np[b, p]}")
        left = int((gw == POISON_F16).sum())
        if left:
            t.poison += left
            t.bad.append(f"{what}: {left} halves of the written groups were never written")
        z = gw.transpose(0, 2, 3, 1, 4)[..., pad]
        if (z != 0).any():
            t.bad.append(f"{what}: {int((z != 0).sum())} of {z.size} padding halves are not zero")
        if (got[:, 11 * L:] != POISON_F16).any():
            t.bad.append(f"{what}: {int((got[:, 11 * L:] != POISON_F16).sum())} halves of the groups from "
                         f"{11 * L} on were written")
        if s != "smooth":
            continue
        # the presplit conv on this buffer (its groups past 11 L still poison, a NaN)
        O, with_bias = (96, False) if L in (1, 3) else (256, True)
        w = _weight(cc.seed_of(name) + 6, O, C)
        bias = torch.from_numpy(prng.normal(cc.seed_of(name) + 7, (O,)) * np.float32(0.1)).to(DEV) if with_bias else None
        pk = _lib.packed_conv1x1_weight(w, O, C, "presplit", _lib.stream_of(w), {})
        obuf, out = _guarded(B * O * q * 4, POISON_F32)
        _lib.check(lib.ecorr_conv1x1_relu_presplit(pre.data_ptr(), B, L, q, scale.data_ptr(), pk.data_ptr(),
                                                   _lib.ptr(bias), O, out.data_ptr(), _stream()), "presplit conv")
        torch.cuda.synchronize()
        o = t.floats(obuf, what + " conv").reshape(B, O, q)
        fin = np.isfinite(want).all(axis=1)   # [B, q]
        assert fin.all(), f"{what}: the smooth set has non-finite samples"
        if not np.isfinite(o).all():
            t.bad.append(f"{what}: {int((~np.isfinite(o)).sum())} non-finite outputs of the presplit conv")
        else:
            err = _normwise(o, _conv_ref(want, w, bias))
            print(f"\n{what}: presplit conv O = {O}, normwise error {err:.3g}")
            if not err <= 1e-5:
                t.bad.append(f"{what}: presplit conv normwise error {err:.3g} > 1e-5")
    t.done()


# ---- ecorr_lookup_conv1x1_relu / _packed

FUSED_CONFIGS = [(O, b) for O in (320, 192, 64) for b in (True, False)]   # (O, with bias)


def pick_maps(C):
    """One pick map per FUSED_CONFIGS entry: output o of config j copies channel 7 (base_j + o) mod C,
    base_j = the outputs of the configs before it (7 is coprime to 81 L: a bijection of the channels)."""
    maps, base = [], 0
    for O, _ in FUSED_CONFIGS:
        maps.append((7 * (base + np.arange(O))) % C)
        base += O
    return maps


def _fused(lib, case, name, c, wt, packed, bias, O, what, t):
    """One fused launch into a guarded buffer -> [B, O, q] float32."""
    from eraft_amd import _lib
    B, H, W, L, _, q = cc.CASES[name]
    obuf, out = _guarded(B * O * q * 4, POISON_F32)
    fn = lib.ecorr_lookup_conv1x1_relu_packed if packed else lib.ecorr_lookup_conv1x1_relu
    _lib.check(fn(case.pyr.data_ptr(), c.data_ptr(), B, H, W, q, L, cc.R, wt.data_ptr(), _lib.ptr(bias), O,
                  out.data_ptr(), _stream()), what)
    torch.cuda.synchronize()
    return t.floats(obuf, what).reshape(B, O, q)


@pytest.mark.parametrize("name", cc.CONV_CASES)
def test_fused_one_hot_is_the_oracle(ea, cases, name):
    from eraft_amd import _lib
    B, H, W, L, _, q = cc.CASES[name]
    C = cc.channels(name)
    case = cases(name)
    lib = _lib.lib()
    maps = pick_maps(C)
    assert np.array_equal(np.unique(np.concatenate(maps)), np.arange(C)), "the pick maps miss channels"
    assert all(np.array_equal(np.unique(np.concatenate([m for m, (_, b) in zip(maps, FUSED_CONFIGS) if b == wb])),
                              np.arange(C)) for wb in (True, False)), "with / without bias: each covers all channels"
    cfg = []
    for j, ((O, with_bias), pick) in enumerate(zip(FUSED_CONFIGS, maps)):
        w = torch.zeros((O, C), dtype=torch.float32)
        w[torch.arange(O), torch.from_numpy(pick)] = 1.0
        w = w.to(DEV)
        bias_np = prng.normal(cc.seed_of(name) + 20 + j, (O,)) if with_bias else None
        bias = torch.from_numpy(bias_np).to(DEV) if with_bias else None
        pk = _lib.packed_conv1x1_weight(w, O, C, "fused", _lib.stream_of(w), {})
        cfg.append((O, pick, w, pk, bias, bias_np))
    t = _Tally(f"{name} / fused")
    for s in cc.SETS:
        want = case.want[s]
        badq = ~np.isfinite(want).all(axis=1)   # [B, q]: 0 x NaN enters every sum of the query
        c = torch.from_numpy(case.coords[s]).to(DEV)
        for O, pick, w, pk, bias, bias_np in cfg:
            what = f"{name} / {s} / O = {O}, {'bias' if bias is not None else 'no bias'}"
            with np.errstate(invalid="ignore"):
                v = want[:, pick, :] + (bias_np[None, :, None] if bias_np is not None else np.float32(0.0))
                assert v.dtype == np.float32
                exp = np.where(v < 0, np.float32(0.0), v)   # NaN stays NaN
            exp = np.where(badq[:, None, :], np.float32(np.nan), exp)
            a = _fused(lib, case, name, c, pk, True, bias, O, what + " packed", t)
            b = _fused(lib, case, name, c, w, False, bias, O, what + " unpacked", t)
            t.same(a, exp, what + " packed")
            if not np.array_equal(a.view(np.uint32), b.view(np.uint32)):
                t.bad.append(f"{what}: packed and unpacked differ: {mismatch(b, a)}")
    t.done()


@pytest.mark.parametrize("name", ["l1_20x20", "l3_23x40", "slab_17x20"])
def test_fused_dense_normwise(ea, cases, name):
    from eraft_amd import _lib
    B, H, W, L, _, q = cc.CASES[name]
    C, O = cc.channels(name), 320
    case = cases(name)
    lib = _lib.lib()
    w = _weight(cc.seed_of(name) + 8, O, C)
    bias = torch.from_numpy(prng.normal(cc.seed_of(name) + 9, (O,)) * np.float32(0.1)).to(DEV)
    pk = _lib.packed_conv1x1_weight(w, O, C, "fused", _lib.stream_of(w), {})
    t = _Tally(f"{name} / fused dense")
    for s in ("smooth", "iid_large"):
        what = f"{name} / {s}"
        want = case.want[s]
        assert np.isfinite(want).all()
        ref = _conv_ref(want, w, bias)
        c = torch.from_numpy(case.coords[s]).to(DEV)
        a = _fused(lib, case, name, c, pk, True, bias, O, what + " packed", t)
        b = _fused(lib, case, name, c, w, False, bias, O, what + " unpacked", t)
        for got, entry in ((a, "packed"), (b, "unpacked")):
            err = _normwise(got, ref)
            print(f"\n{what} / {entry}: normwise error {err:.3g}")
            t.compared += ref.size
            if not err <= 1e-5:
                t.bad.append(f"{what} / {entry}: normwise error {err:.3g} > 1e-5")
    t.done()
