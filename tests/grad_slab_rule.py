"""The Python mirror of the weight-gradient slab rule (csrc/grad_slab.h: gru_grad_slab, kGradWK, kGradChain,
kGradSlabs), shared by the CPU-side workspace formulas (test_gru_grad_abi.py, test_motion_enc_grad_abi.py) and by the
GPU tests that must reach the doubled cap and the second chain (test_gru_grad_gpu.py, test_motion_enc_grad_gpu.py).
Test infrastructure; no torch.

Within one batch item the pixel reduction is split into slabs: a cap of CHAIN pixels, doubled while the launch would
have more than SLABS slabs, then balanced slabs of whole chunks of WK pixels under the cap.  gru_wgrad_kernel and
menc_wgrad_kernel reduce a slab in chains of at most CHAIN pixels (CHAIN / WK chunks): a slab has a second chain only
after the cap has doubled.

SLAB_SHAPES: the smallest (B, H, W) that reach those branches, with the geometry each must have (SLAB_GEOMETRY):
  (33, 25, 41)  1025 pixels, 33 x 2 = 66 > 64 doubles the cap to 2048: one slab of 33 chunks, a chain of 32 and a
                second chain of one chunk that holds one valid pixel;
  (22, 33, 63)  2079 pixels, 22 x 3 = 66 > 64 doubles the cap to 2048 (22 x 2 = 44 stops): slab 0 of 1056 pixels is
                a chain of 32 chunks and a second chain of one full chunk, slab 1 of 1023 pixels one chain whose last
                chunk holds 31 pixels; 44 slabs in the launch.
"""
WK = 32         # kGradWK: pixels per chunk
CHAIN = 1024    # kGradChain: pixels per chain, and the undoubled cap
SLABS = 64      # kGradSlabs

SLAB_SHAPES = [(33, 25, 41), (22, 33, 63)]
# shape -> (cap, nsl, slab, per slab (pixels, chunks, chains))
SLAB_GEOMETRY = {
    (33, 25, 41): (2048, 1, 1056, [(1025, 33, 2)]),
    (22, 33, 63): (2048, 2, 1056, [(1056, 33, 2), (1023, 32, 1)]),
}


def slab_rule(B, P):
    """(cap, nsl, slab, chains) of B items of P pixels: the final cap, the slabs per item, the pixels per slab (the
    last one of an item may hold fewer) and the chains of the longest slab."""
    cap = CHAIN
    while cap < P and B * -(-P // cap) > SLABS:
        cap *= 2
    per = -(-P // cap)
    slab = -(-(-(-P // per)) // WK) * WK
    nsl = -(-P // slab)
    return cap, nsl, slab, max(c for _, _, c in slabs_of(P, nsl, slab))


def slabs_of(P, nsl, slab):
    """Per slab of one item: (pixels, chunks, chains)."""
    out = []
    for s in range(nsl):
        px = min(P, (s + 1) * slab) - s * slab
        chunks = -(-px // WK)
        out.append((px, chunks, -(-chunks // (CHAIN // WK))))
    return out


def assert_slab_shapes():
    """The table above holds under the rule: a change of the constants fails here instead of covering less."""
    for (B, H, W), (cap, nsl, slab, slabs) in SLAB_GEOMETRY.items():
        got = slab_rule(B, H * W)
        assert got == (cap, nsl, slab, 2), ((B, H, W), got)
        assert slabs_of(H * W, nsl, slab) == slabs, ((B, H, W), slabs_of(H * W, nsl, slab))
    assert sorted(SLAB_GEOMETRY) == sorted(SLAB_SHAPES)
    assert 1025 - 32 * WK == 1 and 1023 - 31 * WK == 31      # the one valid pixel; the ragged chunk of 31
    assert 22 * 2 == 44 <= SLABS


def assert_single_chain(shapes):
    """None of `shapes` doubles the cap or runs a second chain: why SLAB_SHAPES are needed beside them."""
    for B, H, W in shapes:
        cap, nsl, slab, chains = slab_rule(B, H * W)
        assert cap == CHAIN and slab <= CHAIN and chains == 1, ((B, H, W), cap, nsl, slab, chains)
