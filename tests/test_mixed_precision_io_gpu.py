"""ERAFT(mixed_precision=True) with the CorrBlock 16-bit at both ends: fnet's amp_dtype fmaps go into the
block as they are (fmap_dtype=amp_dtype) and, with fuse_motion_corr, lookup_conv1x1_relu returns
amp_dtype (out_dtype=amp_dtype).

Arms under torch.no_grad(), at the smallest e2e golden's shape with its PRNG weights and inputs, iters=3:
  ours = ERAFT(mixed_precision=True, fuse_motion_corr=True)
  base = ERAFT(mixed_precision=True, fuse_motion_corr=True, _native_half_lookup=False): fmaps .float(),
         fp32 convc1 output, cast by autocast in front of convc2
with base run twice.  The 16-bit pack is bitwise the fp32 pack of the converted fmaps
(tests/test_fmap_half_gpu.py) and the conv's 16-bit store rounds the fp32 value as autocast's cast does
(tests/test_convc1_half_gpu.py), so ours and base compute the same numbers:
epe(ours, base1) <= 2 * epe(base1, base2) -- exact equality when MIOpen is run-to-run deterministic."""
import os

import numpy as np
import pytest
import torch

import prng
from conftest import GOLDEN
from e2e_weights import make_state_dict

pytestmark = pytest.mark.gpu

CASE = os.path.join(GOLDEN, "e2e_small_standard.npz")   # 128 x 160 events -> a 16 x 20 flow
DTYPES = [torch.float16, torch.bfloat16]
ITERS = 3


def epe(a, b):
    d = np.asarray(a, np.float64) - np.asarray(b, np.float64)
    return float(np.mean(np.sqrt(np.sum(d * d, axis=1))))


def _net(z, **kw):
    import eraft_amd.network as nw
    net = nw.ERAFT({"subtype": str(z["subtype"])}, n_first_channels=int(z["bins"]), **kw)
    net.load_state_dict(make_state_dict(net.state_dict()))
    return net.cuda()


def _inputs(z):
    H, W, bins, seed = int(z["H"]), int(z["W"]), int(z["bins"]), int(z["seed"])
    return (torch.from_numpy(prng.normal(seed, (1, bins, H, W))).cuda(),
            torch.from_numpy(prng.normal(seed + 1, (1, bins, H, W))).cuda())


def _forward(z, build_spy, conv_spy, **kw):
    """(low, all predictions) as fp32 numpy; through the spies what CorrBlock.__init__ received and what
    lookup_conv1x1_relu received and returned."""
    import eraft_amd.corr as corr
    net = _net(z, **kw).eval()
    im1, im2 = _inputs(z)
    init, conv = corr.CorrBlock.__init__, corr.CorrBlock.lookup_conv1x1_relu

    def spy_init(self, fmap1, fmap2, *a, **k):
        build_spy.append((fmap1.dtype, fmap2.dtype, k.get("fmap_dtype", "absent")))
        return init(self, fmap1, fmap2, *a, **k)

    def spy_conv(self, coords, weight, bias=None, *a, **k):
        out = conv(self, coords, weight, bias, *a, **k)
        conv_spy.append((k.get("out_dtype", "absent"), out.dtype, weight.dtype))
        return out
    corr.CorrBlock.__init__, corr.CorrBlock.lookup_conv1x1_relu = spy_init, spy_conv
    try:
        with torch.no_grad():
            low, ups = net(im1, im2, iters=ITERS)
    finally:
        corr.CorrBlock.__init__, corr.CorrBlock.lookup_conv1x1_relu = init, conv
    assert low.dtype == torch.float32 and all(u.dtype == torch.float32 for u in ups)
    assert bool(torch.isfinite(low).all()) and all(bool(torch.isfinite(u).all()) for u in ups)
    return low.cpu().numpy(), [u.cpu().numpy() for u in ups]


@pytest.fixture(scope="module", autouse=True)
def deterministic_convolutions():
    """MIOpen's deterministic algorithm choice for this module, restored afterwards (as
    tests/test_mixed_precision_gpu.py: the base arm is then bitwise reproducible, so the bound below is
    exact equality)."""
    if not torch.cuda.is_available():
        pytest.fail("no HIP device visible")
    saved = torch.backends.cudnn.deterministic
    torch.backends.cudnn.deterministic = True
    torch.backends.cuda.matmul.allow_tf32 = False
    torch.backends.cudnn.allow_tf32 = False
    yield
    torch.backends.cudnn.deterministic = saved


@pytest.mark.parametrize("dt", DTYPES, ids=["f16", "bf16"])
def test_half_at_both_ends_equals_the_cast_arm(dt):
    z = np.load(CASE)
    kw = dict(mixed_precision=True, amp_dtype=dt, fuse_motion_corr=True)
    ob, oc, bb, bc = [], [], [], []
    o_low, o_ups = _forward(z, ob, oc, **kw)
    b1_low, b1_ups = _forward(z, bb, bc, _native_half_lookup=False, **kw)
    b2_low, b2_ups = _forward(z, [], [], _native_half_lookup=False, **kw)
    # ours: amp_dtype fmaps with fmap_dtype=amp_dtype, amp_dtype out of the conv (fp32 weights)
    assert ob == [(dt, dt, dt)], ob
    assert len(oc) == ITERS and all(s == (dt, dt, torch.float32) for s in oc), oc
    # base: fp32 fmaps and no new keyword at all, fp32 out of the conv
    assert bb == [(torch.float32, torch.float32, "absent")], bb
    assert len(bc) == ITERS and all(s == ("absent", torch.float32, torch.float32) for s in bc), bc
    rows = []
    for what, o, b1, b2 in (("low", o_low, b1_low, b2_low), ("up", o_ups[-1], b1_ups[-1], b2_ups[-1]),
                            ("first up", o_ups[0], b1_ups[0], b2_ups[0])):
        e_ob, e_bb = epe(o, b1), epe(b1, b2)
        rows.append((what, e_ob, e_bb))
        print(f"{dt} {what}: epe(ours, base1) {e_ob:.3g} px, epe(base1, base2) {e_bb:.3g} px "
              f"(|flow| mean {np.abs(b1).mean():.3g} px)")
    for what, e_ob, e_bb in rows:
        assert e_ob <= 2 * e_bb, f"{what}: ours vs base {e_ob} px, base run to run {e_bb} px"


def test_plain_network_passes_no_new_keyword():
    """Without mixed_precision nothing changes: fp32 fmaps, neither keyword passed."""
    z = np.load(CASE)
    b, c = [], []
    _forward(z, b, c, fuse_motion_corr=True)
    assert b == [(torch.float32, torch.float32, "absent")], b
    assert len(c) == ITERS and all(s == ("absent", torch.float32, torch.float32) for s in c), c


def test_trains_through_16bit_fmaps_and_convc1():
    """bf16 autocast + train_motion_corr (16-bit fmaps saved by the build, 16-bit convc1 output, fp32
    backward) + the HIP upsampling: finite, non-zero fnet and convc1 gradients."""
    z = np.load(CASE)
    net = _net(z, mixed_precision=True, amp_dtype=torch.bfloat16, train_motion_corr=True, hip_upsample=True).train()
    im1, im2 = _inputs(z)
    low, ups = net(im1, im2, iters=2)
    assert low.dtype == torch.float32 and all(u.dtype == torch.float32 for u in ups)
    loss = sum(u.abs().mean() for u in ups)
    assert bool(torch.isfinite(loss))
    loss.backward()
    grads = [p.grad for p in net.fnet.parameters() if p.requires_grad]
    assert grads and all(g is not None for g in grads)
    assert all(bool(torch.isfinite(g).all()) for g in grads)
    assert float(net.fnet.conv1.weight.grad.abs().max()) > 0, "no gradient reached fnet's first convolution"
    c1 = net.update_block.encoder.convc1
    for g in (c1.weight.grad, c1.bias.grad):
        assert g is not None and bool(torch.isfinite(g).all()) and float(g.abs().max()) > 0
