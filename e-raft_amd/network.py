"""ERAFT counterpart on top of the HIP CorrBlock -- the caller of the hot path, plain PyTorch-ROCm.

This is the end-to-end parity harness SURVEY §2 row 3 asks for: the same network as
/root/reference/model/eraft.py + extractor.py + update.py (identical state_dict keys, so the
reference's checkpoints and our PRNG test weights load unchanged), with the correlation hot path
served by eraft_amd.CorrBlock (libecorr.so) and the coordinate grids by eraft_amd.coords_grid.
Everything that is not CorrBlock stays ordinary PyTorch (MIOpen convolutions), as the north star
requires; the arithmetic of each layer follows the reference expression for expression so that
the only numerical differences come from the backends.

Reference map:
    ERAFT.forward            eraft.py:88-145       ERAFT.upsample_flow   eraft.py:74-85
    ImagePadder              image_utils.py:83-123 BasicEncoder          extractor.py:119-189
    ResidualBlock            extractor.py:7-57     BasicUpdateBlock      update.py:84-106
    BasicMotionEncoder       update.py:63-81       SepConvGRU            update.py:33-60
    FlowHead                 update.py:6-14
"""
import contextlib

import torch
import torch.nn as nn
import torch.nn.functional as F

from .alt_corr import AlternateCorrBlock
from .corr import CorrBlock
from .flow import upsample_flow as hip_upsample_flow
from .gru import sepconv_gru, sepconv_gru_train
from .motion_enc import motion_encoder, motion_encoder_train
from .utils import coords_grid


def _norm(kind, ch):
    if kind == "batch":
        return nn.BatchNorm2d(ch)
    if kind == "instance":
        return nn.InstanceNorm2d(ch)
    if kind == "group":
        return nn.GroupNorm(num_groups=ch // 8, num_channels=ch)
    return nn.Sequential()


class ResidualBlock(nn.Module):
    """conv-norm-relu x2 with a strided 1x1 projection shortcut (extractor.py:7-57).  norm3 is
    registered both directly and inside `downsample`, like the reference, so both key sets exist."""

    def __init__(self, cin, cout, norm_fn="group", stride=1):
        super().__init__()
        self.conv1 = nn.Conv2d(cin, cout, 3, padding=1, stride=stride)
        self.conv2 = nn.Conv2d(cout, cout, 3, padding=1)
        self.relu = nn.ReLU(inplace=True)
        self.norm1 = _norm(norm_fn, cout)
        self.norm2 = _norm(norm_fn, cout)
        if stride != 1:
            self.norm3 = _norm(norm_fn, cout)
            self.downsample = nn.Sequential(nn.Conv2d(cin, cout, 1, stride=stride), self.norm3)
        else:
            self.downsample = None

    def forward(self, x):
        y = self.relu(self.norm1(self.conv1(x)))
        y = self.relu(self.norm2(self.conv2(y)))
        skip = x if self.downsample is None else self.downsample(x)
        return self.relu(skip + y)


class BasicEncoder(nn.Module):
    """1/8-resolution feature / context encoder (extractor.py:119-189)."""

    def __init__(self, output_dim=128, norm_fn="batch", dropout=0.0, n_first_channels=1):
        super().__init__()
        self.norm_fn = norm_fn
        self.norm1 = _norm(norm_fn, 64)
        self.conv1 = nn.Conv2d(n_first_channels, 64, 7, stride=2, padding=3)
        self.relu1 = nn.ReLU(inplace=True)
        widths, cin, layers = (64, 96, 128), 64, []
        for i, wdt in enumerate(widths):
            stride = 1 if i == 0 else 2
            layers.append(nn.Sequential(ResidualBlock(cin, wdt, norm_fn, stride),
                                        ResidualBlock(wdt, wdt, norm_fn, 1)))
            cin = wdt
        self.layer1, self.layer2, self.layer3 = layers
        self.conv2 = nn.Conv2d(128, output_dim, 1)
        self.dropout = nn.Dropout2d(p=dropout) if dropout > 0 else None

    def forward(self, x):
        pair = isinstance(x, (list, tuple))
        if pair:
            n = x[0].shape[0]
            x = torch.cat(x, dim=0)
        x = self.relu1(self.norm1(self.conv1(x)))
        x = self.conv2(self.layer3(self.layer2(self.layer1(x))))
        if self.training and self.dropout is not None:
            x = self.dropout(x)
        return torch.split(x, [n, n], dim=0) if pair else x


class BasicMotionEncoder(nn.Module):
    """Consumes the 324-channel lookup output (update.py:63-81)."""

    def __init__(self, corr_levels=4, corr_radius=4):
        super().__init__()
        planes = corr_levels * (2 * corr_radius + 1) ** 2
        self.convc1 = nn.Conv2d(planes, 256, 1, padding=0)
        self.convc2 = nn.Conv2d(256, 192, 3, padding=1)
        self.convf1 = nn.Conv2d(2, 128, 7, padding=3)
        self.convf2 = nn.Conv2d(128, 64, 3, padding=1)
        self.conv = nn.Conv2d(64 + 192, 128 - 2, 3, padding=1)

    def forward(self, flow, corr, corr_is_convc1=False):
        # corr_is_convc1: `corr` already is F.relu(convc1(corr)) -- the fused CorrBlock path
        c = F.relu(self.convc2(corr if corr_is_convc1 else F.relu(self.convc1(corr))))
        f = F.relu(self.convf2(F.relu(self.convf1(flow))))
        out = F.relu(self.conv(torch.cat([c, f], dim=1)))
        return torch.cat([out, flow], dim=1)


class SepConvGRU(nn.Module):
    """Separable ConvGRU: a 1x5 half-step then a 5x1 half-step (update.py:33-60)."""

    def __init__(self, hidden_dim=128, input_dim=192 + 128):
        super().__init__()
        cin = hidden_dim + input_dim
        for tag, k, p in (("1", (1, 5), (0, 2)), ("2", (5, 1), (2, 0))):
            for gate in ("z", "r", "q"):
                setattr(self, f"conv{gate}{tag}", nn.Conv2d(cin, hidden_dim, k, padding=p))

    @staticmethod
    def _half(h, x, cz, cr, cq):
        hx = torch.cat([h, x], dim=1)
        z = torch.sigmoid(cz(hx))
        r = torch.sigmoid(cr(hx))
        q = torch.tanh(cq(torch.cat([r * h, x], dim=1)))
        return (1 - z) * h + z * q

    def forward(self, h, x):
        h = self._half(h, x, self.convz1, self.convr1, self.convq1)
        return self._half(h, x, self.convz2, self.convr2, self.convq2)


class FlowHead(nn.Module):
    def __init__(self, input_dim=128, hidden_dim=256):
        super().__init__()
        self.conv1 = nn.Conv2d(input_dim, hidden_dim, 3, padding=1)
        self.conv2 = nn.Conv2d(hidden_dim, 2, 3, padding=1)
        self.relu = nn.ReLU(inplace=True)

    def forward(self, x):
        return self.conv2(self.relu(self.conv1(x)))


class BasicUpdateBlock(nn.Module):
    def __init__(self, hidden_dim=128, corr_levels=4, corr_radius=4, hip_gru=False, train_gru=False):
        super().__init__()
        self.hip_gru = bool(hip_gru)   # the GRU as eraft_amd.sepconv_gru on self.gru's weights (same keys)
        self.train_gru = bool(train_gru)   # ... as eraft_amd.sepconv_gru_train: the same forward, with its HIP backward
        self.encoder = BasicMotionEncoder(corr_levels, corr_radius)
        self.gru = SepConvGRU(hidden_dim=hidden_dim, input_dim=128 + hidden_dim)
        self.flow_head = FlowHead(hidden_dim, hidden_dim=256)
        self.mask = nn.Sequential(nn.Conv2d(128, 256, 3, padding=1), nn.ReLU(inplace=True),
                                  nn.Conv2d(256, 64 * 9, 1, padding=0))

    def forward(self, net, inp, corr, flow, corr_is_convc1=False, x=None):
        # x: the GRU's input [inp, motion features] already assembled (ERAFT hip_motion_encoder=True: inp once,
        # eraft_amd.motion_encoder into its upper half every iteration); inp, corr and flow are then not read
        inp = torch.cat([inp, self.encoder(flow, corr, corr_is_convc1)], dim=1) if x is None else x
        if self.train_gru:
            net = sepconv_gru_train(net.contiguous(), inp, self.gru)
        else:
            net = sepconv_gru(net.contiguous(), inp, self.gru) if self.hip_gru else self.gru(net, inp)
        return net, 0.25 * self.mask(net), self.flow_head(net)


class ImagePadder:
    """Zero-pads top/left to a multiple of min_size and remembers it (image_utils.py:83-123)."""

    def __init__(self, min_size=64):
        self.min_size = min_size
        self.pad_height = None
        self.pad_width = None

    def pad(self, image):
        h, w = image.shape[-2:]
        ph = (self.min_size - h % self.min_size) % self.min_size
        pw = (self.min_size - w % self.min_size) % self.min_size
        if self.pad_width is None:
            self.pad_height, self.pad_width = ph, pw
        elif (ph, pw) != (self.pad_height, self.pad_width):
            raise RuntimeError("ImagePadder: image size changed between calls")
        return F.pad(image, (pw, 0, ph, 0))

    def unpad(self, image):
        return image[..., self.pad_height:, self.pad_width:]


class ERAFT(nn.Module):
    """E-RAFT with the MI355X CorrBlock (eraft.py:37-145).  config needs 'subtype' in
    {'standard', 'warm_start'}; n_first_channels = voxel bins.  fuse_motion_corr=True replaces
    `corr_fn(coords1)` + BasicMotionEncoder's `relu(convc1(corr))` with the HIP lookup + convc1
    (CorrBlock.lookup_conv1x1_relu; its ECORR_CONVC1 mode); hip_upsample=True runs upsample_flow as
    the one-pass HIP kernel (eraft_amd.upsample_flow), which is differentiable in
    flow and mask (its HIP backward), so a loss on the predictions trains through
    it.  differentiable_corr=True
    builds the CorrBlock with differentiable=True, so a loss on the predictions trains fnet (not with
    fuse_motion_corr).  With both, the native ops run on both ends of the GRU loop in training.
    train_motion_corr=True is fuse_motion_corr on a differentiable CorrBlock: every iteration runs
    CorrBlock.lookup_conv1x1_relu in the forward and its HIP backward, so fnet and
    convc1 train through it; under torch.no_grad() its predictions are bitwise fuse_motion_corr's.
    mixed_precision=True is the reference's mixed-precision path (eraft.py:101, 110-117, 131-132, which
    its get_args() switches off): fnet, cnet and the update block run under
    torch.autocast("cuda", dtype=amp_dtype) (torch.float16 or torch.bfloat16), coords and predictions
    stay fp32, and the CorrBlock is 16-bit at both ends: fnet's amp_dtype fmaps go to
    CorrBlock(..., fmap_dtype=amp_dtype) as they are (the split build reads them itself: bitwise the
    pyramid of their .float()), the lookup is asked for amp_dtype directly (corr_fn(coords1,
    out_dtype=amp_dtype): the kernel stores what autocast's cast in front of convc1 would produce, bit
    for bit), and with fuse_motion_corr / train_motion_corr lookup_conv1x1_relu(..., out_dtype=amp_dtype)
    stores what autocast's cast in front of convc2 would produce.  It composes with fuse_motion_corr,
    differentiable_corr and train_motion_corr; hip_upsample gets the mask as fp32.
    _native_half_lookup=False (private: the A/B arm of the tests, tools/bench_lookup_half.py and
    tools/bench_half_io.py) is the whole path without any of the three: the fmaps go back to fp32
    (.float()), the lookup and lookup_conv1x1_relu return fp32 and autocast casts them.
    alternate_corr=True (keyword only) serves the lookups from AlternateCorrBlock (alt_corr.py, DESIGN.md
    §3.10): no all-pairs volume is built, memory grows with H W instead of (H W)^2 and each lookup costs
    more time.  It composes with mixed_precision (16-bit fmaps in, 16-bit lookup out) and hip_upsample; it
    is forward-only and has no fused convc1, so fuse_motion_corr, train_motion_corr and
    differentiable_corr raise ValueError with it.
    train_alternate_corr=True (keyword only; named after train_motion_corr) is alternate_corr on a trainable
    AlternateCorrBlock (trainable=True; csrc/alt_grad.hip): a loss on the predictions trains
    fnet through the volume-free lookup's HIP backward, without a pyramid or a gradient pyramid.  It implies
    alternate_corr=True, combines with mixed_precision and hip_upsample as alternate_corr does, and raises
    ValueError with fuse_motion_corr, train_motion_corr or differentiable_corr.
    hip_gru=True (keyword only) runs the update block's SepConvGRU as eraft_amd.sepconv_gru (csrc/gru.hip,
    DESIGN.md §3.11) on the same parameters (the state_dict keys are unchanged): fp32 and forward-only.  It
    composes with fuse_motion_corr, hip_upsample and alternate_corr, and raises ValueError with
    mixed_precision, differentiable_corr, train_motion_corr or train_alternate_corr.
    train_gru=True (keyword only) runs it as eraft_amd.sepconv_gru_train instead: the same forward launches (under
    torch.no_grad() the predictions are bitwise hip_gru=True's) with the HIP backward of csrc/gru_grad.hip
    (DESIGN.md §3.11.1), so a loss on the predictions trains the GRU's twelve parameters and everything in
    front of it through native kernels.  It composes with differentiable_corr, train_motion_corr,
    train_alternate_corr, fuse_motion_corr, hip_upsample and alternate_corr; hip_gru=True may be passed along and
    changes nothing (its own refusals apply only without train_gru).  The kernels are fp32:
    train_gru=True with mixed_precision=True raises ValueError.
    hip_motion_encoder=True (keyword only) runs what BasicMotionEncoder does behind convc1 -- convc2, convf1, convf2,
    conv and both concatenations -- as eraft_amd.motion_encoder (csrc/motion_enc.hip) on the same
    parameters (the state_dict keys are unchanged): the GRU's input x [B, 256, H/8, W/8] is allocated once per
    forward with the context features in its lower half, and every iteration the kernels write the motion
    features into its upper half, so neither torch.cat runs.  relu(convc1(corr)) comes from
    CorrBlock.lookup_conv1x1_relu under fuse_motion_corr, else from the lookup and torch's convc1.  fp32 and
    forward-only: it composes with fuse_motion_corr, hip_upsample, hip_gru and alternate_corr, and raises ValueError
    with mixed_precision, differentiable_corr, train_motion_corr, train_alternate_corr or train_gru.
    train_motion_encoder=True (keyword only) runs it as eraft_amd.motion_encoder_train instead: the same forward
    launches (under torch.no_grad() the predictions are bitwise hip_motion_encoder=True's) with the HIP backward of
    csrc/motion_enc_grad.hip, so a loss on the predictions trains convc2, convf1, convf2 and conv
    and everything in front of them through native kernels.  Every iteration gets a fresh x = cat([inp, m]): writing
    into one reused x would overwrite what the GRU's node saved for its backward.  It composes with
    differentiable_corr, train_motion_corr, train_alternate_corr, train_gru, fuse_motion_corr, alternate_corr and
    hip_upsample; hip_motion_encoder=True may be passed along and changes nothing (its own refusals apply only
    without train_motion_encoder).  The kernels are fp32: train_motion_encoder=True with mixed_precision=True raises
    ValueError, and so does hip_gru=True without train_gru=True (a forward-only GRU behind a differentiable encoder).
    The defaults keep the reference's call pattern exactly."""

    corr_levels = 4
    corr_radius = 4

    def __init__(self, config, n_first_channels, fuse_motion_corr=False, hip_upsample=False,
                 differentiable_corr=False, train_motion_corr=False, mixed_precision=False,
                 amp_dtype=torch.float16, _native_half_lookup=True, *, alternate_corr=False,
                 train_alternate_corr=False, hip_gru=False, train_gru=False, hip_motion_encoder=False,
                 train_motion_encoder=False):
        super().__init__()
        if train_motion_encoder and mixed_precision:
            raise ValueError("train_motion_encoder=True cannot be combined with mixed_precision: the HIP motion "
                             "encoder and its backward are fp32")
        if train_motion_encoder and hip_gru and not train_gru:
            raise ValueError("train_motion_encoder=True cannot be combined with hip_gru=True unless train_gru=True: "
                             "the HIP SepConvGRU alone is forward-only, so no gradient would reach the encoder")
        self.train_motion_encoder = bool(train_motion_encoder)
        if hip_motion_encoder and not train_motion_encoder and (mixed_precision or differentiable_corr or
                                                                train_motion_corr or train_alternate_corr or train_gru):
            raise ValueError("hip_motion_encoder=True cannot be combined with mixed_precision, differentiable_corr, "
                             "train_motion_corr, train_alternate_corr or train_gru: the HIP motion encoder is fp32 "
                             "and forward-only")
        self.hip_motion_encoder = bool(hip_motion_encoder)
        if train_gru and mixed_precision:
            raise ValueError("train_gru=True cannot be combined with mixed_precision: the HIP SepConvGRU and its "
                             "backward are fp32")
        self.train_gru = bool(train_gru)
        if hip_gru and not train_gru and (mixed_precision or differentiable_corr or train_motion_corr or
                                          train_alternate_corr):
            raise ValueError("hip_gru=True cannot be combined with mixed_precision, differentiable_corr, "
                             "train_motion_corr or train_alternate_corr: the HIP SepConvGRU is fp32 and forward-only")
        self.hip_gru = bool(hip_gru)
        if train_alternate_corr and (fuse_motion_corr or train_motion_corr or differentiable_corr):
            raise ValueError("train_alternate_corr=True cannot be combined with fuse_motion_corr, train_motion_corr or "
                             "differentiable_corr: it trains through AlternateCorrBlock(trainable=True), which has no "
                             "volume, no gradient pyramid and no fused convc1")
        self.train_alternate_corr = bool(train_alternate_corr)
        alternate_corr = alternate_corr or self.train_alternate_corr
        if alternate_corr and (fuse_motion_corr or train_motion_corr or differentiable_corr):
            raise ValueError("alternate_corr=True cannot be combined with fuse_motion_corr, train_motion_corr or "
                             "differentiable_corr: AlternateCorrBlock is forward-only and has no fused convc1")
        self.alternate_corr = bool(alternate_corr)
        if amp_dtype not in (torch.float16, torch.bfloat16):
            raise TypeError(f"amp_dtype must be torch.float16 or torch.bfloat16 (got {amp_dtype!r})")
        self.mixed_precision = bool(mixed_precision)
        self.amp_dtype = amp_dtype
        self._native_half_lookup = bool(_native_half_lookup)
        if train_motion_corr:
            differentiable_corr = fuse_motion_corr = True
        elif differentiable_corr and fuse_motion_corr:
            raise ValueError("differentiable_corr=True cannot be combined with fuse_motion_corr=True: the fused "
                             "lookup + convc1 is forward-only")
        self.train_motion_corr = train_motion_corr
        self.differentiable_corr = differentiable_corr
        self.fuse_motion_corr = fuse_motion_corr
        self.hip_upsample = hip_upsample
        self.image_padder = ImagePadder(min_size=32)
        self.subtype = config["subtype"].lower()
        if self.subtype not in ("standard", "warm_start"):
            raise ValueError(f"unknown subtype {self.subtype}")
        self.hidden_dim = 128
        self.context_dim = 128
        self.fnet = BasicEncoder(output_dim=256, norm_fn="instance", dropout=0,
                                 n_first_channels=n_first_channels)
        self.cnet = BasicEncoder(output_dim=self.hidden_dim + self.context_dim, norm_fn="batch",
                                 dropout=0, n_first_channels=n_first_channels)
        self.update_block = BasicUpdateBlock(self.hidden_dim, self.corr_levels, self.corr_radius,
                                             hip_gru=self.hip_gru, train_gru=self.train_gru)

    def freeze_bn(self):
        """Keep every BatchNorm2d on its running statistics while the rest trains (eraft.py:60-63)."""
        for mod in self.modules():
            if isinstance(mod, nn.BatchNorm2d):
                mod.eval()

    def initialize_flow(self, img):
        N, _, H, W = img.shape
        c0 = coords_grid(N, H // 8, W // 8, device=img.device)
        c1 = coords_grid(N, H // 8, W // 8, device=img.device)
        return c0, c1

    @staticmethod
    def upsample_flow(flow, mask):
        """Convex 8x upsampling with a softmax over the 3x3 neighbourhood (eraft.py:74-85)."""
        N, _, H, W = flow.shape
        m = torch.softmax(mask.view(N, 1, 9, 8, 8, H, W), dim=2)
        nb = F.unfold(8 * flow, [3, 3], padding=1).view(N, 2, 9, 1, 1, H, W)
        up = torch.sum(m * nb, dim=2).permute(0, 1, 4, 2, 5, 3)
        return up.reshape(N, 2, 8 * H, 8 * W)

    def _autocast(self):
        """The reference's autocast(enabled=args.mixed_precision) (eraft.py:101, 110, 131); without
        mixed_precision no context at all, so the default path is the one it always was."""
        if not self.mixed_precision:
            return contextlib.nullcontext()
        return torch.autocast("cuda", dtype=self.amp_dtype)

    def forward(self, image1, image2, iters=12, flow_init=None, upsample=True):
        image1 = self.image_padder.pad(image1).contiguous()
        image2 = self.image_padder.pad(image2).contiguous()
        with self._autocast():
            fmap1, fmap2 = self.fnet([image1, image2])
        # mixed precision: the block reads fnet's amp_dtype fmaps itself and the lookup (or the fused
        # convc1) stores amp_dtype itself, what autocast would cast it to for convc1 (convc2)
        half_lookup = self.mixed_precision and self._native_half_lookup
        # differentiable_corr: gradients reach fnet through the HIP backward (corr.py); the keywords
        # are passed only on their paths, so a reference-signature CorrBlock can stand in otherwise
        kw = {"differentiable": True} if self.differentiable_corr else {}
        if self.train_alternate_corr:
            kw = {"trainable": True}
        block = AlternateCorrBlock if self.alternate_corr else CorrBlock   # the volume-free lookup, or the pyramid
        if half_lookup and fmap1.dtype == self.amp_dtype and fmap2.dtype == self.amp_dtype:
            corr_fn = block(fmap1.contiguous(), fmap2.contiguous(), num_levels=self.corr_levels,
                            radius=self.corr_radius, fmap_dtype=self.amp_dtype, **kw)
        else:
            corr_fn = block(fmap1.float().contiguous(), fmap2.float().contiguous(),
                            num_levels=self.corr_levels, radius=self.corr_radius, **kw)
        with self._autocast():
            net, inp = torch.split(self.cnet(image2), [self.hidden_dim, self.context_dim], dim=1)
            net, inp = torch.tanh(net), torch.relu(inp)
        coords0, coords1 = self.initialize_flow(image1)
        if flow_init is not None:
            coords1 = coords1 + flow_init
        predictions = []
        # the GRU's input, assembled in place: inp once, the motion features per iteration
        if self.hip_motion_encoder and not self.train_motion_encoder:
            x = torch.empty((inp.shape[0], self.context_dim + 128) + tuple(inp.shape[2:]), dtype=torch.float32,
                            device=inp.device)
            x[:, :self.context_dim].copy_(inp)
        for _ in range(iters):
            coords1 = coords1.detach()
            if self.hip_motion_encoder or self.train_motion_encoder:   # fp32, no autocast: mixed_precision is refused
                enc = self.update_block.encoder
                if self.fuse_motion_corr:
                    c1 = corr_fn.lookup_conv1x1_relu(coords1, enc.convc1.weight, enc.convc1.bias)
                else:
                    c1 = F.relu(enc.convc1(corr_fn(coords1)))
                if self.train_motion_encoder:   # a fresh x: the GRU's node keeps the previous iteration's
                    m = motion_encoder_train(coords1 - coords0, c1.contiguous(), enc)
                    x = torch.cat([inp, m], 1)
                else:
                    motion_encoder(coords1 - coords0, c1.contiguous(), enc, out=x[:, self.context_dim:])
                net, up_mask, delta = self.update_block(net, None, None, None, x=x)
            else:
                if self.fuse_motion_corr:
                    c1 = self.update_block.encoder.convc1
                    corr = corr_fn.lookup_conv1x1_relu(coords1, c1.weight, c1.bias,
                                                       **({"out_dtype": self.amp_dtype} if half_lookup else {}))
                elif half_lookup:
                    corr = corr_fn(coords1, out_dtype=self.amp_dtype)
                else:
                    corr = corr_fn(coords1)
                with self._autocast():
                    net, up_mask, delta = self.update_block(net, inp, corr, coords1 - coords0,
                                                            corr_is_convc1=self.fuse_motion_corr)
            coords1 = coords1 + delta
            if self.hip_upsample:   # the HIP kernel takes fp32 (autocast's mask is amp_dtype)
                up = hip_upsample_flow(coords1 - coords0, up_mask.float())
            else:
                up = self.upsample_flow(coords1 - coords0, up_mask)
            predictions.append(self.image_padder.unpad(up))
        return coords1 - coords0, predictions
