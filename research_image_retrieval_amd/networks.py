"""networks-style extractors (reference: src/benchmark/networks/) on librr.

Every object here exposes the reference's extractor contract
(networks/RetrievalNet.py:327-344): ``.outputdim`` and
``.forward_test(x: float32 [B,3,H,W]) -> float32 [B,outputdim]`` L2-normalised,
eval-mode semantics, no autograd.  All arithmetic runs in librr's gfx950
kernels; torch only allocates device buffers.  There is no CPU path: calling
forward_test on a CPU tensor raises.
"""
import numpy as np
import torch

from . import ops
from . import weights as W

EPS_L2 = 1e-12  # F.normalize default eps (networks/RetrievalNet.py:343)


def _check_conv_math(conv_math):
    if conv_math not in ("h2", "f32"):
        raise ValueError("conv_math must be 'h2' or 'f32'")


class _BottleneckTrunk:
    """What the bottleneck trunks (ResNet, SENet) share: the folded convs, the
    stem, forward() and maps(), the one walk over the block schedule
    (self.blocks = weights.trunk_blocks).  A subclass supplies _block(x, xa, b,
    rec, hook, ci): block b on x (record xa) -> its output, rec the block's
    three zeroed records (conv1's output, conv2's, the block's) on the f16x2
    core and None on "f32", hook(ci), hook(ci + 1), hook(ci + 2) called after
    its three convs."""

    outputdim_block5 = 2048
    outputdim_block4 = 1024

    def _load_trunk_convs(self, sd, arch, device, conv_math, stride_on="3x3"):
        """The torchvision-keyed convs of sd (arch: a weights.RESNET_LAYERS
        name) with their BNs folded, on the device in self.convs, the stem
        padded to 4 input channels; on the f16x2 core the split weights in
        self.convs_h2."""
        self.device = torch.device(device)
        self.stride_on = stride_on
        self.blocks = W.trunk_blocks(arch, stride_on)
        folded = W.folded_resnet(sd, arch)
        # stem weights padded to 4 input channels (zero) for the NHWC4 tap path
        w1, b1 = folded["conv1"]
        folded["conv1"] = (torch.nn.functional.pad(w1, (0, 1)).contiguous(), b1)
        self.convs = {k: (w.to(self.device), b.to(self.device)) for k, (w, b) in folded.items()}
        self.layers = W.RESNET_LAYERS[arch]
        self.conv_math = conv_math
        self.convs_h2 = {}
        if conv_math == "h2":
            self.convs_h2 = {k: ops.H2Conv(w) for k, (w, _) in self.convs.items()}
            # the stem conv + ReLU + max-pool as one launch (ops.stem_pool_h2)
            self.fuse_stem_pool = True

    def _stem_h2(self, x, rec):
        """The f16x2 stem: x's record into rec[0], then the stem conv, its ReLU
        and the max-pool (one launch where self.fuse_stem_pool and the stem has
        64 channels, so the stem's full-resolution map never reaches HBM), the
        output's record in rec[1]: the max-pool output reuses the stem's (every
        stem output lies in some 3x3/2 window, so the max is the same)."""
        cv, h2 = self.convs, self.convs_h2
        ops.amax_f32(x, rec[0])
        if self.fuse_stem_pool and h2["conv1"].cout == 64:
            return ops.stem_pool_h2(x, rec[0], h2["conv1"], cv["conv1"][1], 2, 3, rec[1])
        x = ops.conv2d_h2(x, rec[0], h2["conv1"], cv["conv1"][1], 2, 3, None, True, rec[1])
        return ops.maxpool2d(x, 3, 2, 1)

    def _conv(self, x, xa, name, stride, pad, relu, residual=None, ya=None):
        """One folded conv on the trunk's core (xa / ya: the input's and the
        output's max-|x| record, read by the f16x2 core alone)."""
        w, b = self.convs[name]
        if self.conv_math == "h2":
            return ops.conv2d_h2(x, xa, self.convs_h2[name], b, stride, pad, residual, relu, ya)
        return ops.conv2d(x, w, b, stride, pad, residual, relu)

    def maps(self, x, hook=None, want_x3=False, **block_kw):
        """x: NHWC fp32 with 3 channels or 4 (zero 4th channel, preferred) ->
        (x3, x4, x3_amax, x4_amax), the order _Extractor._tail and
        ops.TrunkPlan.forward_u8(return_x3=True) use: layer3's and layer4's
        outputs (ResNet_DOLG.forward's (x3, x4), networks/backbone.py:236-242)
        and their max-|x| records, the ones x3's and x4's last launch
        published, for a caller that runs another f16x2 conv on either map.
        The records are None on the "f32" trunk; x3 and its record are None
        unless want_x3, so a caller that never reads x3 does not keep it alive.

        On the f16x2 core every conv reads its input's max-|x| record and
        writes its output's (one zeroed [2 + 3 blocks, 64] tensor per forward,
        block k's three at [2 + 3 k, 5 + 3 k)), and hook(i), if given, is
        called after the i-th conv launch (i = 0: the stem and its pool; a
        downsample projection launched by itself is not counted) -- the point
        where a caller can record a stream event.  The "f32" trunk never calls
        it.  block_kw: passed on to the subclass's _block."""
        if x.shape[-1] == 3:
            x = torch.nn.functional.pad(x, (0, 1))
        x = x.contiguous()
        h2 = self.conv_math == "h2"
        hook = (hook if h2 else None) or _no_hook
        rec = xa = x3 = x3a = None
        if h2:
            rec = ops.amax_records(2 + 3 * len(self.blocks), x.device)
            x = self._stem_h2(x, rec)
            hook(0)
            xa = rec[1]
        else:
            x = ops.maxpool2d(self._conv(x, None, "conv1", 2, 3, True), 3, 2, 1)
        for k, b in enumerate(self.blocks):
            r = rec[2 + 3 * k:5 + 3 * k] if h2 else None
            x = self._block(x, xa, b, r, hook, 1 + 3 * k, **block_kw)
            if h2:
                xa = r[2]
            if b.stage == 2 and b.stage_end:
                x3, x3a = x, xa
        return (x3, x, x3a, xa) if want_x3 else (None, x, None, xa)

    def forward(self, x, return_x3=False, hook=None, return_x3_amax=False, return_amax=False):
        """A selection from maps(x, hook, return_x3): x4; with return_x3 (x3,
        x4); return_x3_amax (f16x2 trunk, with return_x3) appends x3's max-|x|
        record; return_amax (f16x2 trunk) appends x4's, last: (x4, record) or
        (x3, x4, [x3's record,] record)."""
        if (return_x3_amax or return_amax) and self.conv_math != "h2":
            raise ValueError("return_x3_amax / return_amax: only the f16x2 trunk (conv_math='h2') keeps max-|x| "
                             "records")
        x3, x4, x3a, x4a = self.maps(x, hook, return_x3)
        ret = (x3, x4) if return_x3 else (x4,)
        if return_x3 and return_x3_amax:
            ret += (x3a,)
        if return_amax:
            ret += (x4a,)
        return ret if len(ret) > 1 else x4

    __call__ = forward


def _no_hook(i):
    pass


class ResNet(_BottleneckTrunk):
    """torchvision resnet children[:-2] trunk (networks/backbone.py:60-109:
    block1 = conv1/bn1/relu/maxpool, block2..5 = layer1..4), NHWC, BN folded.

    forward(x_nhwc [B,H,W,3]) -> [B,H/32,W/32,2048] NHWC.

    conv_math: "h2" (default) runs every conv, the stem included (NHWC4
    taps, K padded to 224), on the f16x2 split core (fp32-accurate: per conv
    mean error vs float64 within 1.05x and max within 1.25x of the exact-fp32
    core's, descriptors within 2x and <= 1e-6, tests/test_gpu_h2.py; three
    fp16 MFMAs per product; weights split once here, each conv publishes max
    |y| for the next one's split scale); "f32" keeps all convs on the
    exact-fp32 MFMA core.  (The split-bf16 core, "s3", was retired in round 6.)
    On "h2" a stage's first block runs conv3 and its downsample projection as
    one GEMM (ops.bottleneck_out_h2, where fuse_downsample is set and conv3's
    Cout is a multiple of 256), so the projected identity never reaches HBM.

    stride_on: "3x3" (default) = torchvision v1.5 bottlenecks; "1x1" = the
    reference's own torchvision-free R101, ResNet_DOLG
    (networks/backbone.py:218-274, BottleneckTransform :305-325: the stride of
    a stage's first block sits on the 1x1 `a` conv).  A ResNet_DOLG state dict
    (stem.*, s{K}.b{M}.*) is accepted as is (weights.to_torchvision_keys)."""

    def __init__(self, name="resnet101", state_dict=None, seed=0, device="cuda", conv_math="h2", stride_on="3x3"):
        _check_conv_math(conv_math)
        W.block_strides(1, stride_on)  # validates
        if name not in W.RESNET_LAYERS:
            raise ValueError(f"Unsupported or unknown architecture: {name}!")
        self.name = name
        sd = W.synthetic_resnet_state_dict(name, seed) if state_dict is None else W.to_torchvision_keys(state_dict)
        self._load_trunk_convs(sd, name, device, conv_math, stride_on)
        if conv_math == "h2":
            # each stage's first block: conv3 + downsample as one GEMM (ops.H2Bottleneck)
            self.fuse_downsample = True
            self.bneck_h2 = {}
            for b in self.blocks:
                if b.entry and b.cout % 256 == 0:
                    (w3, b3), (wd, bd) = self.convs[b.prefix + ".conv3"], self.convs[b.prefix + ".downsample.0"]
                    self.bneck_h2[b.prefix] = ops.H2Bottleneck(w3, b3, wd, bd)

    def _fused_entry(self, b):
        """Block b runs conv3 + its downsample projection as one GEMM (read per call: tests flip the flag)."""
        return b.entry and self.conv_math == "h2" and bool(self.fuse_downsample) and b.prefix in self.bneck_h2

    def _block(self, x, xa, b, rec, hook, ci):
        p, fused = b.prefix, self._fused_entry(b)
        r0, r1, r2 = rec if rec is not None else (None, None, None)
        idn = self._conv(x, xa, p + ".downsample.0", b.stride, 0, False) if b.entry and not fused else x
        y = self._conv(x, xa, p + ".conv1", b.s1, 0, True, None, r0)
        hook(ci)
        y = self._conv(y, r0, p + ".conv2", b.s2, 1, True, None, r1)
        hook(ci + 1)
        if fused:
            x = ops.bottleneck_out_h2(y, r1, x, xa, self.bneck_h2[p], b.stride, r2)
        else:
            x = self._conv(y, r1, p + ".conv3", 1, 0, True, idn, r2)
        hook(ci + 2)
        return x

    def plan_convs(self):
        """The f16x2 trunk's convs in the order the native plan (ops.TrunkPlan,
        rr_trunk_h2_create) takes them, under the current fuse_downsample:
        (convs, fuse_entry), fuse_entry per stage, convs the stem, then per
        block the downsample projection where it is a launch of its own,
        conv1, conv2, and conv3 or the fused [W3 | Wd].  A conv is
        rr_trunk_conv_t's fields with tensors for pointers: (planes, iscale,
        bias, cin, cout, kh, kw, stride, pad, residual, relu)."""
        def conv(name, stride, pad, residual, relu):
            c = self.convs_h2[name]
            return (c.planes, c.iscale, self.convs[name][1], c.cin, c.cout, c.kh, c.kw, stride, pad, residual, relu)

        convs, fuse_entry = [conv("conv1", 2, 3, False, True)], []
        for b in self.blocks:
            p, fused = b.prefix, self._fused_entry(b)
            if b.entry:
                fuse_entry.append(fused)
                if not fused:
                    convs.append(conv(p + ".downsample.0", b.stride, 0, False, False))
            convs.append(conv(p + ".conv1", b.s1, 0, False, True))
            convs.append(conv(p + ".conv2", b.s2, 1, False, True))
            if fused:
                e = self.bneck_h2[p]
                convs.append((e.planes2, e.iscale, e.bias, e.planes + e.cin, e.cout, 1, 1, b.stride, 0, False, True))
            else:
                convs.append(conv(p + ".conv3", 1, 0, True, True))
        return convs, fuse_entry

    def plan(self, lag=1):
        """The f16x2 trunk as a native plan (ops.TrunkPlan, built on first use,
        one per lag): uint8 pixels -> x4 (x3) and their records in one call, the
        same launches as maps() under the current fuse_downsample /
        fuse_stem_pool."""
        plans = self.__dict__.setdefault("_plans", {})
        key = (lag, bool(self.fuse_downsample), bool(self.fuse_stem_pool))
        if key not in plans:
            plans[key] = ops.TrunkPlan(self, lag)
        return plans[key]


class SENet(_BottleneckTrunk):
    """The SE-ResNet trunk of models/senet_g2.py:32-129 (SEBottleneck, SENet),
    NHWC, BN folded: torchvision-v1.5 bottlenecks (the stride on the 3x3, :41)
    whose conv3 + bn3 output is gated per channel by a Squeeze-and-Excitation
    block (:12-29) before the identity is added.  name: "senet50" = (3, 4, 6,
    3) or "senet101" = (3, 4, 23, 3); reduction: the SE blocks' (default 16).

    maps() is the trunks' shared walk, with taps: a dict that receives {block
    prefix: {mean, hidden, gate}} (tests).  Launches per block: conv1, conv2,
    conv3 WITHOUT residual, ReLU or record (a stage's first block: its
    downsample projection as a separate conv before them; no fused conv3 +
    downsample GEMM, whose epilogue cannot gate one half of its sum), then
    ops.se_squeeze, ops.linear_splitk (fc.0 + ReLU) and ops.se_apply in place
    on conv3's output (fc.2, the sigmoid, the scale, the identity, the ReLU),
    which on the f16x2 core publishes the block's max-|x| record for the next
    block's convs.  There is no plan(): the native trunk plan has no SE
    launches.

    state_dict: conv / BN keys as ResNet accepts them, plus
    layerN.M.se.fc.{0,2}.weight (weights.senet_se_from_state_dict); None: the
    seeded weights.synthetic_senet_state_dict."""

    def __init__(self, name="senet50", state_dict=None, seed=0, device="cuda", conv_math="h2", reduction=16):
        _check_conv_math(conv_math)
        if name not in W.SENET_TRUNKS:
            raise ValueError(f"Unsupported backbone: {name}")
        self.name = name
        self.reduction = W.senet_check_reduction(reduction)
        sd = W.synthetic_senet_state_dict(name, seed, reduction) if state_dict is None else state_dict
        se = W.senet_se_from_state_dict(sd, name, reduction)
        self._load_trunk_convs(W.to_torchvision_keys(sd), W.SENET_TRUNKS[name], device, conv_math)
        self.se = {p: (w1.to(self.device), w2.to(self.device)) for p, (w1, w2) in se.items()}

    def block(self, x, xa, p, entry, stride, rec=None, hook=None, ci=0, taps=None):
        """SEBottleneck.forward (:51-72) for block p on x (record xa): entry =
        the block has a downsample projection, stride = the 3x3's.  rec: three
        zeroed records (conv1's output, conv2's, the block's) on the f16x2
        core, None on "f32".  taps: a dict that receives mean, hidden and gate
        (tests).  Returns the block's output; its record is rec[2]."""
        r0, r1, r2 = rec if rec is not None else (None, None, None)
        hook = hook or _no_hook
        idn = self._conv(x, xa, f"{p}.downsample.0", stride, 0, False) if entry else x
        y = self._conv(x, xa, f"{p}.conv1", 1, 0, True, None, r0)
        hook(ci)
        y = self._conv(y, r0, f"{p}.conv2", stride, 1, True, None, r1)
        hook(ci + 1)
        y = self._conv(y, r1, f"{p}.conv3", 1, 0, False)
        hook(ci + 2)
        w1, w2 = self.se[p]
        mean = ops.se_squeeze(y)
        hidden = ops.linear_splitk(mean, w1, None, act=1)
        got = ops.se_apply(y, hidden, w2, idn, relu=True, want_gate=taps is not None, out=y, out_amax=r2)
        if taps is not None:
            taps.update(mean=mean, hidden=hidden, gate=got[1])
            return got[0]
        return got

    def _block(self, x, xa, b, rec, hook, ci, taps=None):
        return self.block(x, xa, b.prefix, b.entry, b.stride, rec, hook, ci,
                          None if taps is None else taps.setdefault(b.prefix, {}))


class gem:
    """GeM pooling with python-float p (networks/RetrievalNet.py:318-325)."""

    def __init__(self, p=3.0, eps=1e-6):
        self.p = float(p)
        self.eps = float(eps)

    def __call__(self, x_nhwc):
        return ops.gem_pool(x_nhwc, self.p, self.eps)


class HeadConv:
    """A head's stride-1 conv on the core its trunk runs on.  w: [Cout,KH,KW,
    Cin] on the device; conv_math "h2": the f16x2 core (the weights split once
    here), "f32": rr_conv2d."""

    def __init__(self, w, conv_math):
        _check_conv_math(conv_math)
        self.w = w
        self.h2 = ops.H2Conv(w) if conv_math == "h2" else None

    def __call__(self, x, x_amax, bias, pad=0, relu=False, residual=None, y_amax=None):
        """x_amax: x's max-|x| record, passed on as given (ops.amax_of for a
        caller that has none); y_amax (optional, zeroed) gets max |y|.  The
        "f32" core reads neither."""
        if self.h2 is not None:
            return ops.conv2d_h2(x, x_amax, self.h2, bias, 1, pad, residual, relu, y_amax)
        return ops.conv2d(x, self.w, bias, 1, pad, residual, relu)


class _Extractor:
    def eval(self):
        return self

    def train(self, mode=False):
        if mode:
            raise NotImplementedError("training is out of scope (SURVEY.md §2: row 13)")
        return self

    def to(self, *_a, **_k):
        return self

    in_channels = 3  # NHWC channel count the first layer consumes (4 = RGB + zero pad)

    def _input(self, x):
        if not isinstance(x, torch.Tensor) or not x.is_cuda:
            raise ValueError("forward_test expects a float32 [B,3,H,W] tensor on a ROCm device")
        x = x.float() if x.dtype != torch.float32 else x
        return ops.nchw_to_nhwc(x.contiguous(), out_c=self.in_channels)

    # A ResNet-based extractor names its trunk and what follows it, so that
    # forward_test_nhwc can run them in turn and forward_test_u8 can run the
    # trunk as the native plan (ResNet.plan): _trunk() -> the networks.ResNet
    # (None: no such trunk), _needs_x3: the tail reads layer3's output,
    # _tail(x3, x4, x3_amax, x4_amax) -> descriptors.
    _needs_x3 = False

    def _trunk(self):
        return None

    def _tail(self, x3, x4, x3_amax, x4_amax):
        raise NotImplementedError

    def forward_test_nhwc(self, x_nhwc, hook=None):
        """hook: the trunk's maps()'s (forward_test_u8_streams records its gate there)."""
        t = self._trunk()
        if t is None:
            raise NotImplementedError
        return self._tail(*t.maps(x_nhwc, hook, self._needs_x3))

    @torch.no_grad()
    def forward_test(self, x):
        return self.forward_test_nhwc(self._input(x))

    @torch.no_grad()
    def forward_test_u8(self, img_nhwc_u8):
        """uint8 [B,H,W,3] pixels -> descriptors, with ToTensor+Normalize fused
        into the first kernel (dataset/configdataset.py:417).  A ResNet-based
        extractor on the f16x2 core runs its trunk as one native call
        (ops.TrunkPlan: the launches of ResNet.maps, in two parts on two
        streams where the batch is large enough) and its tail on the current
        stream after the plan's join."""
        x = img_nhwc_u8
        t = self._trunk()
        if t is not None and t.conv_math == "h2":
            if self._needs_x3:
                return self._tail(*t.plan().forward_u8(x, return_x3=True))
            x4, x4a = t.plan().forward_u8(x)
            return self._tail(None, x4, None, x4a)
        return self.forward_test_nhwc(ops.preprocess_u8(x, out_c=self.in_channels))

    @torch.no_grad()
    def forward_test_u8_streams(self, img_nhwc_u8, streams, lag=1):
        """forward_test_u8 with the batch cut into len(streams) contiguous parts,
        part i on HIP stream streams[i], part i + 1 held back until part i has
        launched its lag-th conv (ResNet.maps' hook; lag 0 = after the
        stem).  The parts' kernels then run side by side, offset by about one
        layer, so an MFMA-bound conv of one part shares the chip with an
        HBM-bound conv of the other instead of every layer holding the chip by
        itself.  (Giving each stream's persistent kernels half the CUs, so
        that two kernels always co-run, measured slower: 68.5 vs 66.5 ms per
        1280-image embed, DESIGN.md.)  Each part is exactly
        forward_test_u8 of its images (its own
        max-|x| records for the f16x2 split scales): descriptors are
        bit-identical to running the parts one after another
        (tests/test_gpu_overlap.py) and within the split core's bar of the
        whole batch in one part.  Returns [B, outputdim] on the current stream."""
        x = img_nhwc_u8
        dev = x.device
        cur = torch.cuda.current_stream(dev)
        n = len(streams)
        b = x.shape[0]
        cuts = [b * i // n for i in range(n + 1)]
        outs, gate = [], None
        for i, s in enumerate(streams):
            if cuts[i] == cuts[i + 1]:
                continue
            s.wait_stream(cur)
            if gate is not None:
                s.wait_event(gate)
            ev = torch.cuda.Event()

            def hook(ci, ev=ev, s=s):
                if ci == lag:
                    ev.record(s)

            with torch.cuda.stream(s):
                f = self.forward_test_nhwc(ops.preprocess_u8(x[cuts[i]:cuts[i + 1]], out_c=self.in_channels),
                                           hook=hook)
            outs.append(f)
            gate = ev
        if not outs:
            return self.forward_test_u8(x)
        for s in streams:
            cur.wait_stream(s)
        for f in outs:
            f.record_stream(cur)
        return torch.cat(outs)


class GeM(_Extractor):
    """GeM network (networks/RetrievalNet.py:327-344): backbone -> gem(p=3) ->
    whiten 1x1 conv (outputdim -> 2048, +bias) -> F.normalize.

    As in the reference, the whitening conv takes ``outputdim`` input channels,
    so the network is only well-formed for outputdim == 2048 (:332)."""

    in_channels = 4

    def __init__(self, outputdim=2048, backbone="resnet101", state_dict=None, whiten=None, seed=0, device="cuda",
                 conv_math="h2"):
        if outputdim != 2048:
            raise ValueError("networks.GeM requires outputdim == 2048 (whiten is Conv2d(outputdim, 2048), "
                             "networks/RetrievalNet.py:332)")
        self.device = torch.device(device)
        self.backbone = ResNet(backbone, state_dict, seed, device, conv_math)
        self.pooling = gem()
        if whiten is None:
            ww, wb = W.synthetic_linear(2048, outputdim, seed + 1)
        else:
            ww, wb = whiten
            ww = ww.reshape(ww.shape[0], -1)
        self.whiten_w = ww.float().contiguous().to(self.device)
        self.whiten_b = wb.float().contiguous().to(self.device)
        self.outputdim = outputdim

    def _trunk(self):
        return self.backbone

    def _tail(self, x3, x4, x3_amax, x4_amax):
        f = self.pooling(x4)
        f = ops.linear(f, self.whiten_w, self.whiten_b)
        return ops.l2_normalize(f, EPS_L2, out=f)


class DOLG(_Extractor):
    """DOLG (networks/RetrievalNet.py:367-431, forward_test; local branch
    SpatialAttention2d :433-474): trunk (f3, f4) -> local branch on f3 (1x1
    conv1 + BN, channel-normalised map weighted by softplus(conv2(relu)))
    and global branch fc_t(gem_3(f4)) -> the local map's component orthogonal
    to the global vector, average-pooled -> fc(cat) -> F.normalize.

    The projection is linear in the local map, so fo = m - fg (fg . m) /
    (fg . fg) with m the local map's spatial mean: rr_dolg_local_pool reads
    the conv1+BN map once and writes m, rr_dolg_orth_fuse builds [fg | fo];
    the local map and its projection are never stored ("DOLG").

    Constructor as the reference's (pretrained, with_aspp, backbone) plus
    state_dict (trunk keys as networks.ResNet accepts, head keys as
    weights.dolg_head_from_state_dict), seed (synthetic weights when
    state_dict is None), device, conv_math and stride_on ("3x3" = the
    reference's torchvision trunk, ResNet_STAGE45; "1x1" for a ResNet_DOLG /
    MSRA-layout checkpoint).  with_aspp=True (dilated 3x3 convs) and
    pretrained downloads are not supported."""

    in_channels = 4

    def __init__(self, pretrained=None, with_aspp=False, backbone="resnet101", state_dict=None, seed=0,
                 device="cuda", conv_math="h2", stride_on="3x3"):
        if with_aspp:
            raise ValueError("networks.DOLG: with_aspp=True is not supported (ASPP needs dilated 3x3 convs)")
        if pretrained is not None:
            raise ValueError("networks.DOLG: pretrained weights cannot be downloaded; pass state_dict")
        self.device = torch.device(device)
        head = W.dolg_head_from_state_dict(W.synthetic_dolg_head(seed + 1) if state_dict is None else state_dict)
        self.globalmodel = ResNet(backbone, state_dict, seed, device, conv_math, stride_on)
        cin = self.globalmodel.outputdim_block4
        if tuple(head["conv1_w"].shape[1:]) != (1, 1, cin) or head["fc_t_w"].shape[1] != ResNet.outputdim_block5 or \
                head["fc_t_w"].shape[0] != head["conv1_w"].shape[0] or head["fc_w"].shape[1] != 2 * head["conv1_w"].shape[0]:
            raise ValueError("networks.DOLG: head weight shapes do not fit the trunk")
        self.conv_math = conv_math
        self.pool_g = gem(3.0)
        self.conv1 = HeadConv(head["conv1_w"].to(self.device), conv_math)
        self.conv1_b = head["conv1_b"].to(self.device)
        self.conv2_w = head["conv2_w"].to(self.device)
        self.conv2_b = head["conv2_b"]
        self.fc_t = (head["fc_t_w"].to(self.device), head["fc_t_b"].to(self.device))
        self.fc = (head["fc_w"].to(self.device), head["fc_b"].to(self.device))
        self.outputdim = head["fc_w"].shape[0]
        self.meta = {"outputdim": self.outputdim}

    def local_mean(self, x3, x3_amax=None):
        """m [B,1024]: the spatial mean of SpatialAttention2d's output on x3."""
        return ops.dolg_local_pool(self.conv1(x3, x3_amax, self.conv1_b), self.conv2_w, self.conv2_b)

    _needs_x3 = True

    def _trunk(self):
        return self.globalmodel

    def _tail(self, x3, x4, x3_amax, x4_amax):
        return self.head(x3, x4, x3_amax)

    def head(self, x3, x4, x3_amax=None):
        """Everything after the trunk: (x3, x4) NHWC -> descriptors [B,512]."""
        m = self.local_mean(x3, x3_amax)
        fg = ops.linear(self.pool_g(x4), *self.fc_t)
        f = ops.linear(ops.dolg_orth_fuse(fg, m), *self.fc)
        return ops.l2_normalize(f, EPS_L2, out=f)


class SOABlock_GeM:
    """SOLAR's pooling stage (networks/RetrievalNet.py:534-569): second-order
    attention over the map's positions, the 1x1 conv v, the residual, gem(p=3).
    Callable on x4 NHWC [B,H,W,in_ch] -> pooled [B,in_ch].

    Four launches: the f, g and h 1x1 convs as ONE conv (Cout = 3 in_ch / k,
    BN folded, no ReLU), rr_soa_attention (applies f's and g's ReLU on load,
    online softmax, the scores never stored), the v conv with x4 as its
    residual epilogue, rr_gem_pool.  head: weights.solar_head_from_state_dict's
    dict (fgh_w, fgh_b, v_w, v_b).  conv_math "h2" runs both convs on the f16x2
    core: x4's max-|x| record is the trunk's (x4_amax; computed here when the
    caller has none), the attention output's comes from ops.amax_f32."""

    def __init__(self, in_ch, k, head, device="cuda", conv_math="h2"):
        _check_conv_math(conv_math)
        self.in_ch, self.out_ch, self.mid_ch = in_ch, in_ch, in_ch // k
        if tuple(head["fgh_w"].shape) != (3 * self.mid_ch, 1, 1, in_ch) or \
                tuple(head["v_w"].shape) != (in_ch, 1, 1, self.mid_ch):
            raise ValueError("networks.SOABlock_GeM: head weight shapes do not fit in_ch and k")
        self.device = torch.device(device)
        self.conv_math = conv_math
        self.fgh = HeadConv(head["fgh_w"].to(self.device), conv_math)
        self.v = HeadConv(head["v_w"].to(self.device), conv_math)
        self.fgh_b, self.v_b = head["fgh_b"].to(self.device), head["v_b"].to(self.device)
        self.pooling = gem(3.0)

    def attended(self, x4, x4_amax=None):
        """z = v(softmax(c^-0.5 f^T g) h^T) + x4, NHWC (:558-567)."""
        h2 = self.conv_math == "h2"
        if h2 and x4_amax is None:
            x4_amax = ops.amax_of(x4)
        a = ops.soa_attention(self.fgh(x4, x4_amax, self.fgh_b), self.mid_ch)
        return self.v(a, ops.amax_of(a) if h2 else None, self.v_b, residual=x4)

    def __call__(self, x4, x4_amax=None):
        return self.pooling(self.attended(x4, x4_amax))


class SOLAR(_Extractor):
    """SOLAR (networks/RetrievalNet.py:572-590, forward_test): backbone ->
    SOABlock_GeM(2048, k=2) -> F.normalize -> whiten (1x1 conv 2048 -> 2048,
    +bias) -> F.normalize.

    Constructor: the reference's positional order (outputdim, classifier_num,
    s, m, backbone) first; classifier_num, s and m belong to the ArcFace
    training head and are accepted and ignored.  Then state_dict (trunk keys
    as networks.ResNet accepts, head keys as weights.solar_head_from_state_dict),
    seed (synthetic weights when state_dict is None), device, conv_math and
    stride_on as networks.DOLG.  whiten always emits 2048 values (:577), so
    outputdim must be 2048."""

    in_channels = 4

    def __init__(self, outputdim=2048, classifier_num=None, s=32, m=0.15, backbone="resnet101", state_dict=None,
                 seed=0, device="cuda", conv_math="h2", stride_on="3x3"):
        if outputdim != 2048:
            raise ValueError("networks.SOLAR requires outputdim == 2048 (whiten is Conv2d(2048, 2048), "
                             "networks/RetrievalNet.py:577)")
        self.device = torch.device(device)
        head = W.solar_head_from_state_dict(W.synthetic_solar_head(seed + 1) if state_dict is None else state_dict)
        self.backbone = ResNet(backbone, state_dict, seed, device, conv_math, stride_on)
        cin = self.backbone.outputdim_block5
        if head["whiten_w"].shape != (2048, cin):
            raise ValueError("networks.SOLAR: whiten weight shape does not fit the trunk")
        self.conv_math = conv_math
        self.pooling = SOABlock_GeM(cin, 2, head, device, conv_math)
        self.whiten_w = head["whiten_w"].to(self.device)
        self.whiten_b = head["whiten_b"].to(self.device)
        self.outputdim = outputdim
        self.meta = {"outputdim": outputdim}

    def _trunk(self):
        return self.backbone

    def _tail(self, x3, x4, x3_amax, x4_amax):
        return self.tail(self.pooling(x4, x4_amax))

    def tail(self, pooled):
        """:587-590: F.normalize -> whiten -> F.normalize on the pooled [B,2048]."""
        f = ops.linear(ops.l2_normalize(pooled, EPS_L2), self.whiten_w, self.whiten_b)
        return ops.l2_normalize(f, EPS_L2, out=f)


class Token_Refine:
    """The Token head (networks/RetrievalNet.py:164-187, with Attention :94-126,
    Encoder :129-142, Decoder :145-161, Mlp :75-91), eval mode.  Callable on x4
    NHWC [B,H,W,2048] -> [B,1024] (before forward_test's F.normalize).

    head: weights.token_head_from_state_dict's dict.  The constructor keeps the
    reference's (num_heads, num_object, mid_dim, encoder_layer, decoder_layer);
    the kernels are built for heads of 128, one encoder and two decoders.

    Launches, N = H W positions, 4 = num_object tokens per image:
      per position (1x1 convs; conv_math "h2": the f16x2 core, each conv reading
      its input's max-|x| record and publishing its output's; "f32": rr_conv2d):
        conv + BN                 2048 -> 1024
        encoder q | k | v         1024 -> 3072, one GEMM
        rr_attention_hd128        nq = nk = N, column slices of the stacked rows
        (h2: rr_amax_f32 of the attention output)
        proj + X                  residual in the epilogue
        mlp(BN) + X               the BatchNorm1d folded into the weights
        decoder k1 | v1 | k2 | v2 1024 -> 4096, one GEMM for both decoders
      rr_token_pool               softmax over the objects, A X, one read of X
      per token (4 rows per image; rr_linear_ex / rr_layernorm always):
        token_norm: linear, LayerNorm
        per decoder: LayerNorm, q linear, rr_attention_hd128 (nq = 4, nk = N),
          proj + T; fc1, rr_gelu in place, fc2 + T; LayerNorm, q | k | v linear,
          rr_attention_hd128 (nq = nk = 4), proj + T
      proj + BatchNorm1d          [B,4096] -> [B,1024]
    No torch arithmetic: torch allocates buffers and takes views."""

    def __init__(self, num_heads=8, num_object=4, mid_dim=1024, encoder_layer=1, decoder_layer=2, head=None,
                 device="cuda", conv_math="h2"):
        _check_conv_math(conv_math)
        if mid_dim != 128 * num_heads:
            raise ValueError("networks.Token_Refine: mid_dim must be 128 * num_heads (rr_attention_hd128)")
        if encoder_layer != 1 or decoder_layer != 2:
            raise ValueError("networks.Token_Refine: one encoder layer and two decoder layers")
        if head is None:
            raise ValueError("networks.Token_Refine needs head=weights.token_head_from_state_dict(...)")
        if tuple(head["query"].shape) != (num_object, mid_dim) or head["conv_w"].shape[0] != mid_dim or \
                tuple(head["out_w"].shape) != (1024, num_object * mid_dim):
            raise ValueError("networks.Token_Refine: head weight shapes do not fit num_object and mid_dim")
        self.heads, self.n_obj, self.mid_dim = num_heads, num_object, mid_dim
        self.device = torch.device(device)
        self.conv_math = conv_math
        self.w = {k: v.to(self.device) for k, v in head.items()}
        self.convs = {k: HeadConv(self.w[k + "_w"], conv_math)
                      for k in ("conv", "enc_qkv", "enc_proj", "enc_mlp", "dec_kv")}

    def _conv(self, x, xa, name, residual=None, ya=None):
        return self.convs[name](x, xa, self.w[name + "_b"], residual=residual, y_amax=ya)

    def _lin(self, x, name, residual=None):
        return ops.linear_ex(x, self.w[name + "_w"], self.w[name + "_b"], residual)

    def __call__(self, x4, x4_amax=None, taps=None):
        """x4 NHWC -> [B,1024].  x4_amax: x4's max-|x| record (f16x2 trunk).
        taps: a dict that receives the intermediates X (encoder output), T0
        (pooled tokens), tn, dec0, dec1 (tests)."""
        w, m, nh, no = self.w, self.mid_dim, self.heads, self.n_obj
        b, hh, ww, _ = x4.shape
        n = hh * ww
        h2 = self.conv_math == "h2"
        rec = ops.amax_records(5, x4.device) if h2 else [None] * 5
        if h2 and x4_amax is None:
            x4_amax = ops.amax_f32(x4, rec[4])
        x = self._conv(x4, x4_amax, "conv", None, rec[0])
        qkv = self._conv(x, rec[0], "enc_qkv").view(b * n, 3 * m)
        a = ops.attention_hd128(qkv[:, :m], qkv[:, m:2 * m], qkv[:, 2 * m:], b, n, n, nh).view(b, hh, ww, m)
        if h2:
            ops.amax_f32(a, rec[1])
        x = self._conv(a, rec[1], "enc_proj", x, rec[2])
        x = self._conv(x, rec[2], "enc_mlp", x, rec[3])
        kv = self._conv(x, rec[3], "dec_kv").view(b * n, 4 * m)
        t0 = ops.token_pool(x, w["query"])
        t = ops.layernorm(self._lin(t0.view(b * no, m), "tn"), w["tn_g"], w["tn_beta"])
        if taps is not None:
            taps.update(X=x.view(b, n, m), T0=t0, tn=t.view(b, no, m))
        for i in (0, 1):
            p = f"d{i}_"
            q = self._lin(ops.layernorm(t, w[p + "ln1_g"], w[p + "ln1_b"]), p + "cq")
            ca = ops.attention_hd128(q, kv[:, 2 * i * m:(2 * i + 1) * m], kv[:, (2 * i + 1) * m:(2 * i + 2) * m], b, no,
                                     n, nh)
            t = self._lin(ca, p + "cproj", t)
            hdn = self._lin(t, p + "fc1")
            t = self._lin(ops.gelu(hdn, out=hdn), p + "fc2", t)
            sq = self._lin(ops.layernorm(t, w[p + "ln2_g"], w[p + "ln2_b"]), p + "sqkv")
            sa = ops.attention_hd128(sq[:, :m], sq[:, m:2 * m], sq[:, 2 * m:], b, no, no, nh)
            t = self._lin(sa, p + "sproj", t)
            if taps is not None:
                taps[f"dec{i}"] = t.view(b, no, m)
        return self._lin(t.view(b, no * m), "out")


class Token(_Extractor):
    """Token (networks/RetrievalNet.py:290-305, forward_test): backbone ->
    Token_Refine(8 heads, 4 object tokens, mid_dim 1024, 1 encoder, 2 decoders)
    -> F.normalize, 1024 values per image.  The network spca_train.py and the
    training drivers construct.

    Constructor: the reference's positional order (outputdim, classifier_num,
    pretrained, backbone) first; classifier_num belongs to the ArcFace training
    head and is accepted and ignored; pretrained weights cannot be downloaded,
    so pretrained must stay None.  Then state_dict (trunk keys as
    networks.ResNet accepts, head keys as weights.token_head_from_state_dict),
    seed (synthetic weights when state_dict is None), device, conv_math and
    stride_on as networks.SOLAR.  outputdim must be 1024 (mid_dim and the
    width tr.proj emits)."""

    in_channels = 4

    def __init__(self, outputdim=1024, classifier_num=81313, pretrained=None, backbone="resnet101", state_dict=None,
                 seed=0, device="cuda", conv_math="h2", stride_on="3x3"):
        if outputdim != 1024:
            raise ValueError("networks.Token requires outputdim == 1024 (Token_Refine's proj emits 1024 values, "
                             "networks/RetrievalNet.py:173)")
        if pretrained is not None:
            raise ValueError("networks.Token: pretrained weights cannot be downloaded; pass state_dict")
        self.device = torch.device(device)
        head = W.token_head_from_state_dict(W.synthetic_token_head(seed + 1) if state_dict is None else state_dict)
        self.backbone = ResNet(backbone, state_dict, seed, device, conv_math, stride_on)
        if head["conv_w"].shape[-1] != self.backbone.outputdim_block5:
            raise ValueError("networks.Token: tr.conv does not fit the trunk")
        self.conv_math = conv_math
        self.tr = Token_Refine(8, head["query"].shape[0], outputdim, 1, 2, head, device, conv_math)
        self.outputdim = outputdim
        self.meta = {"outputdim": outputdim}

    def _trunk(self):
        return self.backbone

    def _tail(self, x3, x4, x3_amax, x4_amax):
        return self.tail(self.tr(x4, x4_amax))

    def tail(self, f):
        """:304: F.normalize on the head's [B,1024]."""
        return ops.l2_normalize(f, EPS_L2, out=f)


class RetrievalNet(Token):
    """RetrievalNet (networks/RetrievalNet.py:263-278): the same backbone, the
    same Token_Refine head and the same forward_test as Token, with the
    reference's (classifier_num) signature (its ArcFace_Delg classifier is
    training-only and ignored).  The keyword arguments are Token's."""

    def __init__(self, classifier_num=None, **kw):
        super().__init__(1024, classifier_num, None, "resnet101", **kw)


class ConvDimReduction:
    """PCA-whitening as a frozen 1x1 conv (networks/spca.py:205-227):
    weight = P[:dim], bias = -(P m)[:dim]."""

    def __init__(self, input_dim, dim, device="cuda"):
        self.input_dim, self.dim = input_dim, dim
        self.device = torch.device(device)
        self.weight = None
        self.bias = None

    def initialize_pca_whitening(self, des):
        """Fit (m, P) on descriptors des [N, input_dim] (numpy), exactly as
        pcawhitenlearn_shrinkage (networks/backbone.py:42-58) + spca.py:215-227."""
        m, P = pcawhitenlearn_shrinkage(des, device=self.device)
        m, P = m.T, P.T
        self.weight = torch.tensor(P[: self.dim, :], dtype=torch.float32).contiguous().to(self.device)
        shift = -torch.mm(torch.tensor(P, dtype=torch.float32), torch.tensor(m, dtype=torch.float32)).squeeze()
        self.bias = shift[: self.dim].contiguous().to(self.device)
        return m.T, P.T

    def set_params(self, weight, bias):
        self.weight = weight.reshape(weight.shape[0], -1).float().contiguous().to(self.device)
        self.bias = bias.float().contiguous().to(self.device)

    def __call__(self, x):
        if self.weight is None:
            raise RuntimeError("ConvDimReduction: call initialize_pca_whitening or set_params first")
        return ops.linear(x, self.weight, self.bias)


def pcawhitenlearn_shrinkage(X, s=1.0, device="cuda"):
    """PCA whitening with shrinkage (networks/backbone.py:42-58).

    The O(n d^2) part — column mean and centred Gram Xc^T Xc — runs on the GPU
    (rr_pcaw_gram: fp32 MFMA over 8192-row slices, fp64 sums).  The d x d tail
    stays on the host exactly as the reference writes it: symmetrise / 2n,
    LAPACK geev (np.linalg.eig, so eigenvector signs follow the reference's
    solver), descending eigenvalue order, projection scaled by lambda^(-s/2),
    in X's floating dtype.  Returns (mean [1,D], P^T [D,D])."""
    if isinstance(X, torch.Tensor):
        dt = np.float64 if X.dtype == torch.float64 else np.float32
    else:
        X = np.asarray(X)
        dt = X.dtype if X.dtype in (np.float32, np.float64) else np.float32
    x = torch.as_tensor(X).to(device=device, dtype=torch.float32).contiguous()
    n = x.shape[0]
    mean64, gram = ops.pcaw_gram(x)
    gram = gram.cpu().numpy()
    cov = ((gram + gram.T) / (2 * n)).astype(dt)
    lam, vec = np.linalg.eig(cov)
    desc = np.argsort(lam)[::-1]
    lam, vec = lam[desc], vec[:, desc]
    # np.power, not `**`: numpy turns `x ** 0.5` into sqrt, 1 ulp off pow
    proj = np.linalg.inv(np.diag(np.power(lam, 0.5 * s))) @ vec.T
    return mean64.cpu().numpy()[None, :].astype(dt), proj.T


class GeMPCAw(_Extractor):
    """Config C3 extractor: networks.GeM (R101, 2048-d) -> PCA-whitening
    (ConvDimReduction) -> L2.  The reference has no caller wiring the two
    (SURVEY.md §3.4); this is the cirtorch-style composition normalise ->
    whiten -> normalise."""

    def __init__(self, net, pcaw):
        self.in_channels = net.in_channels
        self.net = net
        self.pcaw = pcaw
        self.outputdim = pcaw.dim
        self._needs_x3 = net._needs_x3

    def _trunk(self):
        return self.net._trunk()

    def _whiten(self, f):
        f = self.pcaw(f)
        return ops.l2_normalize(f, EPS_L2, out=f)

    def _tail(self, x3, x4, x3_amax, x4_amax):
        return self._whiten(self.net._tail(x3, x4, x3_amax, x4_amax))

    def forward_test_nhwc(self, x_nhwc, hook=None):
        return self._whiten(self.net.forward_test_nhwc(x_nhwc, hook=hook))


class VisionTransformer(_Extractor):
    """CLIP-style ViT image tower (networks/model.py:206-243) on librr.

    forward(x) returns ``ln_post(x[:, 0]) @ proj`` as the reference does;
    forward_test(x) additionally L2-normalises (the extractor contract).
    Weights: a CLIP-layout state dict (conv1.weight, class_embedding,
    positional_embedding, ln_pre.*, transformer.resblocks.{i}.{attn.in_proj_*,
    attn.out_proj.*, ln_1.*, mlp.c_fc.*, mlp.c_proj.*, ln_2.*}, ln_post.*,
    proj).  LayerNorm eps 1e-5 (nn.LayerNorm default)."""

    def __init__(self, input_resolution=224, patch_size=16, width=768, layers=12, heads=12, output_dim=512,
                 state_dict=None, device="cuda", dtype="fp32"):
        if width % heads or width // heads != 64:
            raise ValueError("VisionTransformer: librr's fused attention needs head_dim == 64")
        if state_dict is None:
            raise ValueError("VisionTransformer needs a state_dict (no pretrained download offline)")
        self.device = torch.device(device)
        self.res, self.patch, self.width, self.layers, self.heads = input_resolution, patch_size, width, layers, heads
        self.output_dim = self.outputdim = output_dim
        self.seq = (input_resolution // patch_size) ** 2 + 1
        if self.seq > 256:
            raise ValueError("VisionTransformer: sequence longer than 256 tokens")
        t = lambda k: state_dict[k].float().contiguous().to(self.device)  # noqa: E731
        # patch conv [width, 3, p, p] -> [width][p][p][3] to match patchify's (kh, kw, c) rows
        self.conv_w = state_dict["conv1.weight"].float().permute(0, 2, 3, 1).reshape(width, -1).contiguous().to(
            self.device)
        self.cls = t("class_embedding")
        self.pos = t("positional_embedding")
        self.ln_pre = (t("ln_pre.weight"), t("ln_pre.bias"))
        self.blocks = []
        for i in range(layers):
            p = f"transformer.resblocks.{i}."
            self.blocks.append({k: t(p + k) for k in (
                "attn.in_proj_weight", "attn.in_proj_bias", "attn.out_proj.weight", "attn.out_proj.bias",
                "ln_1.weight", "ln_1.bias", "mlp.c_fc.weight", "mlp.c_fc.bias", "mlp.c_proj.weight",
                "mlp.c_proj.bias", "ln_2.weight", "ln_2.bias")})
        self.ln_post = (t("ln_post.weight"), t("ln_post.bias"))
        self.proj_t = state_dict["proj"].float().t().contiguous().to(self.device)  # [out, width]
        if dtype not in ("fp32", "bf16"):
            raise ValueError("VisionTransformer dtype must be fp32 or bf16")
        self.dtype = dtype
        if dtype == "bf16":
            # config C4: bf16 GEMM operands (weights rounded once, RNE), fp32
            # accumulate, fp32 residual stream / LayerNorm / softmax
            self.conv_w_bf = self.conv_w.to(torch.bfloat16)
            for blk in self.blocks:
                for k in ("attn.in_proj_weight", "attn.out_proj.weight", "mlp.c_fc.weight", "mlp.c_proj.weight"):
                    blk[k + ".bf16"] = blk[k].to(torch.bfloat16)
                # ln_1 / ln_2 folded into the in-proj / c_fc GEMMs (rr_linear_bf16_ln)
                if not ops.ln_fold_supported(width, dtype):
                    continue
                blk["qkv.fold"] = ops.ln_fold_weights(blk["attn.in_proj_weight"], blk["attn.in_proj_bias"],
                                                      blk["ln_1.weight"], blk["ln_1.bias"])
                blk["fc.fold"] = ops.ln_fold_weights(blk["mlp.c_fc.weight"], blk["mlp.c_fc.bias"],
                                                     blk["ln_2.weight"], blk["ln_2.bias"])
        # the LayerNorm fold needs 256-column residual rows and K <= 768 (a
        # wider model, e.g. ViT-L/14's 1024, which networks/model.py:405
        # builds, runs the LayerNorm passes)
        self.ln_fold = ops.ln_fold_supported(width, dtype)

    def _forward_bf16(self, x_nhwc, b):
        # patch rows straight to bf16; ln_pre fused into the token assembly
        p = ops.patchify(x_nhwc, self.patch, out_bf16=True)
        x = ops.vit_tokens(ops.linear_bf16(p, self.conv_w_bf), b, self.cls, self.pos, ln=self.ln_pre)
        if self.ln_fold:
            # ln_1 / ln_2 (:188-190) folded into the in-proj / c_fc GEMMs: the
            # residual GEMMs' epilogues write the bf16 rows and the row
            # statistics, so no LayerNorm pass re-reads the fp32 stream
            xb, st = ops.ln_partials_bf16(x)
            for li, blk in enumerate(self.blocks):
                qkv = ops.linear_bf16_ln_fold(xb, st, *blk["qkv.fold"])
                a = ops.attention_bf16(qkv, b, self.seq, self.heads)
                x, xb, st = ops.linear_bf16_ln_produce(a, blk["attn.out_proj.weight.bf16"], blk["attn.out_proj.bias"], x)
                y = ops.linear_bf16_ln_fold(xb, st, *blk["fc.fold"], act=2)
                if li + 1 < len(self.blocks):
                    x, xb, st = ops.linear_bf16_ln_produce(y, blk["mlp.c_proj.weight.bf16"], blk["mlp.c_proj.bias"], x)
                else:
                    # the last block's output feeds only ln_post (fp32 CLS rows):
                    # no bf16 copy or partials (they would be ~390 MB per
                    # 1280-image step that nothing reads)
                    x = ops.linear_bf16(y, blk["mlp.c_proj.weight.bf16"], blk["mlp.c_proj.bias"], residual=x)
            cls = ops.layernorm(x, *self.ln_post, rows=b, row_stride=self.seq * self.width)
            return ops.linear(cls, self.proj_t)
        for blk in self.blocks:
            y = ops.layernorm_bf16(x, blk["ln_1.weight"], blk["ln_1.bias"])
            # QKV rows in bf16 (RNE, exactly as the attention rounds fp32 rows): half the bytes
            qkv = ops.linear_bf16(y, blk["attn.in_proj_weight.bf16"], blk["attn.in_proj_bias"], out_bf16=True)
            a = ops.attention_bf16(qkv, b, self.seq, self.heads)
            x = ops.linear_bf16(a, blk["attn.out_proj.weight.bf16"], blk["attn.out_proj.bias"], residual=x)
            y = ops.layernorm_bf16(x, blk["ln_2.weight"], blk["ln_2.bias"])
            y = ops.linear_bf16(y, blk["mlp.c_fc.weight.bf16"], blk["mlp.c_fc.bias"], act=2, out_bf16=True)
            x = ops.linear_bf16(y, blk["mlp.c_proj.weight.bf16"], blk["mlp.c_proj.bias"], residual=x)
        cls = ops.layernorm(x, *self.ln_post, rows=b, row_stride=self.seq * self.width)
        return ops.linear(cls, self.proj_t)

    def forward_nhwc(self, x_nhwc):
        b, h, w, _ = x_nhwc.shape
        if self.dtype == "bf16" and h == self.res and w == self.res:
            return self._forward_bf16(x_nhwc, b)
        if h != self.res or w != self.res:
            raise ValueError(f"VisionTransformer: fixed {self.res}x{self.res} input (positional embedding has "
                             f"{self.seq} tokens; networks/model.py:228)")
        x = ops.linear(ops.patchify(x_nhwc, self.patch), self.conv_w)
        x = ops.vit_tokens(x, b, self.cls, self.pos, ln=self.ln_pre)
        for blk in self.blocks:
            y = ops.layernorm(x, blk["ln_1.weight"], blk["ln_1.bias"])
            qkv = ops.linear(y, blk["attn.in_proj_weight"], blk["attn.in_proj_bias"])
            a = ops.attention(qkv, b, self.seq, self.heads)
            x = ops.linear_ex(a, blk["attn.out_proj.weight"], blk["attn.out_proj.bias"], residual=x)
            y = ops.layernorm(x, blk["ln_2.weight"], blk["ln_2.bias"])
            y = ops.linear_ex(y, blk["mlp.c_fc.weight"], blk["mlp.c_fc.bias"], act=2)
            x = ops.linear_ex(y, blk["mlp.c_proj.weight"], blk["mlp.c_proj.bias"], residual=x)
        cls = ops.layernorm(x, *self.ln_post, rows=b, row_stride=self.seq * self.width)
        return ops.linear(cls, self.proj_t)

    @torch.no_grad()
    def forward(self, x):
        return self.forward_nhwc(self._input(x))

    __call__ = forward

    def forward_test_nhwc(self, x_nhwc):
        f = self.forward_nhwc(x_nhwc)
        return ops.l2_normalize(f, EPS_L2, out=f)
