"""Table-1 style extractors and registry (reference: src/benchmark/models/).

Mirrors models/gem_pooling.py:12-143 and models/wrappers.py:18-90 for the GeM
family named by the hot path: ``get_model('gem_r50' | 'gem_r101', num_classes,
feature_dim=..., gem_p=...)`` returns a wrapper whose
``extract_global_descriptor(x)`` yields L2-normalised [B, feature_dim] fp32.
The HOW family (models/how_vlad.py:14-287) is served the same way:
``get_model('how_vlad_r50' | 'how_vlad_r101' | 'how_asmk_r50' | 'how_asmk_r101',
num_classes, local_dim=..., num_clusters=...)``, [B, 2048] descriptors.
SoSNet (models/sosnet.py:95-212) is built with ``get_sosnet_model(num_classes,
backbone=..., second_order_dim=...)`` or ``SoSNetWrapper``; its registry names
are NOT registered yet: ``get_model('sosnet_r50' | 'sosnet_r101', ...)`` still
raises NotImplementedError (the names stay in OUT_OF_SCOPE).
The token aggregator (models/token_based.py:13-212) likewise: ``get_token_model(
num_classes, backbone=..., hidden_dim=..., num_heads=..., num_layers=...)`` or
``TokenWrapper``, inputs up to 448 x 448 (196 positions); ``get_model('token_r50'
| 'token_r101', ...)`` still raises NotImplementedError.
SpoC (models/spoc.py:97-248) likewise: ``get_spoc_model(num_classes,
backbone=..., pyramid_levels=..., context_dim=..., use_context=...)`` or
``SpoCWrapper``; ``get_model('spoc_r50' | 'spoc_r101', ...)`` still raises
NotImplementedError.
SENet-G2+ (models/senet_g2.py:12-274), the one method on an SE-ResNet trunk
(networks.SENet), likewise: ``get_senet_g2_model(num_classes, backbone='senet50'
| 'senet101', reduction=..., gem_p=...)`` or ``SENetG2Wrapper``;
``get_model('senet_g2_50' | 'senet_g2_101', ...)`` still raises
NotImplementedError.
Training (``forward(x, targets)`` losses, optimizers) is out of scope
(SURVEY.md §2 row 13): ``forward`` only produces eval-mode logits.
"""
import torch

from . import ops
from . import weights as W
from .networks import ResNet, SENet, HeadConv, _Extractor, EPS_L2


class _TrunkHeadModel(_Extractor):
    """A Table-1 model: a networks.ResNet trunk in self.backbone and a head on
    the trunk's last map.  A subclass's __init__ calls, in this order,
    _check_backbone, its own argument checks, _load_head, its own head-shape
    checks and host-side reads, and _build, where the device work starts; it
    defines head(x4, x4_amax=None) -> features [B,outputdim].  self.w holds the
    head's tensors on the device under the loader's keys, cls_w and cls_b among
    them.  _Extractor._trunk() stays None: forward_test_u8 preprocesses and
    calls forward_test_nhwc, it does not run the trunk as the native plan."""

    in_channels = 4

    @staticmethod
    def _check_backbone(pretrained, backbone, cite):
        """cite: where the reference's constructor defaults to pretrained=True."""
        if pretrained:
            raise ValueError("pretrained weights need a download; pass a local state_dict instead "
                             f"({cite} defaults to pretrained=True)")
        if backbone not in ("resnet50", "resnet101"):
            raise ValueError(f"Unsupported backbone: {backbone}")

    @staticmethod
    def _load_head(state_dict, seed, from_sd, synthetic, *args):
        """from_sd of the state dict, or of synthetic(seed + 1, *args) when there is none."""
        return from_sd(synthetic(seed + 1, *args) if state_dict is None else state_dict)

    def _make_trunk(self, backbone, state_dict, seed, device, conv_math, stride_on):
        """The trunk _build puts in self.backbone: a networks.ResNet, unless a
        subclass builds another class with ResNet.maps' contract."""
        return ResNet(backbone, state_dict, seed, device, conv_math=conv_math, stride_on=stride_on)

    def _build(self, head, fit, backbone, state_dict, seed, device, conv_math, stride_on):
        """The trunk, then the head's tensors on its device.  fit: (key, the
        reference's name) of the head weight whose columns are the trunk's
        channels, or None."""
        self.device = torch.device(device)
        self.conv_math = conv_math
        self.backbone = self._make_trunk(backbone, state_dict, seed, device, conv_math, stride_on)
        if fit is not None and head[fit[0]].shape[1] != self.backbone.outputdim_block5:
            raise ValueError(f"{type(self).__name__}: {fit[1]} does not fit the trunk")
        self.w = {k: v.to(self.device) for k, v in head.items()}

    def trunk_map(self, x_nhwc, hook=None):
        """NHWC pixels -> (x4, x4's max-|x| record; None on the "f32" trunk)."""
        _, x4, _, x4_amax = self.backbone.maps(x_nhwc, hook)
        return x4, x4_amax

    def extract_features_nhwc(self, x_nhwc, hook=None):
        return self.head(*self.trunk_map(x_nhwc, hook))

    @torch.no_grad()
    def extract_features(self, x):
        return self.extract_features_nhwc(self._input(x))

    def forward_test_nhwc(self, x_nhwc, hook=None):
        f = self.extract_features_nhwc(x_nhwc, hook)
        return ops.l2_normalize(f, EPS_L2, out=f)

    @torch.no_grad()
    def extract_descriptor(self, x):
        return self.forward_test(x)

    @torch.no_grad()
    def forward(self, x, targets=None):
        feats = self.extract_features(x)
        return None, ops.linear(feats, self.w["cls_w"], self.w["cls_b"])

    def __call__(self, x, targets=None):
        return self.forward(x, targets)


class _Wrapper(_Extractor):
    """The reference's training-loop facade over a _TrunkHeadModel, kept in
    self.backbone as the reference's wrappers keep theirs."""

    in_channels = 4

    def __init__(self, model):
        self.backbone = model
        self.outputdim = model.outputdim

    def forward_test_nhwc(self, x_nhwc, hook=None):
        return self.backbone.forward_test_nhwc(x_nhwc, hook)

    @torch.no_grad()
    def forward(self, x, targets=None):
        return self.backbone(x)

    def __call__(self, x, targets=None):
        return self.forward(x, targets)

    def extract_features(self, x):
        return self.backbone.extract_features(x)

    def extract_descriptor(self, x):
        return self.backbone.extract_descriptor(x)

    @torch.no_grad()
    def extract_global_descriptor(self, x):
        return self.backbone.extract_descriptor(x)


class GeMPooling:
    """GeM with a tensor-valued p (models/gem_pooling.py:12-23).  The
    reference stores p as a 1-element Parameter; the exponent 1/p is formed
    in fp32 from it, which is what gem_pool's powf path does."""

    def __init__(self, p=3.0, eps=1e-6):
        self.p = torch.ones(1) * p
        self.eps = eps

    def __call__(self, x_nhwc):
        return ops.gem_pool(x_nhwc, float(self.p.item()), self.eps)


class GeMModel(_TrunkHeadModel):
    """resnet trunk -> GeMPooling -> feature_proj Linear(2048, feature_dim)
    (models/gem_pooling.py:26-92); extract_descriptor adds F.normalize(p=2, dim=1)."""

    def __init__(self, backbone="resnet50", pretrained=False, num_classes=1000, feature_dim=2048, gem_p=3.0,
                 state_dict=None, seed=0, device="cuda", conv_math="h2", stride_on="3x3"):
        self._check_backbone(pretrained, backbone, "models/gem_pooling.py:35")
        backbone_dim = 2048
        pw, pb = _from_sd(state_dict, "feature_proj") or W.synthetic_linear(feature_dim, backbone_dim, seed + 2)
        cw, cb = _from_sd(state_dict, "classifier") or W.synthetic_linear(num_classes, feature_dim, seed + 3)
        head = {k: v.float().contiguous() for k, v in (("proj_w", pw), ("proj_b", pb), ("cls_w", cw), ("cls_b", cb))}
        self._build(head, None, backbone, state_dict, seed, device, conv_math, stride_on)
        self.proj_w, self.proj_b, self.cls_w, self.cls_b = (self.w[k] for k in ("proj_w", "proj_b", "cls_w", "cls_b"))
        self.gem_pool = GeMPooling(p=gem_p)
        self.feature_dim = feature_dim
        self.outputdim = feature_dim

    def head(self, x4, x4_amax=None):
        return ops.linear(self.gem_pool(x4), self.proj_w, self.proj_b)


def _from_sd(sd, name):
    if sd is None:
        return None
    for pre in ("", "backbone.", "module.backbone."):
        k = f"{pre}{name}.weight"
        if k in sd:
            return sd[k], sd[f"{pre}{name}.bias"]
    return None


class GeMWrapper(_Wrapper):
    """models/gem_pooling.py:95-119: training-loop facade over GeMModel."""

    def __init__(self, num_classes, backbone="resnet50", feature_dim=2048, gem_p=3.0, **kw):
        super().__init__(GeMModel(backbone=backbone, num_classes=num_classes, feature_dim=feature_dim, gem_p=gem_p,
                                  **kw))


def get_gem_model(num_classes, backbone="resnet50", **kwargs):
    return GeMWrapper(num_classes=num_classes, backbone=backbone, **kwargs)


class HOWModel(_TrunkHeadModel):
    """models/how_vlad.py:107-199, eval mode: resnet trunk -> local_proj (1x1
    conv 2048 -> local_dim, +bias) -> F.normalize per position -> VLADPooling
    (alpha = 100) or ASMKPooling -> final_proj Linear(K D or K, 2048);
    extract_descriptor adds F.normalize.

    Launches after the trunk: the 1x1 conv (conv_math "h2": the f16x2 core on
    the trunk's max-|x| record; "f32": rr_conv2d), rr_how_vlad or rr_how_asmk on
    its RAW rows (the per-position normalisation, the distances, the assignment
    and the aggregation in one read), rr_l2_normalize over the pooled vector
    (:56, :102), rr_linear, rr_l2_normalize.

    Constructor: the reference's (backbone, pretrained, num_classes, local_dim,
    pooling_type, num_clusters), then state_dict (trunk keys as networks.ResNet
    accepts, the reference's index-named nn.Sequential keys included; head
    keys as weights.how_head_from_state_dict), seed (synthetic weights when
    state_dict is None), device, conv_math and stride_on as GeMModel."""

    alpha = 100.0  # VLADPooling's default (:17); HOWModel never passes another

    def __init__(self, backbone="resnet50", pretrained=False, num_classes=1000, local_dim=128, pooling_type="vlad",
                 num_clusters=64, state_dict=None, seed=0, device="cuda", conv_math="h2", stride_on="3x3"):
        self._check_backbone(pretrained, backbone, "models/how_vlad.py:110")
        if pooling_type not in ("vlad", "asmk"):
            raise ValueError(f"Unsupported pooling type: {pooling_type}")
        if local_dim % 32 or not 32 <= local_dim <= 256 or not 1 <= num_clusters <= 128:
            raise ValueError("HOWModel: local_dim % 32 == 0, 32 <= local_dim <= 256, 1 <= num_clusters <= 128 "
                             "(rr_how_vlad / rr_how_asmk)")
        head = self._load_head(state_dict, seed, W.how_head_from_state_dict, W.synthetic_how_head, pooling_type,
                               local_dim, num_clusters, num_classes)
        if ("weights" in head) != (pooling_type == "asmk"):
            raise ValueError(f"HOWModel: the state dict's head is not a {pooling_type} head")
        if tuple(head["centroids"].shape) != (num_clusters, local_dim) or head["final_w"].shape[0] != 2048:
            raise ValueError("HOWModel: head weight shapes do not fit local_dim and num_clusters")
        self.pooling_type = pooling_type
        self._build(head, ("local_w", "local_proj"), backbone, state_dict, seed, device, conv_math, stride_on)
        self.local_proj = HeadConv(self.w["local_w"].view(local_dim, 1, 1, -1), conv_math)
        self.local_dim, self.num_clusters = local_dim, num_clusters
        self.outputdim = 2048

    def local_map(self, x4, x4_amax=None):
        """The raw local_proj output [B,H,W,local_dim] of a trunk map x4 NHWC."""
        if self.conv_math == "h2" and x4_amax is None:
            x4_amax = ops.amax_of(x4)
        return self.local_proj(x4, x4_amax, self.w["local_b"])

    def head(self, x4, x4_amax=None, taps=None):
        """x4 NHWC -> features [B,2048] (:155-175).  taps: a dict that receives
        local (the raw local_proj rows [B,N,D]), pooled (after its L2) and
        features (tests)."""
        y = self.local_map(x4, x4_amax)
        if self.pooling_type == "vlad":
            v = ops.how_vlad(y, self.w["centroids"], self.alpha)
        else:
            v = ops.how_asmk(y, self.w["centroids"], self.w["weights"])
        v = ops.l2_normalize(v, EPS_L2, out=v)
        f = ops.linear(v, self.w["final_w"], self.w["final_b"])
        if taps is not None:
            taps.update(local=y.view(y.shape[0], -1, y.shape[-1]), pooled=v, features=f)
        return f

    @torch.no_grad()
    def extract_local_descriptors(self, x):
        """L2-normalised local descriptors [B,N,D] (:149-164), for callers: the
        pooling kernels normalise on load and never write these."""
        y = self.local_map(*self.trunk_map(self._input(x)))
        b, d = y.shape[0], y.shape[-1]
        return ops.l2_normalize(y.view(-1, d), EPS_L2).view(b, -1, d)


class _HOWWrapper(_Wrapper):
    """models/how_vlad.py:202-255: training-loop facade over HOWModel."""

    pooling_type = None

    def __init__(self, num_classes, backbone="resnet50", local_dim=128, num_clusters=64, **kw):
        super().__init__(HOWModel(backbone=backbone, num_classes=num_classes, local_dim=local_dim,
                                  pooling_type=self.pooling_type, num_clusters=num_clusters, **kw))

    def extract_local_descriptors(self, x):
        return self.backbone.extract_local_descriptors(x)


class HOWVLADWrapper(_HOWWrapper):
    pooling_type = "vlad"


class HOWASMKWrapper(_HOWWrapper):
    pooling_type = "asmk"


def get_how_vlad_model(num_classes, backbone="resnet50", **kwargs):
    return HOWVLADWrapper(num_classes=num_classes, backbone=backbone, **kwargs)


def get_how_asmk_model(num_classes, backbone="resnet50", **kwargs):
    return HOWASMKWrapper(num_classes=num_classes, backbone=backbone, **kwargs)


class SoSNetModel(_TrunkHeadModel):
    """models/sosnet.py:95-183, eval mode: resnet trunk -> SimilarityAttention
    (a per-position MLP 2048 -> 512 -> 256 -> 1, sigmoid, multiply) ->
    SecondOrderPooling (1x1 conv 2048 -> second_order_dim, centred covariance
    / (N - 1), packed upper triangle, F.normalize) -> feature_proj (Linear,
    ReLU, Dropout as a no-op, Linear); extract_descriptor adds F.normalize.

    Launches after the trunk: the attention MLP's first layer as a 1x1 conv
    with ReLU and the projection conv, RAW and without its bias (conv_math
    "h2": the f16x2 core on the trunk's max-|x| record; "f32": rr_conv2d);
    rr_linear_ex 512 -> 256 with ReLU; rr_sos_cov (the last attention layer,
    the sigmoid, the weighting, the centring, the covariance and the packing
    in one kernel chain; y_p = a_p (Wp x_p) + bp, and bp cancels under the
    centring); rr_linear_splitk with row_scale = rr_sos_cov's 1 / ||v|| and
    ReLU (the L2 over the packed vector commutes with the Linear);
    rr_linear; rr_l2_normalize.

    Constructor: the reference's (backbone, pretrained, num_classes,
    feature_dim, second_order_dim, use_attention), then state_dict (trunk keys
    as networks.ResNet accepts, the reference's index-named nn.Sequential keys
    included; head keys as weights.sos_head_from_state_dict), seed (synthetic
    weights when state_dict is None), device, conv_math and stride_on as
    GeMModel.  second_order_dim must fit rr_sos_cov (a multiple of 32 in
    32..512): at 2048 the reference drops the projection and its first Linear
    would hold 17 GB.

    get_model("sosnet_r50" | "sosnet_r101") still raises NotImplementedError:
    the names stay in OUT_OF_SCOPE and out of MODEL_REGISTRY (build the model
    with get_sosnet_model)."""

    def __init__(self, backbone="resnet50", pretrained=False, num_classes=1000, feature_dim=2048, second_order_dim=512,
                 use_attention=True, state_dict=None, seed=0, device="cuda", conv_math="h2", stride_on="3x3"):
        self._check_backbone(pretrained, backbone, "models/sosnet.py:98")
        c = second_order_dim
        if c % 32 or not 32 <= c <= 512:
            raise ValueError("SoSNetModel: second_order_dim % 32 == 0, 32 <= second_order_dim <= 512 (rr_sos_cov; at "
                             "2048 the reference drops the projection and its first Linear would hold 17 GB)")
        head = self._load_head(state_dict, seed, W.sos_head_from_state_dict, W.synthetic_sos_head, c, num_classes,
                               use_attention, feature_dim)
        if ("att_w1" in head) != bool(use_attention):
            raise ValueError("SoSNetModel: use_attention does not fit the state dict's head")
        if head["proj_w"].shape[0] != c or head["fp0_w"].shape[0] != feature_dim:
            raise ValueError("SoSNetModel: head weight shapes do not fit second_order_dim and feature_dim")
        if use_attention and (head["att_w1"].shape[0] % 32 or head["att_w2"].shape[0] % 4 or
                              not 4 <= head["att_w2"].shape[0] <= 512):
            raise ValueError("SoSNetModel: the attention MLP's widths do not fit rr_sos_cov")
        self.use_attention = bool(use_attention)
        self.att_b3 = float(head.pop("att_b3")[0]) if use_attention else 0.0  # read on the host, before any device work
        self._build(head, ("proj_w", "second_order_pool.proj"), backbone, state_dict, seed, device, conv_math,
                    stride_on)
        self.proj = HeadConv(self.w["proj_w"].view(c, 1, 1, -1), conv_math)
        if use_attention:
            self.att1 = HeadConv(self.w["att_w1"].view(self.w["att_w1"].shape[0], 1, 1, -1), conv_math)
        self.second_order_dim, self.feature_dim = c, feature_dim
        self.outputdim = feature_dim

    def head(self, x4, x4_amax=None, taps=None):
        """x4 NHWC -> features [B,feature_dim] (:144-161).  taps: a dict that
        receives att [B,N] (use_attention), cov (the packed triangle,
        un-normalised), inv_norm [B], hidden (after feature_proj's ReLU) and
        features (tests)."""
        b, n = x4.shape[0], x4.shape[1] * x4.shape[2]
        if n < 2:
            raise ValueError("SoSNetModel: a map with one position has no covariance (the reference divides by "
                             "N - 1 = 0 and returns NaN, models/sosnet.py:45)")
        if self.conv_math == "h2" and x4_amax is None:
            x4_amax = ops.amax_of(x4)
        hid = None
        if self.use_attention:
            h1 = self.att1(x4, x4_amax, self.w["att_b1"], relu=True)
            hid = ops.linear_ex(h1.view(b * n, -1), self.w["att_w2"], self.w["att_b2"], act=1).view(b, n, -1)
        z = self.proj(x4, x4_amax, None).view(b, n, -1)
        got = ops.sos_cov(z, hid, self.w.get("att_w3"), self.att_b3, want_att=taps is not None)
        hidden = ops.linear_splitk(got[0], self.w["fp0_w"], self.w["fp0_b"], row_scale=got[1], act=1)
        f = ops.linear(hidden, self.w["fp3_w"], self.w["fp3_b"])
        if taps is not None:
            taps.update(att=got[2], cov=got[0], inv_norm=got[1], hidden=hidden, features=f)
        return f


class SoSNetWrapper(_Wrapper):
    """models/sosnet.py:186-212: training-loop facade over SoSNetModel."""

    def __init__(self, num_classes, backbone="resnet50", feature_dim=2048, second_order_dim=512, use_attention=True,
                 **kw):
        super().__init__(SoSNetModel(backbone=backbone, num_classes=num_classes, feature_dim=feature_dim,
                                     second_order_dim=second_order_dim, use_attention=use_attention, **kw))


def get_sosnet_model(num_classes, backbone="resnet50", **kwargs):
    return SoSNetWrapper(num_classes=num_classes, backbone=backbone, **kwargs)


class SpoCModel(_TrunkHeadModel):
    """models/spoc.py:97-195, eval mode: resnet trunk -> ContextualAttention
    (:52-94: two 3x3 convs with BN and ReLU to context_dim channels, a 1x1
    attention conv with a sigmoid, and a 1x1 refine conv over cat[x a, ctx])
    -> SpatialPyramidPooling (:12-49: max-pools with floor-mode windows at
    pyramid_levels, the regions concatenated) -> feature_aggregation (Conv1d(1),
    BatchNorm1d, ReLU, max over the regions) -> feature_proj (Linear, ReLU,
    Dropout as a no-op, Linear); extract_descriptor adds F.normalize.

    Launches after the trunk: the two 3x3 convs with their BNs folded and ReLU
    (conv_math "h2": the f16x2 core, the first on the trunk's max-|x| record
    and publishing the record the second reads; "f32": rr_conv2d); the 1x1
    conv of feature_refine's input half Wx, RAW and without its bias, on the
    same core; rr_spoc_refine in place on it (the attention conv, the sigmoid,
    the gate, the context half Wc and the bias: refined_p = a_p (Wx x_p) +
    Wc ctx_p + b); rr_spp_max; rr_linear_groupmax with ReLU (the [B R, F]
    product stays on the chip); rr_linear_splitk with bias and ReLU, then
    rr_linear_splitk without an activation (few rows at K = 2048, rr_linear's
    K-set floor); rr_l2_normalize.  use_context=False goes from x4 straight to
    rr_spp_max.

    Constructor: the reference's (backbone, pretrained, num_classes,
    feature_dim, pyramid_levels, context_dim, use_context), then state_dict
    (trunk keys as networks.ResNet accepts, head keys as
    weights.spoc_head_from_state_dict), seed (synthetic weights when state_dict
    is None), device, conv_math and stride_on as GeMModel.  context_dim must be
    a multiple of 32 in 32..2048 (rr_spoc_refine, and the f16x2 core's Cin).
    At call time a map with H or W below the largest level raises, as the
    reference does ("stride should not be zero"), and so do more than 64
    regions (rr_linear_groupmax; the default levels give at most 54).

    get_model("spoc_r50" | "spoc_r101") still raises NotImplementedError: the
    names stay in OUT_OF_SCOPE and out of MODEL_REGISTRY (build the model with
    get_spoc_model)."""

    def __init__(self, backbone="resnet50", pretrained=False, num_classes=1000, feature_dim=2048,
                 pyramid_levels=(1, 2, 4), context_dim=512, use_context=True, state_dict=None, seed=0, device="cuda",
                 conv_math="h2", stride_on="3x3"):
        self._check_backbone(pretrained, backbone, "models/spoc.py:100")
        dc = context_dim
        if dc % 32 or not 32 <= dc <= 2048:
            raise ValueError("SpoCModel: context_dim % 32 == 0, 32 <= context_dim <= 2048 (rr_spoc_refine)")
        levels = [int(v) for v in pyramid_levels]
        if not 1 <= len(levels) <= 8 or min(levels) < 1:
            raise ValueError("SpoCModel: pyramid_levels must hold 1 to 8 levels, each >= 1 (rr_spp_max)")
        head = self._load_head(state_dict, seed, W.spoc_head_from_state_dict, W.synthetic_spoc_head, dc, num_classes,
                               use_context, feature_dim)
        if ("ce0_w" in head) != bool(use_context):
            raise ValueError("SpoCModel: use_context does not fit the state dict's head")
        if head["agg_w"].shape[0] != feature_dim or (use_context and head["ce0_w"].shape[0] != dc):
            raise ValueError("SpoCModel: head weight shapes do not fit feature_dim and context_dim")
        self.use_context = bool(use_context)
        self.pyramid_levels = levels
        self.att_b = head.pop("att_b") if use_context else 0.0  # a python float, read before any device work
        self._build(head, ("agg_w", "feature_aggregation"), backbone, state_dict, seed, device, conv_math, stride_on)
        self.convs = {}
        if use_context:
            self.convs = {k: HeadConv(self.w[k], conv_math) for k in ("ce0_w", "ce1_w", "refine_wx")}
        self.context_dim, self.feature_dim = dc, feature_dim
        self.outputdim = feature_dim

    def head(self, x4, x4_amax=None, taps=None):
        """x4 NHWC -> features [B,feature_dim] (:152-173).  taps: a dict that
        receives att [B,N] (use_context), refined [B,H,W,C], pooled [B,R,C], agg
        [B,F], hidden (after feature_proj's ReLU) and features (tests)."""
        b, hgt, wid = x4.shape[0], x4.shape[1], x4.shape[2]
        if hgt < max(self.pyramid_levels) or wid < max(self.pyramid_levels):
            raise ValueError(f"SpoCModel: a {hgt} x {wid} map is below pyramid level {max(self.pyramid_levels)} (the "
                             "reference's max_pool2d raises: stride should not be zero, models/spoc.py:27-35)")
        regions = ops.spp_regions(hgt, wid, self.pyramid_levels)
        if regions > 64:
            raise ValueError(f"SpoCModel: {regions} pyramid regions on a {hgt} x {wid} map; rr_linear_groupmax takes "
                             "at most 64 (the default levels give at most 54)")
        att = None
        refined = x4
        if self.use_context:
            c1_amax = None
            if self.conv_math == "h2":
                if x4_amax is None:
                    x4_amax = ops.amax_of(x4)
                c1_amax = ops.amax_records(1, x4.device)[0]
            c1 = self.convs["ce0_w"](x4, x4_amax, self.w["ce0_b"], pad=1, relu=True, y_amax=c1_amax)
            ctx = self.convs["ce1_w"](c1, c1_amax, self.w["ce1_b"], pad=1, relu=True)
            u = self.convs["refine_wx"](x4, x4_amax, None)
            got = ops.spoc_refine(u, ctx, self.w["att_w"], self.att_b, self.w["refine_wc"], self.w["refine_b"],
                                  want_att=taps is not None, out=u)
            refined, att = got if taps is not None else (got, None)
        pooled = ops.spp_max(refined, self.pyramid_levels)
        agg = ops.linear_groupmax(pooled, self.w["agg_w"], self.w["agg_b"], act=1)
        hidden = ops.linear_splitk(agg, self.w["fp0_w"], self.w["fp0_b"], act=1)
        f = ops.linear_splitk(hidden, self.w["fp3_w"], self.w["fp3_b"])
        if taps is not None:
            taps.update(att=None if att is None else att.view(b, hgt * wid), refined=refined, pooled=pooled, agg=agg,
                        hidden=hidden, features=f)
        return f


class SpoCWrapper(_Wrapper):
    """models/spoc.py:198-225: training-loop facade over SpoCModel."""

    def __init__(self, num_classes, backbone="resnet50", feature_dim=2048, pyramid_levels=(1, 2, 4), context_dim=512,
                 use_context=True, **kw):
        super().__init__(SpoCModel(backbone=backbone, num_classes=num_classes, feature_dim=feature_dim,
                                   pyramid_levels=pyramid_levels, context_dim=context_dim, use_context=use_context,
                                   **kw))


def get_spoc_model(num_classes, backbone="resnet50", **kwargs):
    return SpoCWrapper(num_classes=num_classes, backbone=backbone, **kwargs)


class TokenModel(_TrunkHeadModel):
    """models/token_based.py:89-159, eval mode: resnet trunk -> TokenAggregator
    (:35-86: input_proj Linear(2048, hidden_dim) per position, + the sinusoidal
    pe[i], the learnable global token in front, a post-norm nn.TransformerEncoder
    of num_layers layers (ReLU, FFN width 4 hidden_dim, LN eps 1e-5, no final
    norm), row 0, output_proj back to 2048) -> feature_proj Linear(2048,
    feature_dim); extract_descriptor adds F.normalize.  (networks.Token is the
    OTHER token model, networks/RetrievalNet.py's Token_Refine.)

    Launches after the trunk: input_proj as a 1x1 conv (conv_math "h2": the
    f16x2 core on the trunk's max-|x| record; "f32": rr_conv2d); rr_vit_tokens
    with cls = the global token and a position table whose row 0 is zero and
    row 1 + i is pe[i]; per layer but the last rr_linear_ex (QKV), rr_attention,
    rr_linear_ex (+ residual), rr_layernorm, rr_linear_ex (ReLU), rr_linear_ex
    (+ residual), rr_layernorm over all B (1 + N) rows.  Only row 0 of the last
    layer is used (:81), so that layer runs on B rows with its K and V
    projections folded into two host-side products (weights.
    tokagg_fold_last_layer; 2 heads hidden_dim^2 floats, 16 MB at the defaults):
    rr_linear (q~ = A x0 + a0), rr_cls_attn_pool (one pass over the layer's input),
    rr_linear_splitk_ex (M, + m0, + x0), rr_layernorm, rr_linear_ex (ReLU),
    rr_linear_splitk_ex (+ residual), rr_layernorm; then rr_linear x 2 and
    rr_l2_normalize.  (The two split-K launches have K = heads hidden_dim and
    4 hidden_dim on B rows: through rr_linear_ex, one workgroup per output tile
    walking all of K, the folded layer measured SLOWER than the unfolded one.)  The
    global token's rows are gathered for the B-row launches by one strided
    device copy.  head(..., fold_last=False) runs the last layer like the others
    and takes row 0: the cross-check and the timing baseline, never the default.

    Constructor: the reference's (backbone, pretrained, num_classes,
    feature_dim, hidden_dim, num_heads, num_layers), then state_dict (trunk keys
    as networks.ResNet accepts, the reference's index-named nn.Sequential keys
    included; head keys as weights.tokagg_head_from_state_dict), seed (synthetic
    weights when state_dict is None), device, conv_math and stride_on as
    GeMModel.  hidden_dim % 64 == 0 in 64..1024, 1 <= num_heads <= 16 dividing it
    (rr_cls_attn_pool), hidden_dim == 64 num_heads when num_layers > 1
    (rr_attention), num_layers >= 1.  The reference's pe buffer has max_len = 196
    rows and its broadcast raises on more positions, so inputs go up to 448 x 448.

    get_model("token_r50" | "token_r101") still raises NotImplementedError:
    the names stay in OUT_OF_SCOPE and out of MODEL_REGISTRY (build the model
    with get_token_model)."""

    def __init__(self, backbone="resnet50", pretrained=False, num_classes=1000, feature_dim=2048, hidden_dim=512,
                 num_heads=8, num_layers=2, state_dict=None, seed=0, device="cuda", conv_math="h2", stride_on="3x3"):
        self._check_backbone(pretrained, backbone, "models/token_based.py:92")
        d, nh = hidden_dim, num_heads
        if d % 64 or not 64 <= d <= 1024:
            raise ValueError("TokenModel: hidden_dim % 64 == 0, 64 <= hidden_dim <= 1024 (rr_cls_attn_pool)")
        if not 1 <= nh <= 16 or d % nh:
            raise ValueError("TokenModel: 1 <= num_heads <= 16, num_heads dividing hidden_dim (rr_cls_attn_pool)")
        if num_layers < 1:
            raise ValueError("TokenModel: num_layers >= 1")
        if num_layers > 1 and d != 64 * nh:
            raise ValueError("TokenModel: hidden_dim == 64 num_heads when num_layers > 1 (rr_attention's head width)")
        head = self._load_head(state_dict, seed, W.tokagg_head_from_state_dict, W.synthetic_tokagg_head, d, nh,
                               num_layers, num_classes, feature_dim)
        if head["in_w"].shape[0] != d or W.tokagg_num_layers(head) != num_layers or \
                head["fp_w"].shape[0] != feature_dim:
            raise ValueError("TokenModel: head weight shapes do not fit hidden_dim, num_layers and feature_dim")
        a, a0, m, m0 = W.tokagg_fold_last_layer(W.tokagg_layer(head, num_layers - 1), nh)
        pos = torch.cat([torch.zeros(1, d), head.pop("pe")]).contiguous()  # row 0: the global token gets no term
        self.max_len = pos.shape[0] - 1
        self._build(head, ("in_w", "token_aggregator.input_proj"), backbone, state_dict, seed, device, conv_math,
                    stride_on)
        self.w.update(pos=pos.to(self.device), fold_a=a.to(self.device), fold_a0=a0.to(self.device),
                      fold_m=m.to(self.device), fold_m0=m0.to(self.device))
        self.input_proj = HeadConv(self.w["in_w"].view(d, 1, 1, -1), conv_math)
        self.hidden_dim, self.num_heads, self.num_layers, self.feature_dim = d, nh, num_layers, feature_dim
        self.outputdim = feature_dim

    def _full_layer(self, x, i, b, seq):
        """Encoder layer i on all rows x [b seq, d] (nn.TransformerEncoderLayer, post-norm)."""
        w = self.w
        qkv = ops.linear_ex(x, w[f"l{i}_qkv_w"], w[f"l{i}_qkv_b"])
        att = ops.attention(qkv, b, seq, self.num_heads, self.hidden_dim // self.num_heads)
        y = ops.linear_ex(att, w[f"l{i}_out_w"], w[f"l{i}_out_b"], residual=x)
        return self._ffn(ops.layernorm(y, w[f"l{i}_n1_g"], w[f"l{i}_n1_b"], 1e-5), i)

    def _ffn(self, y, i, few_rows=False):
        """linear1, ReLU, linear2, + residual, norm2.  few_rows (the folded layer's B
        rows): linear2, K = 4 hidden_dim, on the split-K path."""
        w = self.w
        hid = ops.linear_ex(y, w[f"l{i}_l1_w"], w[f"l{i}_l1_b"], act=1)
        if few_rows:
            z = ops.linear_splitk(hid, w[f"l{i}_l2_w"], w[f"l{i}_l2_b"], residual=y)
        else:
            z = ops.linear_ex(hid, w[f"l{i}_l2_w"], w[f"l{i}_l2_b"], residual=y)
        return ops.layernorm(z, w[f"l{i}_n2_g"], w[f"l{i}_n2_b"], 1e-5)

    def _folded_last_layer(self, x, b, seq, taps):
        """Row 0 of the last layer's output from its input x [b seq, d]: [b, d]."""
        w, d, nh, i = self.w, self.hidden_dim, self.num_heads, self.num_layers - 1
        x3 = x.view(b, seq, d)
        x0 = x3[:, 0].contiguous()
        qt = ops.linear(x0, w["fold_a"], w["fold_a0"]).view(b, nh, d)
        got = ops.cls_attn_pool(x3, qt, want_p=taps is not None)
        pooled = got[0] if taps is not None else got
        if taps is not None:
            taps.update(p=got[1], pooled=pooled)
        y = ops.linear_splitk(pooled.view(b, nh * d), w["fold_m"], w["fold_m0"], residual=x0)
        return self._ffn(ops.layernorm(y, w[f"l{i}_n1_g"], w[f"l{i}_n1_b"], 1e-5), i, few_rows=True)

    def head(self, x4, x4_amax=None, taps=None, fold_last=True):
        """x4 NHWC -> features [B,feature_dim] (:126-137).  taps: a dict that
        receives tokens [B,1+N,d], layer_out (the last layer's input), p
        [B,heads,1+N] and pooled [B,heads,d] (fold_last only), agg [B,2048] and
        features (tests).  fold_last=False: the last layer over all rows with
        the other layers' kernels, row 0 taken afterwards."""
        b, n, d = x4.shape[0], x4.shape[1] * x4.shape[2], self.hidden_dim
        if n > self.max_len:
            raise ValueError(f"TokenModel: {n} positions exceed the positional encoding's max_len = {self.max_len} "
                             "(models/token_based.py:16, :32: the reference's broadcast raises; inputs up to 448 x 448)")
        seq = 1 + n
        if self.conv_math == "h2" and x4_amax is None:
            x4_amax = ops.amax_of(x4)
        y = self.input_proj(x4, x4_amax, self.w["in_b"])
        x = ops.vit_tokens(y.view(b * n, d), b, self.w["global_token"], self.w["pos"])
        if taps is not None:
            taps["tokens"] = x.view(b, seq, d)
        for i in range(self.num_layers - 1):
            x = self._full_layer(x, i, b, seq)
        if taps is not None:
            taps["layer_out"] = x.view(b, seq, d)
        if fold_last:
            g = self._folded_last_layer(x, b, seq, taps)
        else:
            g = self._full_layer(x, self.num_layers - 1, b, seq).view(b, seq, d)[:, 0].contiguous()
        agg = ops.linear(g, self.w["op_w"], self.w["op_b"])
        f = ops.linear(agg, self.w["fp_w"], self.w["fp_b"])
        if taps is not None:
            taps.update(agg=agg, features=f)
        return f


class TokenWrapper(_Wrapper):
    """models/token_based.py:162-189: training-loop facade over TokenModel."""

    def __init__(self, num_classes, backbone="resnet50", feature_dim=2048, hidden_dim=512, num_heads=8, num_layers=2,
                 **kw):
        super().__init__(TokenModel(backbone=backbone, num_classes=num_classes, feature_dim=feature_dim,
                                    hidden_dim=hidden_dim, num_heads=num_heads, num_layers=num_layers, **kw))


def get_token_model(num_classes, backbone="resnet50", **kwargs):
    return TokenWrapper(num_classes=num_classes, backbone=backbone, **kwargs)


class SENetG2Model(_TrunkHeadModel):
    """models/senet_g2.py:156-213, eval mode: the SE-ResNet trunk
    (networks.SENet) -> G2Pooling (:132-153: GeM with a learnable p, then
    alpha * g + beta) -> feature_proj Linear(2048, feature_dim);
    extract_descriptor adds F.normalize.

    Launches after the trunk: rr_gem_pool with p read from g2_pool.p (eps
    1e-6), one rr_linear with alpha and beta folded into the projection on the
    host (weights.senet_g2_fold: W' = alpha W, b' = b + beta W 1, float64,
    rounded once), rr_l2_normalize.

    Constructor: the reference's (layers, num_classes, feature_dim, reduction,
    gem_p), then state_dict (trunk keys as networks.SENet accepts, head keys as
    weights.senet_g2_head_from_state_dict; at the wrapper's level, the model's,
    or either under ``module.``), seed (synthetic weights when state_dict is
    None), device and conv_math as GeMModel.  layers: (3, 4, 6, 3) or (3, 4, 23,
    3), or the backbone's name "senet50" / "senet101".  There is no pretrained
    argument: the reference's SENet is randomly initialised (:93-99).

    get_model("senet_g2_50" | "senet_g2_101") still raises NotImplementedError:
    the names stay in OUT_OF_SCOPE and out of MODEL_REGISTRY (build the model
    with get_senet_g2_model)."""

    _LAYERS = {(3, 4, 6, 3): "senet50", (3, 4, 23, 3): "senet101"}

    def __init__(self, layers=(3, 4, 6, 3), num_classes=1000, feature_dim=2048, reduction=16, gem_p=3.0,
                 state_dict=None, seed=0, device="cuda", conv_math="h2"):
        name = layers if isinstance(layers, str) else self._LAYERS.get(tuple(int(v) for v in layers))
        if name not in W.SENET_TRUNKS:
            raise ValueError(f"Unsupported backbone: {layers}")
        self.reduction = W.senet_check_reduction(reduction)
        head = self._load_head(state_dict, seed, W.senet_g2_head_from_state_dict, W.synthetic_senet_g2_head,
                               num_classes, feature_dim, gem_p)
        if head["proj_w"].shape[0] != feature_dim:
            raise ValueError("SENetG2Model: head weight shapes do not fit feature_dim")
        # python floats, read before any device work
        self.p, self.alpha, self.beta = (head.pop(k) for k in ("p", "alpha", "beta"))
        self._build(head, ("proj_w", "feature_proj"), name, state_dict, seed, device, conv_math, "3x3")
        self.feature_dim = feature_dim
        self.outputdim = feature_dim

    def _make_trunk(self, backbone, state_dict, seed, device, conv_math, stride_on):
        return SENet(backbone, state_dict, seed, device, conv_math=conv_math, reduction=self.reduction)

    def head(self, x4, x4_amax=None, taps=None):
        """x4 NHWC -> features [B,feature_dim] (:179-191).  taps: a dict that
        receives pooled [B,2048] (the GeM before alpha and beta) and features
        (tests)."""
        pooled = ops.gem_pool(x4, self.p, 1e-6)
        f = ops.linear(pooled, self.w["proj_wf"], self.w["proj_bf"])
        if taps is not None:
            taps.update(pooled=pooled, features=f)
        return f


class SENetG2Wrapper(_Wrapper):
    """models/senet_g2.py:216-251: training-loop facade over SENetG2Model."""

    def __init__(self, num_classes, backbone="senet50", feature_dim=2048, reduction=16, gem_p=3.0, **kw):
        if backbone not in W.SENET_TRUNKS:
            raise ValueError(f"Unsupported backbone: {backbone}")
        super().__init__(SENetG2Model(layers=backbone, num_classes=num_classes, feature_dim=feature_dim,
                                      reduction=reduction, gem_p=gem_p, **kw))


def get_senet_g2_model(num_classes, backbone="senet50", **kwargs):
    return SENetG2Wrapper(num_classes=num_classes, backbone=backbone, **kwargs)


MODEL_REGISTRY = {
    "gem_r50": lambda num_classes, **kw: get_gem_model(num_classes, backbone="resnet50", **kw),
    "gem_r101": lambda num_classes, **kw: get_gem_model(num_classes, backbone="resnet101", **kw),
    "how_vlad_r50": lambda num_classes, **kw: get_how_vlad_model(num_classes, backbone="resnet50", **kw),
    "how_vlad_r101": lambda num_classes, **kw: get_how_vlad_model(num_classes, backbone="resnet101", **kw),
    "how_asmk_r50": lambda num_classes, **kw: get_how_asmk_model(num_classes, backbone="resnet50", **kw),
    "how_asmk_r101": lambda num_classes, **kw: get_how_asmk_model(num_classes, backbone="resnet101", **kw),
}

# Other Table-1 methods exist in the reference registry (models/wrappers.py:22-50)
# but are outside this build's hot path.
OUT_OF_SCOPE = ("delg_r50", "delg_r101", "token_r50", "token_r101", "senet_g2_50", "senet_g2_101", "sosnet_r50",
                "sosnet_r101", "spoc_r50", "spoc_r101")


def get_model(model_name, num_classes, **kwargs):
    """Factory by name (models/wrappers.py:74-90)."""
    if model_name not in MODEL_REGISTRY:
        if model_name in OUT_OF_SCOPE:
            raise NotImplementedError(f"{model_name} is outside the accelerated hot path (SURVEY.md §2)")
        raise ValueError(f"Unknown model: {model_name}. Available models: {list(MODEL_REGISTRY)}")
    return MODEL_REGISTRY[model_name](num_classes, **kwargs)
