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
Training (``forward(x, targets)`` losses, optimizers) is out of scope
(SURVEY.md §2 row 13): ``forward`` only produces eval-mode logits.
"""
import torch

from . import ops
from . import weights as W
from .networks import ResNet, _Extractor, EPS_L2


class GeMPooling:
    """GeM with a tensor-valued p (models/gem_pooling.py:12-23).  The
    reference stores p as a 1-element Parameter; the exponent 1/p is formed
    in fp32 from it, which is what gem_pool's powf path does."""

    def __init__(self, p=3.0, eps=1e-6):
        self.p = torch.ones(1) * p
        self.eps = eps

    def __call__(self, x_nhwc):
        return ops.gem_pool(x_nhwc, float(self.p.item()), self.eps)


class GeMModel(_Extractor):
    """resnet trunk -> GeMPooling -> feature_proj Linear(2048, feature_dim)
    (models/gem_pooling.py:26-92); extract_descriptor adds F.normalize(p=2, dim=1)."""

    in_channels = 4

    def __init__(self, backbone="resnet50", pretrained=False, num_classes=1000, feature_dim=2048, gem_p=3.0,
                 state_dict=None, seed=0, device="cuda", conv_math="h2", stride_on="3x3"):
        if pretrained:
            raise ValueError("pretrained weights need a download; pass a local state_dict instead "
                             "(models/gem_pooling.py:35 defaults to pretrained=True)")
        if backbone not in ("resnet50", "resnet101"):
            raise ValueError(f"Unsupported backbone: {backbone}")
        self.device = torch.device(device)
        self.backbone = ResNet(backbone, state_dict, seed, device, conv_math=conv_math, stride_on=stride_on)
        self.gem_pool = GeMPooling(p=gem_p)
        backbone_dim = 2048
        pw, pb = _from_sd(state_dict, "feature_proj") or W.synthetic_linear(feature_dim, backbone_dim, seed + 2)
        self.proj_w = pw.float().contiguous().to(self.device)
        self.proj_b = pb.float().contiguous().to(self.device)
        cw, cb = _from_sd(state_dict, "classifier") or W.synthetic_linear(num_classes, feature_dim, seed + 3)
        self.cls_w = cw.float().contiguous().to(self.device)
        self.cls_b = cb.float().contiguous().to(self.device)
        self.feature_dim = feature_dim
        self.outputdim = feature_dim

    def extract_features_nhwc(self, x_nhwc):
        f = self.backbone(x_nhwc)
        f = self.gem_pool(f)
        return ops.linear(f, self.proj_w, self.proj_b)

    @torch.no_grad()
    def extract_features(self, x):
        return self.extract_features_nhwc(self._input(x))

    def forward_test_nhwc(self, x_nhwc):
        f = self.extract_features_nhwc(x_nhwc)
        return ops.l2_normalize(f, EPS_L2, out=f)

    @torch.no_grad()
    def extract_descriptor(self, x):
        return self.forward_test(x)

    @torch.no_grad()
    def forward(self, x, targets=None):
        feats = self.extract_features(x)
        return None, ops.linear(feats, self.cls_w, self.cls_b)

    __call__ = forward


def _from_sd(sd, name):
    if sd is None:
        return None
    for pre in ("", "backbone.", "module.backbone."):
        k = f"{pre}{name}.weight"
        if k in sd:
            return sd[k], sd[f"{pre}{name}.bias"]
    return None


class GeMWrapper(_Extractor):
    """models/gem_pooling.py:95-119: training-loop facade over GeMModel."""

    in_channels = 4

    def __init__(self, num_classes, backbone="resnet50", feature_dim=2048, gem_p=3.0, **kw):
        self.backbone = GeMModel(backbone=backbone, num_classes=num_classes, feature_dim=feature_dim, gem_p=gem_p,
                                 **kw)
        self.outputdim = feature_dim

    def forward_test_nhwc(self, x_nhwc):
        return self.backbone.forward_test_nhwc(x_nhwc)

    @torch.no_grad()
    def forward(self, x, targets=None):
        return self.backbone(x)

    __call__ = forward

    @torch.no_grad()
    def extract_global_descriptor(self, x):
        return self.backbone.extract_descriptor(x)


def get_gem_model(num_classes, backbone="resnet50", **kwargs):
    return GeMWrapper(num_classes=num_classes, backbone=backbone, **kwargs)


class HOWModel(_Extractor):
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

    in_channels = 4
    alpha = 100.0  # VLADPooling's default (:17); HOWModel never passes another

    def __init__(self, backbone="resnet50", pretrained=False, num_classes=1000, local_dim=128, pooling_type="vlad",
                 num_clusters=64, state_dict=None, seed=0, device="cuda", conv_math="h2", stride_on="3x3"):
        if pretrained:
            raise ValueError("pretrained weights need a download; pass a local state_dict instead "
                             "(models/how_vlad.py:110 defaults to pretrained=True)")
        if backbone not in ("resnet50", "resnet101"):
            raise ValueError(f"Unsupported backbone: {backbone}")
        if pooling_type not in ("vlad", "asmk"):
            raise ValueError(f"Unsupported pooling type: {pooling_type}")
        if local_dim % 32 or not 32 <= local_dim <= 256 or not 1 <= num_clusters <= 128:
            raise ValueError("HOWModel: local_dim % 32 == 0, 32 <= local_dim <= 256, 1 <= num_clusters <= 128 "
                             "(rr_how_vlad / rr_how_asmk)")
        if state_dict is None:
            head = W.how_head_from_state_dict(W.synthetic_how_head(seed + 1, pooling_type, local_dim, num_clusters,
                                                                   num_classes))
        else:
            head = W.how_head_from_state_dict(state_dict)
        if ("weights" in head) != (pooling_type == "asmk"):
            raise ValueError(f"HOWModel: the state dict's head is not a {pooling_type} head")
        if tuple(head["centroids"].shape) != (num_clusters, local_dim) or head["final_w"].shape[0] != 2048:
            raise ValueError("HOWModel: head weight shapes do not fit local_dim and num_clusters")
        self.device = torch.device(device)
        self.conv_math = conv_math
        self.pooling_type = pooling_type
        self.backbone = ResNet(backbone, state_dict, seed, device, conv_math=conv_math, stride_on=stride_on)
        if head["local_w"].shape[1] != self.backbone.outputdim_block5:
            raise ValueError("HOWModel: local_proj does not fit the trunk")
        self.w = {k: v.to(self.device) for k, v in head.items()}
        self.local_w = self.w["local_w"].view(local_dim, 1, 1, -1)
        self.local_h2 = ops.H2Conv(self.local_w) if conv_math == "h2" else None
        self.local_dim, self.num_clusters = local_dim, num_clusters
        self.outputdim = 2048

    def local_map(self, x4, x4_amax=None):
        """The raw local_proj output [B,H,W,local_dim] of a trunk map x4 NHWC."""
        if self.conv_math == "h2":
            if x4_amax is None:
                x4_amax = ops.amax_f32(x4, ops.amax_records(1, x4.device)[0])
            return ops.conv2d_h2(x4, x4_amax, self.local_h2, self.w["local_b"], 1, 0, None, False)
        return ops.conv2d(x4, self.local_w, self.w["local_b"], 1, 0, None, False)

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

    def _trunk(self, x_nhwc, hook=None):
        if self.conv_math == "h2":
            return self.backbone(x_nhwc, hook=hook, return_amax=True)
        return self.backbone(x_nhwc), None

    def extract_features_nhwc(self, x_nhwc, hook=None):
        return self.head(*self._trunk(x_nhwc, hook))

    @torch.no_grad()
    def extract_local_descriptors(self, x):
        """L2-normalised local descriptors [B,N,D] (:149-164), for callers: the
        pooling kernels normalise on load and never write these."""
        y = self.local_map(*self._trunk(self._input(x)))
        b, d = y.shape[0], y.shape[-1]
        return ops.l2_normalize(y.view(-1, d), EPS_L2).view(b, -1, d)

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

    __call__ = forward


class _HOWWrapper(_Extractor):
    """models/how_vlad.py:202-255: training-loop facade over HOWModel."""

    in_channels = 4
    pooling_type = None

    def __init__(self, num_classes, backbone="resnet50", local_dim=128, num_clusters=64, **kw):
        self.backbone = HOWModel(backbone=backbone, num_classes=num_classes, local_dim=local_dim,
                                 pooling_type=self.pooling_type, num_clusters=num_clusters, **kw)
        self.outputdim = self.backbone.outputdim

    def forward_test_nhwc(self, x_nhwc, hook=None):
        return self.backbone.forward_test_nhwc(x_nhwc, hook)

    @torch.no_grad()
    def forward(self, x, targets=None):
        return self.backbone(x)

    __call__ = forward

    def extract_local_descriptors(self, x):
        return self.backbone.extract_local_descriptors(x)

    def extract_features(self, x):
        return self.backbone.extract_features(x)

    def extract_descriptor(self, x):
        return self.backbone.extract_descriptor(x)

    def extract_global_descriptor(self, x):
        return self.backbone.extract_descriptor(x)


class HOWVLADWrapper(_HOWWrapper):
    pooling_type = "vlad"


class HOWASMKWrapper(_HOWWrapper):
    pooling_type = "asmk"


def get_how_vlad_model(num_classes, backbone="resnet50", **kwargs):
    return HOWVLADWrapper(num_classes=num_classes, backbone=backbone, **kwargs)


def get_how_asmk_model(num_classes, backbone="resnet50", **kwargs):
    return HOWASMKWrapper(num_classes=num_classes, backbone=backbone, **kwargs)


class SoSNetModel(_Extractor):
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

    in_channels = 4

    def __init__(self, backbone="resnet50", pretrained=False, num_classes=1000, feature_dim=2048, second_order_dim=512,
                 use_attention=True, state_dict=None, seed=0, device="cuda", conv_math="h2", stride_on="3x3"):
        if pretrained:
            raise ValueError("pretrained weights need a download; pass a local state_dict instead "
                             "(models/sosnet.py:98 defaults to pretrained=True)")
        if backbone not in ("resnet50", "resnet101"):
            raise ValueError(f"Unsupported backbone: {backbone}")
        c = second_order_dim
        if c % 32 or not 32 <= c <= 512:
            raise ValueError("SoSNetModel: second_order_dim % 32 == 0, 32 <= second_order_dim <= 512 (rr_sos_cov; at "
                             "2048 the reference drops the projection and its first Linear would hold 17 GB)")
        if state_dict is None:
            head = W.sos_head_from_state_dict(W.synthetic_sos_head(seed + 1, c, num_classes, use_attention,
                                                                   feature_dim))
        else:
            head = W.sos_head_from_state_dict(state_dict)
        if ("att_w1" in head) != bool(use_attention):
            raise ValueError("SoSNetModel: use_attention does not fit the state dict's head")
        if head["proj_w"].shape[0] != c or head["fp0_w"].shape[0] != feature_dim:
            raise ValueError("SoSNetModel: head weight shapes do not fit second_order_dim and feature_dim")
        if use_attention and (head["att_w1"].shape[0] % 32 or head["att_w2"].shape[0] % 4 or
                              not 4 <= head["att_w2"].shape[0] <= 512):
            raise ValueError("SoSNetModel: the attention MLP's widths do not fit rr_sos_cov")
        self.device = torch.device(device)
        self.conv_math = conv_math
        self.use_attention = bool(use_attention)
        self.att_b3 = float(head.pop("att_b3")[0]) if use_attention else 0.0  # read on the host, before any device work
        self.backbone = ResNet(backbone, state_dict, seed, device, conv_math=conv_math, stride_on=stride_on)
        if head["proj_w"].shape[1] != self.backbone.outputdim_block5:
            raise ValueError("SoSNetModel: second_order_pool.proj does not fit the trunk")
        self.w = {k: v.to(self.device) for k, v in head.items()}
        self.proj_w = self.w["proj_w"].view(c, 1, 1, -1)
        self.proj_h2 = ops.H2Conv(self.proj_w) if conv_math == "h2" else None
        if use_attention:
            self.att_w1 = self.w["att_w1"].view(self.w["att_w1"].shape[0], 1, 1, -1)
            self.att_h2 = ops.H2Conv(self.att_w1) if conv_math == "h2" else None
        self.second_order_dim, self.feature_dim = c, feature_dim
        self.outputdim = feature_dim

    def _conv(self, x4, x4_amax, w, wc, bias, relu):
        if self.conv_math == "h2":
            return ops.conv2d_h2(x4, x4_amax, wc, bias, 1, 0, None, relu)
        return ops.conv2d(x4, w, bias, 1, 0, None, relu)

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
            x4_amax = ops.amax_f32(x4, ops.amax_records(1, x4.device)[0])
        hid = None
        if self.use_attention:
            h1 = self._conv(x4, x4_amax, self.att_w1, self.att_h2, self.w["att_b1"], True)
            hid = ops.linear_ex(h1.view(b * n, -1), self.w["att_w2"], self.w["att_b2"], act=1).view(b, n, -1)
        z = self._conv(x4, x4_amax, self.proj_w, self.proj_h2, None, False).view(b, n, -1)
        got = ops.sos_cov(z, hid, self.w.get("att_w3"), self.att_b3, want_att=taps is not None)
        hidden = ops.linear_splitk(got[0], self.w["fp0_w"], self.w["fp0_b"], row_scale=got[1], act=1)
        f = ops.linear(hidden, self.w["fp3_w"], self.w["fp3_b"])
        if taps is not None:
            taps.update(att=got[2], cov=got[0], inv_norm=got[1], hidden=hidden, features=f)
        return f

    def _trunk(self, x_nhwc, hook=None):
        if self.conv_math == "h2":
            return self.backbone(x_nhwc, hook=hook, return_amax=True)
        return self.backbone(x_nhwc), None

    def extract_features_nhwc(self, x_nhwc, hook=None):
        return self.head(*self._trunk(x_nhwc, hook))

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

    __call__ = forward


class SoSNetWrapper(_Extractor):
    """models/sosnet.py:186-212: training-loop facade over SoSNetModel."""

    in_channels = 4

    def __init__(self, num_classes, backbone="resnet50", feature_dim=2048, second_order_dim=512, use_attention=True,
                 **kw):
        self.backbone = SoSNetModel(backbone=backbone, num_classes=num_classes, feature_dim=feature_dim,
                                    second_order_dim=second_order_dim, use_attention=use_attention, **kw)
        self.outputdim = self.backbone.outputdim

    def forward_test_nhwc(self, x_nhwc, hook=None):
        return self.backbone.forward_test_nhwc(x_nhwc, hook)

    @torch.no_grad()
    def forward(self, x, targets=None):
        return self.backbone(x)

    __call__ = forward

    def extract_features(self, x):
        return self.backbone.extract_features(x)

    def extract_descriptor(self, x):
        return self.backbone.extract_descriptor(x)

    def extract_global_descriptor(self, x):
        return self.backbone.extract_descriptor(x)


def get_sosnet_model(num_classes, backbone="resnet50", **kwargs):
    return SoSNetWrapper(num_classes=num_classes, backbone=backbone, **kwargs)


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
