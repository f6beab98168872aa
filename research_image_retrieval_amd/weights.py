"""Backbone weights: seeded synthetic torchvision-keyed state dicts, local
checkpoint loading, reference key-layout remaps and eval-mode BN folding.

No network access exists (pretrained=True/'v1'/'v2' in the reference downloads
ImageNet weights, networks/backbone.py:63-72, models/gem_pooling.py:35-38), so
weights come either from a LOCAL torchvision-keyed file or from a seeded
generator.  The generator uses numpy RandomState (stream-stable across numpy
versions) so the oracle, the tests and bench.py all rebuild identical weights
from a seed.
"""
import collections
import functools
import math

import numpy as np
import torch

# torchvision resnet{50,101} bottleneck counts (networks/backbone.py:63-72 via
# torchvision.models.resnet50/101; models/gem_pooling.py:34-38)
RESNET_LAYERS = {"resnet50": (3, 4, 6, 3), "resnet101": (3, 4, 23, 3), "resnet152": (3, 8, 36, 3)}
BN_EPS = 1e-5
# Where a downsampling bottleneck puts its stride: "3x3" = torchvision v1.5
# (conv2), "1x1" = MSRA / pycls, the reference's own torchvision-free R101
# (networks/backbone.py:310-312: BottleneckTransform.a carries the stride).
STRIDE_ON = ("3x3", "1x1")
_BN_KEYS = ("weight", "bias", "running_mean", "running_var")


def _t(a):
    """A numpy array as a contiguous fp32 tensor (the synthetic draws are float64)."""
    return torch.from_numpy(np.ascontiguousarray(a, dtype=np.float32))


def _f(a):
    return a.float().contiguous()


def _flat_keys(sd):
    """sd keyed without a leading ``module.`` and without the wrappers' leading
    ``backbone.`` after it; of two keys that then meet, the first stays."""
    flat = {}
    for k, v in sd.items():
        for lead in ("module.", "backbone."):
            if k.startswith(lead):
                k = k[len(lead):]
        flat.setdefault(k, v)
    return flat


def _lin(rs, sd, key, out_dim, in_dim, shape=None, gain=1.0, zero_sum=False):
    """sd[key.weight], sd[key.bias] drawn from rs as PyTorch's default init,
    U(+-1 / sqrt(in_dim)); the weight (not the bias) gain times wider, each row
    shifted to sum to zero (zero_sum) and reshaped to shape.  Drawn in blocks
    of 64 rows so that the float64 draws of the widest layers stay small: the
    stream, and so every bit, is the same at any block size."""
    s = 1.0 / np.sqrt(in_dim)
    w = np.empty((out_dim, in_dim), dtype=np.float32)
    for r0 in range(0, out_dim, 64):
        blk = rs.uniform(-1, 1, (min(64, out_dim - r0), in_dim)) * (s * gain)
        w[r0:r0 + 64] = blk - blk.mean(axis=1, keepdims=True) if zero_sum else blk
    sd[key + ".weight"] = _t(w.reshape(shape) if shape else w)
    sd[key + ".bias"] = _t(rs.uniform(-1, 1, out_dim) * s)


def block_strides(stride, stride_on):
    """(conv1 stride, conv2 stride) of a bottleneck whose block stride is `stride`."""
    if stride_on not in STRIDE_ON:
        raise ValueError(f"stride_on must be one of {STRIDE_ON}")
    return (1, stride) if stride_on == "3x3" else (stride, 1)


TrunkBlock = collections.namedtuple("TrunkBlock", "prefix stage index entry stride s1 s2 inplanes planes cout stage_end")


@functools.lru_cache(maxsize=None)
def trunk_blocks(arch, stride_on="3x3"):
    """The bottleneck trunk's block schedule, the one place that decides it: a
    tuple of TrunkBlock in forward order for arch (a RESNET_LAYERS name).
    prefix "layer{stage + 1}.{index}"; entry: the block has a downsample
    projection (a stage's first block); stride: the block's (2 where a stage
    but the first begins), s1 / s2: conv1's / conv2's (block_strides); the
    channel chain inplanes -> planes -> planes -> cout; stage_end: a stage's
    last block."""
    blocks, inplanes = [], 64
    for li, nb in enumerate(RESNET_LAYERS[arch]):
        planes = 64 << li
        for bi in range(nb):
            stride = 2 if (bi == 0 and li > 0) else 1
            blocks.append(TrunkBlock(f"layer{li + 1}.{bi}", li, bi, bi == 0, stride, *block_strides(stride, stride_on),
                                     inplanes, planes, planes * 4, bi == nb - 1))
            inplanes = planes * 4
    return tuple(blocks)


def conv_out(n, k, s, p):
    """Output positions of a conv or pool: n inputs, kernel k, stride s, padding p."""
    return (n + 2 * p - k) // s + 1


def trunk_block_maps(arch, h, w, stride_on="3x3"):
    """trunk_blocks for an h x w image, each block with its map sizes: yields
    (block, (H, W) its input, (H1, W1) after the 1x1 conv1, (Ho, Wo) its
    output); the first input is the stem's 7x7/2 conv and 3x3/2 max-pool of h x w."""
    H, Wd = (conv_out(conv_out(n, 7, 2, 3), 3, 2, 1) for n in (h, w))
    for b in trunk_blocks(arch, stride_on):
        H1, W1 = conv_out(H, 1, b.s1, 0), conv_out(Wd, 1, b.s1, 0)
        Ho, Wo = conv_out(H1, 3, b.s2, 1), conv_out(W1, 3, b.s2, 1)
        yield b, (H, Wd), (H1, W1), (Ho, Wo)
        H, Wd = Ho, Wo


def resnet_conv_specs(arch):
    """Ordered (prefix, cout, cin, k) of every conv + its BN prefix, torchvision layout."""
    specs = [("conv1", "bn1", 64, 3, 7)]
    for b in trunk_blocks(arch):
        p = b.prefix
        specs.append((f"{p}.conv1", f"{p}.bn1", b.planes, b.inplanes, 1))
        specs.append((f"{p}.conv2", f"{p}.bn2", b.planes, b.planes, 3))
        specs.append((f"{p}.conv3", f"{p}.bn3", b.cout, b.planes, 1))
        if b.entry:
            specs.append((f"{p}.downsample.0", f"{p}.downsample.1", b.cout, b.inplanes, 1))
    return specs


def synthetic_resnet_state_dict(arch="resnet101", seed=0):
    """Seeded torchvision-keyed trunk weights (conv1..layer4; no fc).

    Convs: Kaiming-normal (fan_out, ReLU), as torchvision's init.  BatchNorm
    running statistics and affine parameters are randomised (not identity) so
    that BN folding is exercised; the last BN of every bottleneck gets a small
    gamma so activations stay O(1) through 33 residual blocks."""
    rs = np.random.RandomState(seed)
    sd = collections.OrderedDict()
    for conv, bn, cout, cin, k in resnet_conv_specs(arch):
        std = np.sqrt(2.0 / (cout * k * k))
        sd[conv + ".weight"] = torch.from_numpy((rs.standard_normal((cout, cin, k, k)) * std).astype(np.float32))
        last = bn.endswith("bn3") or bn.endswith("downsample.1")
        lo, hi = (0.05, 0.25) if last else (0.5, 1.0)
        sd[bn + ".weight"] = torch.from_numpy(rs.uniform(lo, hi, cout).astype(np.float32))
        sd[bn + ".bias"] = torch.from_numpy((rs.standard_normal(cout) * 0.05).astype(np.float32))
        sd[bn + ".running_mean"] = torch.from_numpy((rs.standard_normal(cout) * 0.05).astype(np.float32))
        sd[bn + ".running_var"] = torch.from_numpy(rs.uniform(0.5, 1.5, cout).astype(np.float32))
        sd[bn + ".num_batches_tracked"] = torch.tensor(0, dtype=torch.int64)
    return sd


def synthetic_linear(out_dim, in_dim, seed, bias=True, scale=None):
    """Seeded Linear / 1x1-conv weights ([out,in], [out])."""
    rs = np.random.RandomState(seed)
    s = scale if scale is not None else 1.0 / np.sqrt(in_dim)
    w = torch.from_numpy((rs.uniform(-1, 1, (out_dim, in_dim)) * s).astype(np.float32))
    b = torch.from_numpy((rs.uniform(-1, 1, out_dim) * s).astype(np.float32)) if bias else None
    return w, b


# ---- reference key layouts -------------------------------------------------
# networks.ResNet (networks/backbone.py:93-101) renames children[:-2] into
# block1 = [conv1, bn1, relu, maxpool], block2..5 = layer1..4;
# GeMModel (models/gem_pooling.py:44) keeps nn.Sequential indices 0..7.
_SEQ_TO_TV = {"0": "conv1", "1": "bn1", "4": "layer1", "5": "layer2", "6": "layer3", "7": "layer4"}
_BLOCK_TO_TV = {"block2": "layer1", "block3": "layer2", "block4": "layer3", "block5": "layer4"}
# ResNet_DOLG (networks/backbone.py:218-274, blocks :305-345): stem.{conv,bn},
# s{K}.b{M}.{proj,bn} (projection shortcut), s{K}.b{M}.f.{a,a_bn,b,b_bn,c,c_bn}
_DOLG_F_TO_TV = {"a": "conv1", "a_bn": "bn1", "b": "conv2", "b_bn": "bn2", "c": "conv3", "c_bn": "bn3"}
_DOLG_SC_TO_TV = {"proj": "downsample.0", "bn": "downsample.1"}


def _dolg_to_tv(parts):
    if parts[0] == "stem" and len(parts) >= 3:
        return [{"conv": "conv1", "bn": "bn1"}.get(parts[1], "?")] + parts[2:]
    if len(parts) >= 4 and parts[0][:1] == "s" and parts[0][1:].isdigit() and parts[1][:1] == "b":
        layer = f"layer{int(parts[0][1:])}"
        blk = str(int(parts[1][1:]) - 1)
        if parts[2] == "f" and len(parts) >= 5 and parts[3] in _DOLG_F_TO_TV:
            return [layer, blk, _DOLG_F_TO_TV[parts[3]]] + parts[4:]
        if parts[2] in _DOLG_SC_TO_TV:
            return [layer, blk, _DOLG_SC_TO_TV[parts[2]]] + parts[3:]
    return None


def to_dolg_keys(sd):
    """torchvision trunk keys -> ResNet_DOLG keys (the inverse of the DOLG
    branch of to_torchvision_keys); used to load seeded weights into the
    reference's own R101 when generating the trunk fixture."""
    inv_f = {v: k for k, v in _DOLG_F_TO_TV.items()}
    out = collections.OrderedDict()
    for k, v in sd.items():
        parts = k.split(".")
        if parts[0] in ("conv1", "bn1"):
            nk = ["stem", {"conv1": "conv", "bn1": "bn"}[parts[0]]] + parts[1:]
        else:
            li, bi = int(parts[0][5:]), int(parts[1])
            head = [f"s{li}", f"b{bi + 1}"]
            if parts[2] == "downsample":
                nk = head + [{"0": "proj", "1": "bn"}[parts[3]]] + parts[4:]
            else:
                nk = head + ["f", inv_f[parts[2]]] + parts[3:]
        out[".".join(nk)] = v
    return out


def to_torchvision_keys(sd, prefix=""):
    """Map a reference checkpoint's trunk keys to torchvision keys.

    Accepts plain torchvision keys, networks-style ``backbone.block{1..5}.*``
    (e.g. ``globalmodel.backbone.block1.0.weight`` saved by the reference's
    load_checkpoint, utils/helpfunc.py:342-368), Table-1
    ``backbone.backbone.{0..7}.*`` keys and ResNet_DOLG keys
    (``stem.conv``, ``s3.b7.f.b_bn``, ``s1.b1.proj``; networks/backbone.py:218-345,
    whose bottlenecks carry the stride on the 1x1: build the trunk with
    stride_on="1x1").  Non-trunk keys are dropped."""
    out = collections.OrderedDict()
    for k, v in sd.items():
        if prefix and not k.startswith(prefix):
            continue
        k2 = k[len(prefix):]
        for lead in ("module.", "globalmodel.", "backbone.backbone.", "backbone."):
            if k2.startswith(lead):
                k2 = k2[len(lead):]
        parts = k2.split(".")
        dolg = _dolg_to_tv(parts)
        if dolg is not None:
            parts = dolg
        elif parts[0] == "block1" and len(parts) >= 3:
            parts = [{"0": "conv1", "1": "bn1"}.get(parts[1], "?")] + parts[2:]
        elif parts[0] in _BLOCK_TO_TV:
            parts = [_BLOCK_TO_TV[parts[0]]] + parts[1:]
        elif parts[0] in _SEQ_TO_TV:
            parts = [_SEQ_TO_TV[parts[0]]] + parts[1:]
        k2 = ".".join(parts)
        if k2.startswith(("conv1.", "bn1.", "layer1.", "layer2.", "layer3.", "layer4.")):
            out[k2] = v
    return out


def load_state_dict(path):
    """Load a LOCAL checkpoint without executing anything from the file."""
    if path.endswith(".safetensors"):
        from safetensors.torch import load_file
        return load_file(path)
    obj = torch.load(path, map_location="cpu", weights_only=True)
    for key in ("state_dict", "model"):
        if isinstance(obj, dict) and key in obj and isinstance(obj[key], dict):
            obj = obj[key]
    return obj


def fold_bn(conv_w, bn, eps=BN_EPS):
    """Eval-mode BN folded into the preceding bias-free conv.

    Returns (w [Cout,KH,KW,Cin] fp32 NHWC-ready, bias [Cout] fp32); the fold
    is computed in float64 then rounded once."""
    w = conv_w.double()
    g = bn["weight"].double()
    b = bn["bias"].double()
    m = bn["running_mean"].double()
    v = bn["running_var"].double()
    scale = g / torch.sqrt(v + eps)
    wf = (w * scale[:, None, None, None]).permute(0, 2, 3, 1).contiguous().float()
    bf = (b - m * scale).float()
    return wf, bf


# ---- DOLG head (networks/RetrievalNet.py:367-474, with_aspp=False) ----------
DOLG_HEAD_KEYS = tuple(f"localmodel.{k}" for k in (
    "conv1.weight", "conv1.bias", "bn.weight", "bn.bias", "bn.running_mean", "bn.running_var", "conv2.weight",
    "conv2.bias")) + ("fc_t.weight", "fc_t.bias", "fc.weight", "fc.bias")


def dolg_head_from_state_dict(sd, eps=BN_EPS):
    """The DOLG head of a reference checkpoint (keys localmodel.conv1.*,
    localmodel.bn.*, localmodel.conv2.*, fc_t.*, fc.*; a leading ``module.``
    is dropped; trunk and ArcFace keys are ignored) as fp32 tensors:

      conv1_w [1024,1,1,1024] NHWC-ready, conv1_b [1024]: SpatialAttention2d's
        conv1 with its eval-mode BN folded in, the conv's OWN bias included
        (b' = (b_conv - mean) * scale + beta; fold_bn assumes a bias-free
        conv), computed in float64 and rounded once;
      conv2_w [1024], conv2_b (python float); fc_t_w [1024,2048], fc_t_b;
      fc_w [512,2048], fc_b.

    ASPP weights (localmodel.aspp.*, with_aspp=True) raise ValueError: the
    dilated 3x3 branch is not implemented."""
    sd = {(k[len("module."):] if k.startswith("module.") else k): v for k, v in sd.items()}
    if any(k.startswith("localmodel.aspp.") for k in sd):
        raise ValueError("DOLG checkpoint has localmodel.aspp.* weights (with_aspp=True), which is not supported")
    missing = [k for k in DOLG_HEAD_KEYS if k not in sd]
    if missing:
        raise ValueError(f"DOLG head: missing keys {missing}")
    w1 = sd["localmodel.conv1.weight"]
    cout = w1.shape[0]
    if w1.dim() != 4 or tuple(w1.shape[2:]) != (1, 1):
        raise ValueError(f"localmodel.conv1.weight: expected [Cout,Cin,1,1], got {tuple(w1.shape)}")
    g, b = sd["localmodel.bn.weight"].double(), sd["localmodel.bn.bias"].double()
    m, v = sd["localmodel.bn.running_mean"].double(), sd["localmodel.bn.running_var"].double()
    scale = g / torch.sqrt(v + eps)
    wf = (w1.double() * scale[:, None, None, None]).permute(0, 2, 3, 1).contiguous().float()
    bf = ((sd["localmodel.conv1.bias"].double() - m) * scale + b).float()
    w2 = sd["localmodel.conv2.weight"]
    if w2.numel() != cout:
        raise ValueError(f"localmodel.conv2.weight: expected {cout} weights, got {tuple(w2.shape)}")
    return {"conv1_w": wf, "conv1_b": bf.contiguous(),
            "conv2_w": w2.reshape(cout).float().contiguous(), "conv2_b": float(sd["localmodel.conv2.bias"].reshape(())),
            "fc_t_w": sd["fc_t.weight"].float().contiguous(), "fc_t_b": sd["fc_t.bias"].float().contiguous(),
            "fc_w": sd["fc.weight"].float().contiguous(), "fc_b": sd["fc.bias"].float().contiguous()}


def synthetic_dolg_head(seed, c=1024, c4=2048, out_dim=512):
    """Seeded DOLG head weights under the reference's keys (DOLG_HEAD_KEYS):
    non-trivial BN statistics, a conv1 gain that makes the BN output O(1) on
    the seeded trunk's x3, and a conv2 scale (std 0.05, bias 0.1) that spreads
    the attention (0.34-0.62 on tests/golden/dolg.npz's inputs).  The fixture
    generator loads them into the
    reference's modules; the tests fold them (dolg_head_from_state_dict)."""
    rs = np.random.RandomState(seed)
    sd = collections.OrderedDict()
    sd["localmodel.conv1.weight"] = _t(rs.standard_normal((c, c, 1, 1)) * (4.0 / np.sqrt(c)))
    sd["localmodel.conv1.bias"] = _t(rs.standard_normal(c) * 0.1)
    sd["localmodel.bn.weight"] = _t(rs.uniform(0.5, 1.5, c))
    sd["localmodel.bn.bias"] = _t(rs.standard_normal(c) * 0.1)
    sd["localmodel.bn.running_mean"] = _t(rs.standard_normal(c) * 0.1)
    sd["localmodel.bn.running_var"] = _t(rs.uniform(0.5, 1.5, c))
    sd["localmodel.conv2.weight"] = _t(rs.standard_normal((1, c, 1, 1)) * 0.05)
    sd["localmodel.conv2.bias"] = _t(np.full(1, 0.1))
    sd["fc_t.weight"] = _t(rs.uniform(-1, 1, (c, c4)) / np.sqrt(c4))
    sd["fc_t.bias"] = _t(rs.uniform(-1, 1, c) / np.sqrt(c4))
    sd["fc.weight"] = _t(rs.uniform(-1, 1, (out_dim, 2 * c)) / np.sqrt(2 * c))
    sd["fc.bias"] = _t(rs.uniform(-1, 1, out_dim) / np.sqrt(2 * c))
    return sd


# ---- SOLAR head (networks/RetrievalNet.py:534-590) --------------------------
SOLAR_HEAD_KEYS = tuple(f"pooling.{n}.0.{k}" for n in "fg" for k in ("weight", "bias")) + \
    tuple(f"pooling.{n}.1.{k}" for n in "fg" for k in ("weight", "bias", "running_mean", "running_var")) + \
    ("pooling.h.weight", "pooling.h.bias", "pooling.v.weight", "pooling.v.bias", "whiten.weight", "whiten.bias")


def solar_head_from_state_dict(sd, eps=BN_EPS):
    """The SOLAR head of a reference checkpoint (keys pooling.{f,g}.0.* conv,
    pooling.{f,g}.1.* BN, pooling.h.*, pooling.v.*, whiten.*; a leading
    ``module.`` is dropped; trunk and ``classifier.*`` keys are ignored) as
    fp32 contiguous tensors:

      fgh_w [3c,1,1,Cin] NHWC-ready, fgh_b [3c]: the f, g and h 1x1 convs as
        one conv, rows [f | g | h]; f and g with their eval-mode BN folded in,
        the conv's OWN bias included (b' = (b_conv - mean) * scale + beta;
        fold_bn assumes a bias-free conv), computed in float64 and rounded
        once; their ReLU is not part of the conv (rr_soa_attention applies it);
      v_w [Cin,1,1,c] NHWC-ready, v_b [Cin]; whiten_w [2048,Cin], whiten_b."""
    sd = {(k[len("module."):] if k.startswith("module.") else k): v for k, v in sd.items()}
    missing = [k for k in SOLAR_HEAD_KEYS if k not in sd]
    if missing:
        raise ValueError(f"SOLAR head: missing keys {missing}")
    ws, bs = [], []
    for n in "fg":
        w = sd[f"pooling.{n}.0.weight"]
        if w.dim() != 4 or tuple(w.shape[2:]) != (1, 1):
            raise ValueError(f"pooling.{n}.0.weight: expected [c,Cin,1,1], got {tuple(w.shape)}")
        g, b = sd[f"pooling.{n}.1.weight"].double(), sd[f"pooling.{n}.1.bias"].double()
        m, v = sd[f"pooling.{n}.1.running_mean"].double(), sd[f"pooling.{n}.1.running_var"].double()
        scale = g / torch.sqrt(v + eps)
        ws.append((w.double() * scale[:, None, None, None]).float())
        bs.append(((sd[f"pooling.{n}.0.bias"].double() - m) * scale + b).float())
    wh, wv = sd["pooling.h.weight"], sd["pooling.v.weight"]
    if tuple(wh.shape) != tuple(ws[0].shape) or tuple(ws[1].shape) != tuple(ws[0].shape) or wv.dim() != 4 or \
            tuple(wv.shape) != (wh.shape[1], wh.shape[0], 1, 1):
        raise ValueError("SOLAR head: pooling.{f,g,h,v} conv shapes do not fit each other")
    ws.append(wh.float())
    bs.append(sd["pooling.h.bias"].float())
    ww = sd["whiten.weight"]
    return {"fgh_w": torch.cat(ws).permute(0, 2, 3, 1).contiguous(), "fgh_b": torch.cat(bs).contiguous(),
            "v_w": wv.float().permute(0, 2, 3, 1).contiguous(), "v_b": sd["pooling.v.bias"].float().contiguous(),
            "whiten_w": ww.float().reshape(ww.shape[0], -1).contiguous(),
            "whiten_b": sd["whiten.bias"].float().contiguous()}


def synthetic_solar_head(seed, cin=2048, k=2):
    """Seeded SOLAR head weights under the reference's keys (SOLAR_HEAD_KEYS):
    f and g conv gains that put the logits at 10-20 on post-ReLU unit-variance
    maps (attention row maxima 0.07-0.41 on tests/golden/solar.npz's head
    inputs, far from uniform), non-trivial BN statistics, and a NON-ZERO v: the
    reference initialises v to zero (:553), which would make the block a no-op.
    The fixture generator loads them into the reference's modules; the tests
    fold them (solar_head_from_state_dict)."""
    rs = np.random.RandomState(seed)
    c = cin // k
    sd = collections.OrderedDict()
    for n in "fg":
        sd[f"pooling.{n}.0.weight"] = _t(rs.standard_normal((c, cin, 1, 1)) * (2.0 / np.sqrt(cin)))
        sd[f"pooling.{n}.0.bias"] = _t(rs.standard_normal(c) * 0.1)
        sd[f"pooling.{n}.1.weight"] = _t(rs.uniform(0.5, 1.5, c))
        sd[f"pooling.{n}.1.bias"] = _t(rs.standard_normal(c) * 0.1)
        sd[f"pooling.{n}.1.running_mean"] = _t(rs.standard_normal(c) * 0.1)
        sd[f"pooling.{n}.1.running_var"] = _t(rs.uniform(0.5, 1.5, c))
    sd["pooling.h.weight"] = _t(rs.standard_normal((c, cin, 1, 1)) / np.sqrt(cin))
    sd["pooling.h.bias"] = _t(rs.standard_normal(c) * 0.1)
    sd["pooling.v.weight"] = _t(rs.standard_normal((cin, c, 1, 1)) / np.sqrt(c))
    sd["pooling.v.bias"] = _t(rs.standard_normal(cin) * 0.1)
    sd["whiten.weight"] = _t(rs.uniform(-1, 1, (2048, cin, 1, 1)) / np.sqrt(cin))
    sd["whiten.bias"] = _t(rs.uniform(-1, 1, 2048) / np.sqrt(cin))
    return sd


# ---- HOW head (models/how_vlad.py:107-199) ----------------------------------
HOW_HEAD_KEYS = ("local_proj.weight", "local_proj.bias", "pooling.centroids", "final_proj.weight", "final_proj.bias",
                 "classifier.weight", "classifier.bias")


def how_head_from_state_dict(sd):
    """The HOW head of a reference checkpoint (HOWModel's keys local_proj.*,
    pooling.centroids, pooling.weights for ASMK, final_proj.*, classifier.*,
    bare or under the wrapper's leading ``backbone.``, a ``module.`` before
    either dropped; trunk keys are ignored) as fp32 contiguous tensors:

      local_w [D,2048] (the 1x1 conv flattened), local_b [D], centroids [K,D],
      weights [K] (ASMK only: its presence says which pooling the head is),
      final_w [2048, K D or K], final_b, cls_w [classes,2048], cls_b."""
    flat = _flat_keys(sd)
    missing = [k for k in HOW_HEAD_KEYS if k not in flat]
    if missing:
        raise ValueError(f"HOW head: missing keys {missing}")
    lw, cent, fw, cw = (flat[k] for k in ("local_proj.weight", "pooling.centroids", "final_proj.weight",
                                          "classifier.weight"))
    if lw.dim() != 4 or tuple(lw.shape[2:]) != (1, 1):
        raise ValueError(f"local_proj.weight: expected [D,Cin,1,1], got {tuple(lw.shape)}")
    if cent.dim() != 2 or cent.shape[1] != lw.shape[0]:
        raise ValueError(f"pooling.centroids: expected [K,{lw.shape[0]}], got {tuple(cent.shape)}")
    asmk = "pooling.weights" in flat
    pooled = cent.shape[0] if asmk else cent.shape[0] * cent.shape[1]
    if fw.dim() != 2 or fw.shape[1] != pooled:
        raise ValueError(f"final_proj.weight: expected [out,{pooled}], got {tuple(fw.shape)}")
    if cw.dim() != 2 or cw.shape[1] != fw.shape[0]:
        raise ValueError(f"classifier.weight: expected [classes,{fw.shape[0]}], got {tuple(cw.shape)}")
    head = {"local_w": _f(lw.reshape(lw.shape[0], lw.shape[1])), "local_b": _f(flat["local_proj.bias"]),
            "centroids": _f(cent), "final_w": _f(fw), "final_b": _f(flat["final_proj.bias"]),
            "cls_w": _f(cw), "cls_b": _f(flat["classifier.bias"])}
    if asmk:
        if tuple(flat["pooling.weights"].shape) != (cent.shape[0],):
            raise ValueError(f"pooling.weights: expected [{cent.shape[0]}], got {tuple(flat['pooling.weights'].shape)}")
        head["weights"] = _f(flat["pooling.weights"])
    return head


def synthetic_how_head(seed, pooling, local_dim=128, num_clusters=64, num_classes=8):
    """Seeded HOW head weights under HOWModel's keys (HOW_HEAD_KEYS, plus
    pooling.weights for pooling == "asmk").  The centroids are unit-norm random
    directions, not the constructor's U(0,1) draws (:24-28): against unit-norm
    descriptors at alpha = 100 the U(0,1) table (norms of about 6.5, logits
    spread over tens of units) pushes the assignments towards one-hots (median
    top weight 0.97 on random rows, against 0.8 for unit-norm centroids), and
    only a soft assignment exercises the softmax; unit-norm centroids are also
    what centroids trained on unit-norm descriptors look like.  ASMK's weights are
    0.5 + U(0,1), not the constructor's ones (:73), so a wrong index shows."""
    if pooling not in ("vlad", "asmk"):
        raise ValueError(f"Unsupported pooling type: {pooling}")
    rs = np.random.RandomState(seed)
    pooled = num_clusters * local_dim if pooling == "vlad" else num_clusters
    sd = collections.OrderedDict()
    sd["local_proj.weight"] = _t(rs.standard_normal((local_dim, 2048, 1, 1)) / np.sqrt(2048))
    sd["local_proj.bias"] = _t(rs.standard_normal(local_dim) * 0.1)
    c = rs.standard_normal((num_clusters, local_dim))
    sd["pooling.centroids"] = _t(c / np.linalg.norm(c, axis=1, keepdims=True))
    if pooling == "asmk":
        sd["pooling.weights"] = _t(0.5 + rs.uniform(0, 1, num_clusters))
    s = 1.0 / np.sqrt(pooled)
    sd["final_proj.weight"] = _t(rs.uniform(-1, 1, (2048, pooled)) * s)
    sd["final_proj.bias"] = _t(rs.uniform(-1, 1, 2048) * s)
    sd["classifier.weight"] = _t(rs.uniform(-1, 1, (num_classes, 2048)) / np.sqrt(2048))
    sd["classifier.bias"] = _t(rs.uniform(-1, 1, num_classes) / np.sqrt(2048))
    return sd


# ---- SoSNet head (models/sosnet.py:95-183) ----------------------------------
SOS_ATT_KEYS = tuple(f"similarity_attention.attention_net.{i}.{k}" for i in (0, 2, 4) for k in ("weight", "bias"))
SOS_HEAD_KEYS = ("second_order_pool.proj.weight", "second_order_pool.proj.bias", "feature_proj.0.weight",
                 "feature_proj.0.bias", "feature_proj.3.weight", "feature_proj.3.bias", "classifier.weight",
                 "classifier.bias")
SOS_ATT_GAIN = 40.0  # synthetic_sos_head: the last attention layer's gain over PyTorch's default init


def sos_head_from_state_dict(sd):
    """The SoSNet head of a reference checkpoint (SoSNetModel's keys
    similarity_attention.attention_net.{0,2,4}.*, second_order_pool.proj.*,
    feature_proj.{0,3}.*, classifier.*, bare or under the wrapper's leading
    ``backbone.``, a ``module.`` before either dropped; trunk keys are ignored)
    as fp32 contiguous tensors:

      att_w1 [H,2048], att_b1, att_w2 [H/2,H], att_b2, att_w3 [H/2], att_b3 [1]
      (absent together: use_attention=False), proj_w [c,2048] (the 1x1 conv
      flattened), proj_b [c], fp0_w [F, c (c + 1) / 2], fp0_b, fp3_w [F,F],
      fp3_b, cls_w [classes,F], cls_b."""
    flat = _flat_keys(sd)
    missing = [k for k in SOS_HEAD_KEYS if k not in flat]
    have_att = [k for k in SOS_ATT_KEYS if k in flat]
    if have_att and len(have_att) != len(SOS_ATT_KEYS):
        missing += [k for k in SOS_ATT_KEYS if k not in flat]
    if missing:
        raise ValueError(f"SoSNet head: missing keys {missing}")
    pw, f0, f3, cw = (flat[k] for k in ("second_order_pool.proj.weight", "feature_proj.0.weight",
                                        "feature_proj.3.weight", "classifier.weight"))
    if pw.dim() != 4 or tuple(pw.shape[2:]) != (1, 1):
        raise ValueError(f"second_order_pool.proj.weight: expected [c,Cin,1,1], got {tuple(pw.shape)}")
    c = pw.shape[0]
    if f0.dim() != 2 or f0.shape[1] != c * (c + 1) // 2:
        raise ValueError(f"feature_proj.0.weight: expected [F,{c * (c + 1) // 2}], got {tuple(f0.shape)}")
    if tuple(f3.shape) != (f0.shape[0], f0.shape[0]):
        raise ValueError(f"feature_proj.3.weight: expected [{f0.shape[0]},{f0.shape[0]}], got {tuple(f3.shape)}")
    if cw.dim() != 2 or cw.shape[1] != f3.shape[0]:
        raise ValueError(f"classifier.weight: expected [classes,{f3.shape[0]}], got {tuple(cw.shape)}")
    head = {"proj_w": _f(pw.reshape(c, pw.shape[1])), "proj_b": _f(flat["second_order_pool.proj.bias"]),
            "fp0_w": _f(f0), "fp0_b": _f(flat["feature_proj.0.bias"]), "fp3_w": _f(f3),
            "fp3_b": _f(flat["feature_proj.3.bias"]), "cls_w": _f(cw), "cls_b": _f(flat["classifier.bias"])}
    if have_att:
        w1, w2, w3 = (flat[f"similarity_attention.attention_net.{i}.weight"] for i in (0, 2, 4))
        if w1.dim() != 2 or w1.shape[1] != pw.shape[1]:
            raise ValueError(f"similarity_attention.attention_net.0.weight: expected [H,{pw.shape[1]}], got "
                             f"{tuple(w1.shape)}")
        if w2.dim() != 2 or w2.shape[1] != w1.shape[0] or tuple(w3.shape) != (1, w2.shape[0]):
            raise ValueError("similarity_attention.attention_net: expected [H/2,H] and [1,H/2] after [H,Cin], got "
                             f"{tuple(w2.shape)} and {tuple(w3.shape)}")
        head.update(att_w1=_f(w1), att_b1=_f(flat[SOS_ATT_KEYS[1]]), att_w2=_f(w2), att_b2=_f(flat[SOS_ATT_KEYS[3]]),
                    att_w3=_f(w3.reshape(-1)), att_b3=_f(flat[SOS_ATT_KEYS[5]].reshape(1)))
    return head


def synthetic_sos_head(seed, second_order_dim=512, num_classes=8, use_attention=True, feature_dim=2048):
    """Seeded SoSNet head weights under SoSNetModel's keys (SOS_ATT_KEYS with
    use_attention, SOS_HEAD_KEYS), each Linear / Conv2d drawn as PyTorch's
    default init, U(+-1 / sqrt(fan_in)) — except the last attention layer,
    whose weights are drawn SOS_ATT_GAIN = 40 times wider and shifted to sum
    to zero (its bias is not widened): with the default init a_p stays within
    0.45-0.55 on post-ReLU maps, a constant a cancels in the L2 of the pooled
    vector, and a head that ignored the attention would pass every test.  The
    hidden layer is non-negative, so weights that do not sum to zero push every
    logit one way (a within 0.0001-0.74 at one seed); zero-sum weights centre
    the logits and a spans [<= 0.2, >= 0.8] on a 7 x 7 map."""
    rs = np.random.RandomState(seed)
    sd = collections.OrderedDict()
    lin = functools.partial(_lin, rs, sd)
    c = second_order_dim
    if use_attention:
        lin("similarity_attention.attention_net.0", 512, 2048)
        lin("similarity_attention.attention_net.2", 256, 512)
        lin("similarity_attention.attention_net.4", 1, 256, gain=SOS_ATT_GAIN, zero_sum=True)
    lin("second_order_pool.proj", c, 2048, shape=(c, 2048, 1, 1))
    lin("feature_proj.0", feature_dim, c * (c + 1) // 2)
    lin("feature_proj.3", feature_dim, feature_dim)
    lin("classifier", num_classes, feature_dim)
    return sd


# ---- SpoC head (models/spoc.py:52-147) --------------------------------------
_CA = "contextual_attention."
SPOC_CTX_KEYS = tuple(f"{_CA}context_encoder.{i}.{k}" for i in (0, 3) for k in ("weight", "bias")) + \
    tuple(f"{_CA}context_encoder.{i}.{k}" for i in (1, 4) for k in _BN_KEYS) + \
    tuple(f"{_CA}{n}.{k}" for n in ("attention_conv", "feature_refine") for k in ("weight", "bias"))
SPOC_HEAD_KEYS = ("feature_aggregation.0.weight", "feature_aggregation.0.bias") + \
    tuple(f"feature_aggregation.1.{k}" for k in _BN_KEYS) + \
    ("feature_proj.0.weight", "feature_proj.0.bias", "feature_proj.3.weight", "feature_proj.3.bias",
     "classifier.weight", "classifier.bias")
SPOC_ATT_GAIN = 32.0  # synthetic_spoc_head: the attention conv's gain over PyTorch's default init


def _fold_bn_biased(w, conv_b, flat, bn, eps):
    """Eval-mode BN `bn`.* of flat folded into a conv / linear WITH its own
    bias: (w * scale per output row, (b_conv - mean) * scale + beta), in
    float64; fold_bn assumes a bias-free conv."""
    g, b, m, v = (flat[f"{bn}.{k}"].double() for k in _BN_KEYS)
    for k in _BN_KEYS:
        if tuple(flat[f"{bn}.{k}"].shape) != (w.shape[0],):
            raise ValueError(f"{bn}.{k}: expected [{w.shape[0]}], got {tuple(flat[f'{bn}.{k}'].shape)}")
    scale = g / torch.sqrt(v + eps)
    return w.double() * scale.reshape(-1, *([1] * (w.dim() - 1))), (conv_b.double() - m) * scale + b


def spoc_head_from_state_dict(sd, eps=BN_EPS):
    """The SpoC head of a reference checkpoint (SpoCModel's keys
    contextual_attention.context_encoder.{0,1,3,4}.*, .attention_conv.*,
    .feature_refine.*, feature_aggregation.{0,1}.*, feature_proj.{0,3}.*,
    classifier.*, bare or under the wrapper's leading ``backbone.``, a
    ``module.`` before either dropped; trunk keys are ignored) as fp32
    contiguous tensors, every BN folded in float64 WITH the conv's own bias
    and rounded once:

      ce0_w [Dc,3,3,Cin] and ce1_w [Dc,3,3,Dc] NHWC-ready, ce0_b, ce1_b [Dc];
      att_w [Dc], att_b (a python float); refine_wx [C,1,1,Cin] and refine_wc
      [C,Dc], feature_refine's weight split at column Cin, refine_b [C] (the
      contextual_attention keys absent together: use_context=False);
      agg_w [F,C], agg_b [F] (Conv1d(1) + BatchNorm1d); fp0_w [F,F], fp0_b,
      fp3_w [F,F], fp3_b; cls_w [classes,F], cls_b."""
    flat = _flat_keys(sd)
    missing = [k for k in SPOC_HEAD_KEYS if k not in flat]
    have_ctx = [k for k in SPOC_CTX_KEYS if k in flat]
    if have_ctx and len(have_ctx) != len(SPOC_CTX_KEYS):
        missing += [k for k in SPOC_CTX_KEYS if k not in flat]
    if missing:
        raise ValueError(f"SpoC head: missing keys {missing}")
    aw, f0, f3, cw = (flat[k] for k in ("feature_aggregation.0.weight", "feature_proj.0.weight",
                                        "feature_proj.3.weight", "classifier.weight"))
    if aw.dim() != 3 or aw.shape[2] != 1:
        raise ValueError(f"feature_aggregation.0.weight: expected [F,C,1], got {tuple(aw.shape)}")
    fd, c = aw.shape[0], aw.shape[1]
    if tuple(f0.shape) != (fd, fd):
        raise ValueError(f"feature_proj.0.weight: expected [{fd},{fd}], got {tuple(f0.shape)}")
    if tuple(f3.shape) != (fd, fd):
        raise ValueError(f"feature_proj.3.weight: expected [{fd},{fd}], got {tuple(f3.shape)}")
    if cw.dim() != 2 or cw.shape[1] != fd:
        raise ValueError(f"classifier.weight: expected [classes,{fd}], got {tuple(cw.shape)}")
    for k, n in (("feature_aggregation.0.bias", fd), ("feature_proj.0.bias", fd), ("feature_proj.3.bias", fd),
                 ("classifier.bias", cw.shape[0])):
        if tuple(flat[k].shape) != (n,):
            raise ValueError(f"{k}: expected [{n}], got {tuple(flat[k].shape)}")
    wa, ba = _fold_bn_biased(aw.reshape(fd, c), flat["feature_aggregation.0.bias"], flat, "feature_aggregation.1", eps)
    head = {"agg_w": _f(wa), "agg_b": _f(ba), "fp0_w": _f(f0), "fp0_b": _f(flat["feature_proj.0.bias"]),
            "fp3_w": _f(f3), "fp3_b": _f(flat["feature_proj.3.bias"]), "cls_w": _f(cw),
            "cls_b": _f(flat["classifier.bias"])}
    if have_ctx:
        enc = _CA + "context_encoder."
        w0, w1 = flat[enc + "0.weight"], flat[enc + "3.weight"]
        if w0.dim() != 4 or tuple(w0.shape[1:]) != (c, 3, 3):
            raise ValueError(f"{enc}0.weight: expected [Dc,{c},3,3], got {tuple(w0.shape)}")
        dc = w0.shape[0]
        if tuple(w1.shape) != (dc, dc, 3, 3):
            raise ValueError(f"{enc}3.weight: expected [{dc},{dc},3,3], got {tuple(w1.shape)}")
        wt, wr = flat[_CA + "attention_conv.weight"], flat[_CA + "feature_refine.weight"]
        if tuple(wt.shape) != (1, dc, 1, 1) or flat[_CA + "attention_conv.bias"].numel() != 1:
            raise ValueError(f"{_CA}attention_conv: expected weight [1,{dc},1,1] and bias [1], got {tuple(wt.shape)} "
                             f"and {tuple(flat[_CA + 'attention_conv.bias'].shape)}")
        if tuple(wr.shape) != (c, c + dc, 1, 1) or tuple(flat[_CA + "feature_refine.bias"].shape) != (c,):
            raise ValueError(f"{_CA}feature_refine: expected weight [{c},{c + dc},1,1] and bias [{c}], got "
                             f"{tuple(wr.shape)} and {tuple(flat[_CA + 'feature_refine.bias'].shape)}")
        for i in (0, 3):
            if tuple(flat[f"{enc}{i}.bias"].shape) != (dc,):
                raise ValueError(f"{enc}{i}.bias: expected [{dc}], got {tuple(flat[f'{enc}{i}.bias'].shape)}")
        wf0, bf0 = _fold_bn_biased(w0, flat[enc + "0.bias"], flat, enc + "1", eps)
        wf1, bf1 = _fold_bn_biased(w1, flat[enc + "3.bias"], flat, enc + "4", eps)
        wr2 = wr.reshape(c, c + dc)
        head.update(ce0_w=_f(wf0.permute(0, 2, 3, 1)), ce0_b=_f(bf0), ce1_w=_f(wf1.permute(0, 2, 3, 1)), ce1_b=_f(bf1),
                    att_w=_f(wt.reshape(dc)), att_b=float(flat[_CA + "attention_conv.bias"].reshape(())),
                    refine_wx=_f(wr2[:, :c]).reshape(c, 1, 1, c), refine_wc=_f(wr2[:, c:]),
                    refine_b=_f(flat[_CA + "feature_refine.bias"]))
    return head


def synthetic_spoc_head(seed, context_dim=512, num_classes=8, use_context=True, feature_dim=2048):
    """Seeded SpoC head weights under SpoCModel's keys (SPOC_CTX_KEYS with
    use_context, SPOC_HEAD_KEYS), each Conv / Linear drawn as PyTorch's default
    init, U(+-1 / sqrt(fan_in)) — except the attention conv, whose weights are
    drawn SPOC_ATT_GAIN times wider and shifted to sum to zero (its bias is not
    widened): ctx is post-ReLU, so this is synthetic_sos_head's problem and its
    cure — with the default init a stays near 0.5 and a head that ignored the
    gate would pass; weights that do not sum to zero push every logit one way.
    The logits' centre still moves with the seed (the channels' means differ),
    so a fixture picks a seed at which a spans [<= 0.2, >= 0.8] on its maps
    (tests/golden/make_golden_spoc.py asserts it).  The BatchNorms get
    non-trivial statistics (gamma and variance in U(0.5, 1.5), beta and mean
    N(0, 0.1)); the folded aggregation bias is then of the size of the
    pre-activations, and ReLU clips every region in some columns (an exact 0
    in agg, the pad-row trap of rr_linear_groupmax)."""
    rs = np.random.RandomState(seed)
    sd = collections.OrderedDict()
    c = 2048
    lin = functools.partial(_lin, rs, sd)

    def bn(key, n):
        sd[key + ".weight"] = _t(rs.uniform(0.5, 1.5, n))
        sd[key + ".bias"] = _t(rs.standard_normal(n) * 0.1)
        sd[key + ".running_mean"] = _t(rs.standard_normal(n) * 0.1)
        sd[key + ".running_var"] = _t(rs.uniform(0.5, 1.5, n))

    dc = context_dim
    if use_context:
        enc = _CA + "context_encoder."
        lin(enc + "0", dc, c * 9, shape=(dc, c, 3, 3))
        bn(enc + "1", dc)
        lin(enc + "3", dc, dc * 9, shape=(dc, dc, 3, 3))
        bn(enc + "4", dc)
        lin(_CA + "attention_conv", 1, dc, shape=(1, dc, 1, 1), gain=SPOC_ATT_GAIN, zero_sum=True)
        lin(_CA + "feature_refine", c, c + dc, shape=(c, c + dc, 1, 1))
    lin("feature_aggregation.0", feature_dim, c, shape=(feature_dim, c, 1))
    bn("feature_aggregation.1", feature_dim)
    lin("feature_proj.0", feature_dim, feature_dim)
    lin("feature_proj.3", feature_dim, feature_dim)
    lin("classifier", num_classes, feature_dim)
    return sd


# ---- token aggregator head (models/token_based.py:13-159) -------------------
# (networks.Token / token_head_from_state_dict below are the OTHER token model,
# networks/RetrievalNet.py's Token_Refine.)
_TA = "token_aggregator."
TOKAGG_LAYER_KEYS = ("self_attn.in_proj_weight", "self_attn.in_proj_bias", "self_attn.out_proj.weight",
                     "self_attn.out_proj.bias", "linear1.weight", "linear1.bias", "linear2.weight", "linear2.bias",
                     "norm1.weight", "norm1.bias", "norm2.weight", "norm2.bias")
_TOKAGG_LAYER_NAMES = ("qkv_w", "qkv_b", "out_w", "out_b", "l1_w", "l1_b", "l2_w", "l2_b", "n1_g", "n1_b", "n2_g",
                       "n2_b")
TOKAGG_PE_KEY = _TA + "pos_encoding.pe"  # optional: a buffer, recomputed when absent
TOKAGG_MAX_LEN = 196  # PositionalEncoding's max_len (:16): the model takes no more positions


def tokagg_head_keys(num_layers=2):
    keys = [_TA + "input_proj.weight", _TA + "input_proj.bias", _TA + "global_token"]
    keys += [f"{_TA}transformer.layers.{i}.{k}" for i in range(num_layers) for k in TOKAGG_LAYER_KEYS]
    return tuple(keys) + (_TA + "output_proj.weight", _TA + "output_proj.bias", "feature_proj.weight",
                          "feature_proj.bias", "classifier.weight", "classifier.bias")


TOKAGG_QK_GAIN = 3.5  # synthetic_tokagg_head: the gain of in_proj's q and k rows over PyTorch's default init


def tokagg_positional_encoding(d_model, max_len=TOKAGG_MAX_LEN):
    """PositionalEncoding's buffer (:19-25) as [max_len, d_model], in float32
    with the reference's own expression (the same bits as its registered pe)."""
    pe = torch.zeros(max_len, d_model)
    position = torch.arange(0, max_len, dtype=torch.float).unsqueeze(1)
    div_term = torch.exp(torch.arange(0, d_model, 2).float() * (-math.log(10000.0) / d_model))
    pe[:, 0::2] = torch.sin(position * div_term)
    pe[:, 1::2] = torch.cos(position * div_term)
    return pe


def tokagg_head_from_state_dict(sd):
    """The token aggregator's head of a reference checkpoint (TokenModel's keys
    token_aggregator.{input_proj.*, pos_encoding.pe, global_token,
    transformer.layers.{i}.*, output_proj.*}, feature_proj.*, classifier.*, bare
    or under the wrapper's leading ``backbone.``, a ``module.`` before either
    dropped; trunk keys are ignored) as fp32 contiguous tensors:

      in_w [d,Cin], in_b, pe [max_len,d] (computed when the buffer is absent),
      global_token [d], per layer i: l{i}_qkv_w [3d,d] (q | k | v), l{i}_qkv_b,
      l{i}_out_w [d,d], l{i}_out_b, l{i}_l1_w [f,d], l{i}_l1_b, l{i}_l2_w [d,f],
      l{i}_l2_b, l{i}_n1_g, l{i}_n1_b, l{i}_n2_g, l{i}_n2_b; op_w [Cin,d], op_b,
      fp_w [F,Cin], fp_b, cls_w [classes,F], cls_b.

    The layer count is the number of consecutive transformer.layers.{i} found."""
    flat = _flat_keys(sd)
    layers = 0
    while any(f"{_TA}transformer.layers.{layers}.{k}" in flat for k in TOKAGG_LAYER_KEYS):
        layers += 1
    missing = [k for k in tokagg_head_keys(max(layers, 1)) if k not in flat]
    if missing:
        raise ValueError(f"token aggregator head: missing keys {missing}")
    in_w, gt = flat[_TA + "input_proj.weight"], flat[_TA + "global_token"]
    if in_w.dim() != 2:
        raise ValueError(f"token_aggregator.input_proj.weight: expected [d,Cin], got {tuple(in_w.shape)}")
    d, cin = in_w.shape
    if gt.numel() != d:
        raise ValueError(f"token_aggregator.global_token: expected {d} values, got {tuple(gt.shape)}")
    head = {"in_w": _f(in_w), "in_b": _f(flat[_TA + "input_proj.bias"]), "global_token": _f(gt.reshape(d))}
    if TOKAGG_PE_KEY in flat:
        pe = flat[TOKAGG_PE_KEY]
        if pe.dim() != 3 or pe.shape[1] != 1 or pe.shape[2] != d:
            raise ValueError(f"token_aggregator.pos_encoding.pe: expected [max_len,1,{d}], got {tuple(pe.shape)}")
        head["pe"] = _f(pe.reshape(pe.shape[0], d))
    else:
        head["pe"] = tokagg_positional_encoding(d)
    for i in range(layers):
        pre = f"{_TA}transformer.layers.{i}."
        shapes = {"qkv_w": (3 * d, d), "qkv_b": (3 * d,), "out_w": (d, d), "out_b": (d,), "l1_b": None, "l2_b": (d,),
                  "n1_g": (d,), "n1_b": (d,), "n2_g": (d,), "n2_b": (d,)}
        ffn = flat[pre + "linear1.weight"].shape[0]
        shapes.update(l1_w=(ffn, d), l1_b=(ffn,), l2_w=(d, ffn))
        for key, name in zip(TOKAGG_LAYER_KEYS, _TOKAGG_LAYER_NAMES):
            t = flat[pre + key]
            if tuple(t.shape) != shapes[name]:
                raise ValueError(f"{pre + key}: expected {list(shapes[name])}, got {tuple(t.shape)}")
            head[f"l{i}_{name}"] = _f(t)
    ow, fw, cw = flat[_TA + "output_proj.weight"], flat["feature_proj.weight"], flat["classifier.weight"]
    if ow.dim() != 2 or ow.shape[1] != d or ow.shape[0] != cin:
        raise ValueError(f"token_aggregator.output_proj.weight: expected [{cin},{d}], got {tuple(ow.shape)}")
    if fw.dim() != 2 or fw.shape[1] != cin:
        raise ValueError(f"feature_proj.weight: expected [F,{cin}], got {tuple(fw.shape)}")
    if cw.dim() != 2 or cw.shape[1] != fw.shape[0]:
        raise ValueError(f"classifier.weight: expected [classes,{fw.shape[0]}], got {tuple(cw.shape)}")
    head.update(op_w=_f(ow), op_b=_f(flat[_TA + "output_proj.bias"]), fp_w=_f(fw), fp_b=_f(flat["feature_proj.bias"]),
                cls_w=_f(cw), cls_b=_f(flat["classifier.bias"]))
    return head


def tokagg_num_layers(head):
    n = 0
    while f"l{n}_qkv_w" in head:
        n += 1
    return n


def tokagg_layer(head, i):
    """Layer i of a tokagg_head_from_state_dict head, keyed without the l{i}_ lead."""
    return {name: head[f"l{i}_{name}"] for name in _TOKAGG_LAYER_NAMES}


def tokagg_fold_last_layer(layer, heads, dtype=torch.float32):
    """The last encoder layer's attention folded for the global token alone
    ("The token aggregator"): layer holds qkv_w [3d,d], qkv_b, out_w
    [d,d], out_b; with e = d / heads and W_h the head's e rows,

      A  = [Wk_h^T Wq_h / sqrt(e)]_h   [heads d, d]    a0 = [Wk_h^T bq_h / sqrt(e)]_h
      M  = [Wo[:, h] Wv_h]_h           [d, heads d]    m0 = Wo bv + bo

    so q~ = A x0 + a0, p_h = softmax_j(q~_h . x_j), and the attention block's
    output is M [sum_j p_hj x_j]_h + m0.  The key bias is never read (it shifts
    a head's scores alike).  Products in float64 on the host, stored as fp32
    (dtype: tests ask for the float64 products)."""
    w, b = layer["qkv_w"].double(), layer["qkv_b"].double()
    wo, bo = layer["out_w"].double(), layer["out_b"].double()
    d = w.shape[1]
    if d % heads:
        raise ValueError(f"tokagg_fold_last_layer: {heads} heads do not divide width {d}")
    e = d // heads
    wq, wk, wv = w[:d].view(heads, e, d), w[d:2 * d].view(heads, e, d), w[2 * d:].view(heads, e, d)
    bq, bv = b[:d].view(heads, e), b[2 * d:]
    s = 1.0 / math.sqrt(e)
    a = torch.bmm(wk.transpose(1, 2), wq) * s                      # [heads, d, d]
    a0 = torch.bmm(wk.transpose(1, 2), bq.unsqueeze(2)).squeeze(2) * s
    m = torch.bmm(wo.view(d, heads, e).permute(1, 0, 2), wv)       # [heads, d, d]: Wo[:, h] Wv_h
    m0 = wo @ bv + bo
    out = lambda v: v.to(dtype).contiguous()  # noqa: E731
    return (out(a.reshape(heads * d, d)), out(a0.reshape(heads * d)), out(m.permute(1, 0, 2).reshape(d, heads * d)),
            out(m0))


def synthetic_tokagg_head(seed, hidden_dim=512, num_heads=8, num_layers=2, num_classes=8, feature_dim=2048,
                          in_dim=2048, qk_gain=TOKAGG_QK_GAIN):
    """Seeded token-aggregator weights under TokenModel's keys
    (tokagg_head_keys), drawn as PyTorch's default initialisers draw them:
    every Linear U(+-1 / sqrt(fan_in)) for weight and bias, in_proj_weight
    Xavier-uniform U(+-sqrt(6 / (4 d))), global_token N(0, 1).  Three
    departures, so that a wrong head cannot pass:
     - the q and k rows of in_proj_weight are drawn qk_gain = 3.5 times wider
       (scores grow with its square):
       with the default init the global token's attention is near-uniform
       (max_j p a few times 1 / N) and a head that averaged the rows would pass;
       with the gain most (image, head) pairs have 0.2 <= max_j p <= 0.99
       (asserted by tests/golden/make_golden_tokagg.py);
     - in_proj_bias and out_proj.bias, zero by default, are U(+-1 / sqrt(d)), so
       the folded biases a0 and m0 are exercised;
     - LayerNorm weights are 1 + 0.1 u and biases 0.1 u, u ~ U(-1, 1).
    num_heads only checks the width; the draw does not depend on it.  The pe
    buffer is not included (the loader computes it)."""
    if hidden_dim % num_heads:
        raise ValueError("synthetic_tokagg_head: num_heads must divide hidden_dim")
    rs = np.random.RandomState(seed)
    sd = collections.OrderedDict()
    d = hidden_dim
    lin = functools.partial(_lin, rs, sd)
    lin(_TA + "input_proj", d, in_dim)
    sd[_TA + "global_token"] = _t(rs.standard_normal((1, 1, d)))
    for i in range(num_layers):
        pre = f"{_TA}transformer.layers.{i}."
        w = rs.uniform(-1, 1, (3 * d, d)) * np.sqrt(6.0 / (4 * d))
        w[:2 * d] *= qk_gain
        sd[pre + "self_attn.in_proj_weight"] = _t(w)
        sd[pre + "self_attn.in_proj_bias"] = _t(rs.uniform(-1, 1, 3 * d) / np.sqrt(d))
        lin(pre + "self_attn.out_proj", d, d)
        lin(pre + "linear1", 4 * d, d)
        lin(pre + "linear2", d, 4 * d)
        for n in ("norm1", "norm2"):
            sd[pre + n + ".weight"] = _t(1 + 0.1 * rs.uniform(-1, 1, d))
            sd[pre + n + ".bias"] = _t(0.1 * rs.uniform(-1, 1, d))
    lin(_TA + "output_proj", in_dim, d)
    lin("feature_proj", feature_dim, in_dim)
    lin("classifier", num_classes, feature_dim)
    return sd


# ---- Token head (networks/RetrievalNet.py:94-187) ---------------------------
_WB = ("weight", "bias")
_ATT = tuple(f"{p}.{k}" for p in ("q", "k", "v", "proj") for k in _WB)


def _token_head_keys(decoders=2):
    ks = ["tr.query"]
    ks += [f"tr.token_norm.{i}.{k}" for i in (0, 1) for k in _WB]
    ks += [f"tr.encoder.0.attn.{k}" for k in _ATT]
    ks += [f"tr.encoder.0.bn.{k}" for k in _BN_KEYS] + [f"tr.encoder.0.mlp.{k}" for k in _WB]
    for i in range(decoders):
        d = f"tr.decoder.{i}."
        ks += [d + f"{a}.{k}" for a in ("self_attn", "cross_attn") for k in _ATT]
        ks += [d + f"{n}.{k}" for n in ("bn1", "bn2", "mlp.fc1", "mlp.fc2") for k in _WB]
    ks += [f"tr.conv.0.{k}" for k in _WB] + [f"tr.conv.1.{k}" for k in _BN_KEYS]
    ks += [f"tr.proj.0.{k}" for k in _WB] + [f"tr.proj.1.{k}" for k in _BN_KEYS]
    return tuple(ks)


TOKEN_HEAD_KEYS = _token_head_keys()


def token_head_from_state_dict(sd, eps=BN_EPS):
    """The Token_Refine head of a reference Token / RetrievalNet checkpoint
    (keys tr.*, TOKEN_HEAD_KEYS; a leading ``module.`` is dropped; trunk,
    ``classifier.*`` and ``num_batches_tracked`` keys are ignored) as fp32
    contiguous tensors.  Every fold is computed in float64 and rounded once.

      conv_w [mid,1,1,2048], conv_b: tr.conv with its BatchNorm2d folded, the
        conv's own bias included ((b - mean) s + beta, s = gamma / sqrt(var + eps));
      enc_qkv_w [3 mid,1,1,mid], enc_qkv_b: the encoder's q | k | v stacked;
      enc_proj_w [mid,1,1,mid], enc_proj_b;
      enc_mlp_w, enc_mlp_b: the encoder's BatchNorm1d (x s + t per channel)
        folded into its mlp: W o s on columns, b + W t;
      query [n_obj, mid];  tn_w [mid,mid], tn_b, tn_g, tn_beta: token_norm;
      dec_kv_w [4 mid,1,1,mid], dec_kv_b: the two decoders' cross-attention
        k1 | v1 | k2 | v2 stacked (both read the encoder output);
      per decoder i in (0, 1): d{i}_ln1_g/_b, d{i}_cq_w/_b, d{i}_cproj_w/_b,
        d{i}_fc1_w/_b [2 mid,mid], d{i}_fc2_w/_b [mid,2 mid], d{i}_ln2_g/_b,
        d{i}_sqkv_w [3 mid,mid] / _b (self-attention q | k | v), d{i}_sproj_w/_b;
      out_w [1024, n_obj mid], out_b: tr.proj with its BatchNorm1d folded."""
    sd = {(k[len("module."):] if k.startswith("module.") else k): v for k, v in sd.items()}
    missing = [k for k in TOKEN_HEAD_KEYS if k not in sd]
    if missing:
        raise ValueError(f"Token head: missing keys {missing}")
    d = lambda k: sd["tr." + k].double()  # noqa: E731
    cw = sd["tr.conv.0.weight"]
    if cw.dim() != 4 or tuple(cw.shape[2:]) != (1, 1):
        raise ValueError(f"tr.conv.0.weight: expected [mid,2048,1,1], got {tuple(cw.shape)}")
    mid, cin = cw.shape[0], cw.shape[1]
    qy = sd["tr.query"]
    if qy.dim() != 3 or qy.shape[0] != 1 or qy.shape[2] != mid:
        raise ValueError(f"tr.query: expected [1,n_obj,{mid}], got {tuple(qy.shape)}")
    n_obj = qy.shape[1]

    def shape(k, want):
        if tuple(sd["tr." + k].shape) != tuple(want):
            raise ValueError(f"tr.{k}: expected {list(want)}, got {list(sd['tr.' + k].shape)}")

    for a in ["encoder.0.attn"] + [f"decoder.{i}.{n}" for i in (0, 1) for n in ("self_attn", "cross_attn")]:
        for p in ("q", "k", "v", "proj"):
            shape(f"{a}.{p}.weight", (mid, mid))
            shape(f"{a}.{p}.bias", (mid,))
    shape("encoder.0.mlp.weight", (mid, mid))
    shape("token_norm.0.weight", (mid, mid))
    for i in (0, 1):
        shape(f"decoder.{i}.mlp.fc1.weight", (2 * mid, mid))
        shape(f"decoder.{i}.mlp.fc2.weight", (mid, 2 * mid))
    shape("proj.0.weight", (sd["tr.proj.0.weight"].shape[0], n_obj * mid))

    def bn(p):
        s = d(p + ".weight") / torch.sqrt(d(p + ".running_var") + eps)
        return s, d(p + ".bias") - d(p + ".running_mean") * s

    as_conv = lambda w: _f(w).reshape(w.shape[0], 1, 1, w.shape[1])  # noqa: E731
    cat = lambda ks: torch.cat([d(k) for k in ks])  # noqa: E731
    h = {}
    s, t = bn("conv.1")
    h["conv_w"] = _f((d("conv.0.weight") * s[:, None, None, None]).permute(0, 2, 3, 1))
    h["conv_b"] = _f(d("conv.0.bias") * s + t)
    e = "encoder.0."
    h["enc_qkv_w"] = as_conv(cat([e + f"attn.{p}.weight" for p in "qkv"]))
    h["enc_qkv_b"] = _f(cat([e + f"attn.{p}.bias" for p in "qkv"]))
    h["enc_proj_w"], h["enc_proj_b"] = as_conv(d(e + "attn.proj.weight")), _f(d(e + "attn.proj.bias"))
    s, t = bn(e + "bn")
    h["enc_mlp_w"] = as_conv(d(e + "mlp.weight") * s[None, :])
    h["enc_mlp_b"] = _f(d(e + "mlp.bias") + d(e + "mlp.weight") @ t)
    h["query"] = _f(qy[0])
    h["tn_w"], h["tn_b"] = _f(d("token_norm.0.weight")), _f(d("token_norm.0.bias"))
    h["tn_g"], h["tn_beta"] = _f(d("token_norm.1.weight")), _f(d("token_norm.1.bias"))
    kv = [f"decoder.{i}.cross_attn.{p}" for i in (0, 1) for p in "kv"]
    h["dec_kv_w"] = as_conv(cat([k + ".weight" for k in kv]))
    h["dec_kv_b"] = _f(cat([k + ".bias" for k in kv]))
    for i in (0, 1):
        p, o = f"decoder.{i}.", f"d{i}_"
        for src, dst in (("bn1", "ln1"), ("bn2", "ln2")):
            h[o + dst + "_g"], h[o + dst + "_b"] = _f(d(p + src + ".weight")), _f(d(p + src + ".bias"))
        for src, dst in (("cross_attn.q", "cq"), ("cross_attn.proj", "cproj"), ("mlp.fc1", "fc1"), ("mlp.fc2", "fc2"),
                         ("self_attn.proj", "sproj")):
            h[o + dst + "_w"], h[o + dst + "_b"] = _f(d(p + src + ".weight")), _f(d(p + src + ".bias"))
        h[o + "sqkv_w"] = _f(cat([p + f"self_attn.{n}.weight" for n in "qkv"]))
        h[o + "sqkv_b"] = _f(cat([p + f"self_attn.{n}.bias" for n in "qkv"]))
    s, t = bn("proj.1")
    h["out_w"] = _f(d("proj.0.weight") * s[:, None])
    h["out_b"] = _f(d("proj.0.bias") * s + t)
    return h


def synthetic_token_head(seed, mid_dim=1024, n_obj=4):
    """Seeded Token_Refine weights under the reference's keys (TOKEN_HEAD_KEYS):
    q / k gains that put the attention logits near 10 on post-ReLU unit-variance
    maps, an object query scaled so the slot softmax is neither uniform nor
    one-hot, non-trivial BatchNorm running statistics and LayerNorm gamma /
    beta, and NON-ZERO attention ``proj`` layers: the reference initialises them
    to zero (:108-109), which would make every attention a no-op.  The fixture
    generator loads them into the reference's modules; the tests fold them
    (token_head_from_state_dict)."""
    rs = np.random.RandomState(seed)
    m = mid_dim
    sd = collections.OrderedDict()

    def lin(key, out_dim, in_dim, gain=1.0, bias=0.1):
        sd[key + ".weight"] = _t(rs.standard_normal((out_dim, in_dim)) * (gain / np.sqrt(in_dim)))
        sd[key + ".bias"] = _t(rs.standard_normal(out_dim) * bias)

    def norm(key, dim, stats):
        sd[key + ".weight"] = _t(rs.uniform(0.5, 1.5, dim))
        sd[key + ".bias"] = _t(rs.standard_normal(dim) * 0.1)
        if stats:
            sd[key + ".running_mean"] = _t(rs.standard_normal(dim) * 0.1)
            sd[key + ".running_var"] = _t(rs.uniform(0.5, 1.5, dim))

    def attention(key, qk_gain):
        lin(key + ".q", m, m, qk_gain)
        lin(key + ".k", m, m, qk_gain)
        lin(key + ".v", m, m)
        lin(key + ".proj", m, m)

    sd["tr.query"] = _t(rs.standard_normal((1, n_obj, m)) * (2.0 / np.sqrt(m)))
    lin("tr.token_norm.0", m, m)
    norm("tr.token_norm.1", m, False)
    attention("tr.encoder.0.attn", 2.0)
    norm("tr.encoder.0.bn", m, True)
    lin("tr.encoder.0.mlp", m, m)
    for i in range(2):
        d = f"tr.decoder.{i}."
        attention(d + "self_attn", 2.0)
        attention(d + "cross_attn", 2.0)
        norm(d + "bn1", m, False)
        norm(d + "bn2", m, False)
        lin(d + "mlp.fc1", 2 * m, m)
        lin(d + "mlp.fc2", m, 2 * m)
    sd["tr.conv.0.weight"] = _t(rs.standard_normal((m, 2048, 1, 1)) / np.sqrt(2048))
    sd["tr.conv.0.bias"] = _t(rs.standard_normal(m) * 0.1)
    norm("tr.conv.1", m, True)
    lin("tr.proj.0", 1024, n_obj * m)
    norm("tr.proj.1", 1024, True)
    return sd


def folded_resnet(sd, arch):
    """torchvision-keyed trunk -> ordered list of folded (name, w, b, stride, pad)."""
    def bn(prefix):
        return {k: sd[f"{prefix}.{k}"] for k in _BN_KEYS}

    out = collections.OrderedDict()
    for conv, bnp, cout, cin, k in resnet_conv_specs(arch):
        w = sd[conv + ".weight"]
        if tuple(w.shape) != (cout, cin, k, k):
            raise ValueError(f"{conv}: expected {(cout, cin, k, k)}, got {tuple(w.shape)}")
        out[conv] = fold_bn(w, bn(bnp))
    return out


# ---- SE-ResNet trunk (models/senet_g2.py:12-129) ----------------------------
# SENet's conv / BN keys are torchvision's (downsample in layer1.0 included), so
# to_torchvision_keys and folded_resnet serve under the matching resnet name;
# each bottleneck adds se.fc.0.weight [c / r, c] and se.fc.2.weight [c, c / r].
SENET_TRUNKS = {"senet50": "resnet50", "senet101": "resnet101"}
SENET_SE_GAIN = 8.0  # synthetic_senet_state_dict: the SE weights' gain over N(0, 1 / fan_in)


def senet_block_names(arch):
    """(block prefix, output channels) of every SE bottleneck, in forward order."""
    if arch not in SENET_TRUNKS:
        raise ValueError(f"Unsupported backbone: {arch}")
    return [(b.prefix, b.cout) for b in trunk_blocks(SENET_TRUNKS[arch])]


def senet_check_reduction(reduction):
    """The hidden widths c // reduction of the four stages must suit rr_se_apply
    (cr % 4 == 0, 4 <= cr <= 512): reductions 4, 8, 16, 32 and 64 do."""
    if not isinstance(reduction, int) or isinstance(reduction, bool) or reduction < 1:
        raise ValueError(f"SENet: reduction must be a positive int, got {reduction!r}")
    for c in (256, 512, 1024, 2048):
        cr = c // reduction
        if c % reduction or cr % 4 or not 4 <= cr <= 512:
            raise ValueError(f"SENet: reduction {reduction} gives a hidden width of {c}/{reduction} at {c} channels; "
                             "rr_se_apply needs a multiple of 4 in 4..512")
    return reduction


def senet_se_from_state_dict(sd, arch, reduction=16):
    """The SE weights of a checkpoint (keys as to_torchvision_keys accepts the
    trunk's) -> {block prefix: (w1 [c / r, c], w2 [c, c / r])} fp32 contiguous;
    ValueError naming the key for a missing or mis-shaped weight."""
    senet_check_reduction(reduction)
    tv = to_torchvision_keys(sd)
    out = collections.OrderedDict()
    for p, c in senet_block_names(arch):
        ws = []
        for i, shape in (("0", (c // reduction, c)), ("2", (c, c // reduction))):
            k = f"{p}.se.fc.{i}.weight"
            if k not in tv:
                raise ValueError(f"SENet: missing key {k}")
            if tuple(tv[k].shape) != shape:
                raise ValueError(f"{k}: expected {shape}, got {tuple(tv[k].shape)}")
            ws.append(_f(tv[k]))
        out[p] = tuple(ws)
    return out


def synthetic_senet_state_dict(arch="senet50", seed=0, reduction=16):
    """synthetic_resnet_state_dict of the matching resnet plus, from a second
    stream seeded [seed, 1], every block's se.fc.0 / se.fc.2 weights drawn
    N(0, 1) * SENET_SE_GAIN / sqrt(fan_in).  With PyTorch's default init every
    gate sits within 0.49-0.51, and a gate computed from the wrong hidden
    column would pass any test; at gain 8 every block's gates span
    [<= 0.2, >= 0.8] on the trunk fixture's inputs (make_golden_senet.py
    asserts it) without saturating."""
    senet_check_reduction(reduction)
    blocks = senet_block_names(arch)
    sd = synthetic_resnet_state_dict(SENET_TRUNKS[arch], seed)
    rs = np.random.RandomState([seed, 1])
    for p, c in blocks:
        cr = c // reduction
        sd[f"{p}.se.fc.0.weight"] = _t(rs.standard_normal((cr, c)) * (SENET_SE_GAIN / np.sqrt(c)))
        sd[f"{p}.se.fc.2.weight"] = _t(rs.standard_normal((c, cr)) * (SENET_SE_GAIN / np.sqrt(cr)))
    return sd


SENET_G2_HEAD_KEYS = ("g2_pool.p", "g2_pool.alpha", "g2_pool.beta", "feature_proj.weight", "feature_proj.bias",
                      "classifier.weight", "classifier.bias")


def senet_g2_fold(proj_w, proj_b, alpha, beta):
    """G2+'s alpha * g + beta (models/senet_g2.py:151) folded into the
    projection that follows it: W (alpha g + beta 1) + b = (alpha W) g + (b +
    beta W 1).  Computed in float64 and rounded once -> (W' fp32, b' fp32)."""
    w = proj_w.double()
    return (w * float(alpha)).float().contiguous(), (proj_b.double() + float(beta) * w.sum(dim=1)).float().contiguous()


def senet_g2_head_from_state_dict(sd):
    """The SENet-G2+ head of a reference checkpoint (SENetG2Model's keys
    g2_pool.{p,alpha,beta}, feature_proj.*, classifier.*, bare or under the
    wrapper's leading ``backbone.``, a ``module.`` before either dropped;
    trunk keys are ignored): p, alpha, beta as python floats, proj_w [F,2048],
    proj_b, cls_w [classes,F], cls_b, and the folded proj_wf / proj_bf
    (senet_g2_fold) as fp32 contiguous tensors."""
    flat = _flat_keys(sd)
    missing = [k for k in SENET_G2_HEAD_KEYS if k not in flat]
    if missing:
        raise ValueError(f"SENet-G2+ head: missing keys {missing}")
    for k in SENET_G2_HEAD_KEYS[:3]:
        if flat[k].numel() != 1:
            raise ValueError(f"{k}: expected one element, got {tuple(flat[k].shape)}")
    p, alpha, beta = (float(flat[k].reshape(-1)[0]) for k in SENET_G2_HEAD_KEYS[:3])
    pw, cw = flat["feature_proj.weight"], flat["classifier.weight"]
    if pw.dim() != 2 or flat["feature_proj.bias"].numel() != pw.shape[0]:
        raise ValueError(f"feature_proj.weight: expected [F,C] with a bias [F], got {tuple(pw.shape)}")
    if cw.dim() != 2 or cw.shape[1] != pw.shape[0] or flat["classifier.bias"].numel() != cw.shape[0]:
        raise ValueError(f"classifier.weight: expected [classes,{pw.shape[0]}], got {tuple(cw.shape)}")
    wf, bf = senet_g2_fold(pw, flat["feature_proj.bias"], alpha, beta)
    return {"p": p, "alpha": alpha, "beta": beta, "proj_w": _f(pw), "proj_b": _f(flat["feature_proj.bias"]),
            "proj_wf": wf, "proj_bf": bf, "cls_w": _f(cw), "cls_b": _f(flat["classifier.bias"])}


def synthetic_senet_g2_head(seed, num_classes=8, feature_dim=2048, p=3.0, alpha=1.0, beta=0.0):
    """Seeded SENet-G2+ head weights under SENetG2Model's keys: the two Linears
    as PyTorch's default init, g2_pool's p / alpha / beta as given (the
    reference starts them at gem_p / 1 / 0)."""
    rs = np.random.RandomState(seed)
    sd = collections.OrderedDict()
    for k, v in (("p", p), ("alpha", alpha), ("beta", beta)):
        sd[f"g2_pool.{k}"] = torch.tensor([v], dtype=torch.float32)
    _lin(rs, sd, "feature_proj", feature_dim, 2048)
    _lin(rs, sd, "classifier", num_classes, feature_dim)
    return sd


def resnet_conv_flops(arch, h, w, stride_on="3x3"):
    """Algorithmic FLOPs (2*M*N*K) of every trunk conv for one h x w image,
    following the trunk's strides/pads (trunk_block_maps)."""
    flops = {"conv1": 2 * conv_out(h, 7, 2, 3) * conv_out(w, 7, 2, 3) * 64 * 7 * 7 * 3}
    for b, _, (H1, W1), (Ho, Wo) in trunk_block_maps(arch, h, w, stride_on):
        p = b.prefix
        if b.entry:
            flops[p + ".downsample.0"] = 2 * Ho * Wo * b.cout * b.inplanes
        flops[p + ".conv1"] = 2 * H1 * W1 * b.planes * b.inplanes
        flops[p + ".conv2"] = 2 * Ho * Wo * b.planes * b.planes * 9
        flops[p + ".conv3"] = 2 * Ho * Wo * b.cout * b.planes
    return flops


def resnet_conv_bytes(arch, h, w, batch, stride_on="3x3", weight_bytes=6, fused=False):
    """Algorithmic HBM bytes of every trunk conv launch for `batch` h x w
    images (the same layer walk as resnet_conv_flops): the fp32 NHWC input map
    read once (the stem's NHWC4 image: 4 channels), the fp32 output written
    once, the block's fp32 identity read once by the residual conv3, and the
    weights once per launch (`weight_bytes` per parameter: 6 = the split-bf16
    core's three bf16 planes, 4 = fp32 or the f16x2 core's two fp16 planes).
    fused (the f16x2 trunk, networks.ResNet): the stem writes only
    its max-pooled map (rr_stem_pool_h2), and a stage's first block computes
    conv3 and the downsample projection as one GEMM (rr_bottleneck_out_h2),
    which reads the block input at the sampled pixels and writes no projected
    identity (its bytes are split between the two names)."""
    H, Wd = conv_out(h, 7, 2, 3), conv_out(w, 7, 2, 3)
    if fused:
        H, Wd = conv_out(H, 3, 2, 1), conv_out(Wd, 3, 2, 1)
    by = {"conv1": batch * (h * w * 4 + H * Wd * 64) * 4 + 64 * 7 * 7 * 4 * weight_bytes}
    for b, (H, Wd), (H1, W1), (Ho, Wo) in trunk_block_maps(arch, h, w, stride_on):
        p, planes, inplanes = b.prefix, b.planes, b.inplanes
        x_in = H * Wd * inplanes
        wd_by = b.cout * inplanes * weight_bytes
        if b.entry and fused:
            by[p + ".downsample.0"] = batch * Ho * Wo * inplanes * 4 + wd_by
        elif b.entry:
            by[p + ".downsample.0"] = batch * (x_in + Ho * Wo * b.cout) * 4 + wd_by
        by[p + ".conv1"] = batch * (x_in + H1 * W1 * planes) * 4 + planes * inplanes * weight_bytes
        by[p + ".conv2"] = batch * (H1 * W1 * planes + Ho * Wo * planes) * 4 + planes * planes * 9 * weight_bytes
        n_res = 0 if (b.entry and fused) else 1  # the identity map read by the residual epilogue
        by[p + ".conv3"] = batch * (Ho * Wo * planes + (1 + n_res) * Ho * Wo * b.cout) * 4 + b.cout * planes * weight_bytes
    return by


def synthetic_vit_state_dict(width=768, layers=12, heads=12, patch=16, res=224, out_dim=512, seed=0):
    """Seeded CLIP-layout ViT weights (networks/model.py:206-243 key names)."""
    rs = np.random.RandomState(seed)
    sc = width ** -0.5
    sd = collections.OrderedDict()
    sd["conv1.weight"] = _t(rs.standard_normal((width, 3, patch, patch)) / np.sqrt(3 * patch * patch))
    sd["class_embedding"] = _t(rs.standard_normal(width) * sc)
    sd["positional_embedding"] = _t(rs.standard_normal(((res // patch) ** 2 + 1, width)) * sc)
    sd["ln_pre.weight"], sd["ln_pre.bias"] = _t(np.ones(width)), _t(np.zeros(width))
    for i in range(layers):
        p = f"transformer.resblocks.{i}."
        sd[p + "attn.in_proj_weight"] = _t(rs.standard_normal((3 * width, width)) * sc)
        sd[p + "attn.in_proj_bias"] = _t(np.zeros(3 * width))
        sd[p + "attn.out_proj.weight"] = _t(rs.standard_normal((width, width)) * sc)
        sd[p + "attn.out_proj.bias"] = _t(np.zeros(width))
        sd[p + "ln_1.weight"], sd[p + "ln_1.bias"] = _t(np.ones(width)), _t(np.zeros(width))
        sd[p + "mlp.c_fc.weight"] = _t(rs.standard_normal((4 * width, width)) * sc)
        sd[p + "mlp.c_fc.bias"] = _t(np.zeros(4 * width))
        sd[p + "mlp.c_proj.weight"] = _t(rs.standard_normal((width, 4 * width)) * (0.5 / np.sqrt(4 * width)))
        sd[p + "mlp.c_proj.bias"] = _t(np.zeros(width))
        sd[p + "ln_2.weight"], sd[p + "ln_2.bias"] = _t(np.ones(width)), _t(np.zeros(width))
    sd["ln_post.weight"], sd["ln_post.bias"] = _t(np.ones(width)), _t(np.zeros(width))
    sd["proj"] = _t(rs.standard_normal((width, out_dim)) * sc)
    return sd


def vit_flops(width=768, layers=12, heads=12, patch=16, res=224, out_dim=512):
    """Algorithmic FLOPs per image: (GEMM FLOPs, attention FLOPs)."""
    L = (res // patch) ** 2 + 1
    gemm = 2 * (L - 1) * width * 3 * patch * patch
    gemm += layers * 2 * L * width * (3 * width + width + 4 * width + 4 * width)
    gemm += 2 * width * out_dim
    attn = layers * heads * 2 * (2 * L * L * (width // heads))
    return gemm, attn
