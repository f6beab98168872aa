"""SpoC without a GPU: the new C-ABI entries, the head-weight loader and its BN
folds, the constructor's checks, and the torch restatement (tests/spoc_ref.py)
pinned to the reference's own SpoCModel / ContextualAttention /
SpatialPyramidPooling output (tests/golden/spoc.npz, make_golden_spoc.py).

Bars, as tests/test_gpu_spoc.py: kernel bar max(1e-6, 4 e32) of the row norm,
descriptor bar max(2e-6, 4 x the float32 restatement's distance from the
float64 one)."""
import collections
import ctypes
import inspect
import os
import sys

import numpy as np
import pytest
import torch
import torch.nn as nn
import torch.nn.functional as F

from research_image_retrieval_amd import _lib, models, ops
from research_image_retrieval_amd import weights as W

HERE = os.path.dirname(os.path.abspath(__file__))
GOLD = os.path.join(HERE, "golden")
sys.path.insert(0, GOLD)
sys.path.insert(0, HERE)
import inputs as I  # noqa: E402
import spoc_ref  # noqa: E402

TAGS = ("b2_224", "b1_odd")
HEAD_CASES = ((2, 7, 7), (1, 5, 9), (1, 17, 19), (1, 4, 4))
LEVELS = (1, 2, 4)
BAR = 1e-6
NEW_SYMBOLS = ("rr_spp_regions", "rr_spp_max", "rr_spoc_refine", "rr_linear_groupmax")


def _tag(b, h, w):
    return f"head_b{b}_{h}x{w}"


def _head_input(b, h, w):
    return torch.from_numpy(I.feature_map(13000 + h * w, b, 2048, h, w))


def _row_err(got, ref):
    got, ref = torch.as_tensor(got).double(), torch.as_tensor(ref).double()
    return ((got - ref).abs().amax(dim=-1) / ref.norm(dim=-1)).max().item()


@pytest.fixture(scope="module")
def fx():
    return np.load(os.path.join(GOLD, "spoc.npz"))


@pytest.fixture(scope="module")
def raw(fx):
    return W.synthetic_spoc_head(int(fx["head_seed"]), 512, 8)


@pytest.fixture(scope="module")
def head(raw):
    return W.spoc_head_from_state_dict(raw)


@pytest.fixture(scope="module")
def refs(head):
    """The float64 and float32 literal restatements of every group-(b) case, computed once."""
    torch.set_num_threads(min(16, os.cpu_count() or 1))
    return {c: {dt: spoc_ref.head_forward(_head_input(*c), head, dt) for dt in (torch.float64, torch.float32)}
            for c in HEAD_CASES}


def test_symbols_and_abi():
    L = ctypes.CDLL(_lib.LIB_PATH)
    for name in NEW_SYMBOLS:
        assert hasattr(L, name) and name in _lib.SIGNATURES
    L = _lib.lib()
    lv = (ctypes.c_int * 3)(1, 2, 4)
    assert L.rr_spp_max(None, None, 1, 7, 7, 4, ctypes.cast(lv, ctypes.c_void_p), 3, None, None) == _lib.RR_EINVAL
    assert L.rr_spoc_refine(None, None, None, 1, 4, 32, None, 0.0, None, None, None, None, None) == _lib.RR_EINVAL
    assert L.rr_linear_groupmax(None, None, 1, 1, 4, None, None, 1, 0, None, None) == _lib.RR_EINVAL


def test_fixture_is_small_and_holds_data_only(fx):
    assert os.path.getsize(os.path.join(GOLD, "spoc.npz")) < 400 * 1024
    assert list(fx["levels"]) == list(LEVELS)
    assert all(fx[k].dtype.kind in "fi" for k in fx.files)


def test_regions_follow_the_reference_windows():
    """R on five maps as the reference's module gives it, 54 as the maximum
    over 4..39, rr_spp_regions against the restatement, and both against
    F.max_pool2d's own output shape."""
    for (h, w), r in (((7, 7), 54), ((5, 9), 25), ((4, 4), 21), ((17, 19), 21), ((4, 7), 33)):
        assert spoc_ref.regions(h, w, LEVELS) == r == ops.spp_regions(h, w, LEVELS)
    most = 0
    for h in range(4, 40):
        for w in range(4, 40):
            r = spoc_ref.regions(h, w, LEVELS)
            most = max(most, r)
            assert r == ops.spp_regions(h, w, LEVELS)
            if (h + w) % 7 == 0:
                assert spoc_ref.spp(torch.zeros(1, 1, h, w), LEVELS).shape[2] == r
    assert most == 54
    for lv in ([1], [3], [2, 2], [1, 2, 3, 6]):
        assert ops.spp_regions(7, 9, lv) == spoc_ref.regions(7, 9, lv) == spoc_ref.spp(torch.zeros(1, 1, 7, 9), lv).shape[2]
    for h, w, lv in ((3, 7, LEVELS), (7, 3, LEVELS), (4, 4, [5]), (4, 4, [0])):
        with pytest.raises(ValueError):
            ops.spp_regions(h, w, lv)
    with pytest.raises(ValueError, match="stride should not be zero"):
        spoc_ref.regions(3, 7, LEVELS)
    with pytest.raises(ValueError):
        ops.spp_regions(7, 7, [])
    with pytest.raises(ValueError):
        ops.spp_regions(7, 7, [1] * 9)
    lv = (ctypes.c_int * 3)(1, 2, 4)
    assert _lib.lib().rr_spp_regions(7, 7, None, 3) == -1
    assert _lib.lib().rr_spp_regions(0, 7, ctypes.cast(lv, ctypes.c_void_p), 3) == -1


@pytest.mark.parametrize("case", HEAD_CASES)
def test_float32_restatement_reproduces_head_fixture(fx, refs, case):
    """The stored descriptor at the descriptor bar, every other stored array of
    the head group at the kernel bar, and pooled's stored slice by value."""
    tag = _tag(*case)
    r32, r64 = refs[case][torch.float32], refs[case][torch.float64]
    a = r64["att"]
    print(tag, "a in", float(a.min()), float(a.max()), "; agg columns exactly 0:", int((r64["agg"] == 0).sum()))
    assert float(a.min()) <= 0.2 and float(a.max()) >= 0.8
    d32 = (r32["out"].double() - r64["out"]).abs().max().item()
    err = np.abs(r32["out"].numpy() - fx[tag + "_out"]).max()
    print(f"  {tag} out: vs reference {err:.3e}; float32 vs float64 restatement {d32:.3e}")
    assert fx[tag + "_out"].shape == (case[0], 2048) and err <= max(2e-6, 4 * d32)
    if case == (1, 5, 9):
        for key in ("att", "agg", "features"):
            ref = fx[f"{tag}_{key}"]
            assert ref.shape == tuple(r32[key].shape), key
            e, d = _row_err(r32[key], ref), _row_err(r32[key], r64[key])
            print(f"  {tag} {key}: vs reference {e:.3e} of the row norm; float32 vs float64 restatement {d:.3e}")
            assert e <= max(BAR, 4 * d), key
        assert fx[tag + "_att"].shape == (1, 45) and fx[tag + "_pooled64"].shape == (1, 25, 64)
        # max-pooling selects: the restatement's pyramid on the reference's own refined map (stored beside the
        # slice) IS the reference's pooled, value for value; on its own refined map (BNs folded: other last bits)
        # it is within the kernel bar
        mine = spoc_ref.spp(torch.from_numpy(fx[tag + "_refined64"]).permute(0, 3, 1, 2), LEVELS).transpose(1, 2)
        assert np.array_equal(mine.numpy(), fx[tag + "_pooled64"])
        e = _row_err(r32["pooled"][:, :, :64], fx[tag + "_pooled64"])
        d = _row_err(r32["pooled"][:, :, :64], r64["pooled"][:, :, :64])
        print(f"  {tag} pooled[..., :64]: vs reference {e:.3e} of the row norm; float32 vs float64 restatement {d:.3e}")
        assert e <= max(BAR, 4 * d)
        assert bool((torch.from_numpy(fx[tag + "_agg"]) == 0).any())


@pytest.mark.parametrize("tag", TAGS)
def test_restatement_reproduces_end_to_end_fixture(fx, head, tag):
    """Group (a), from the reference trunk's saved x4 (wiring)."""
    tr = np.load(os.path.join(GOLD, "resnet_dolg_v15.npz"))
    assert int(tr["weight_seed"]) == int(fx["weight_seed"])
    assert list(tr[tag + "_case"]) == list(fx[tag + "_case"])
    x4 = torch.from_numpy(tr[tag + "_x4"])
    if tag == "b1_odd":
        assert tuple(x4.shape[2:]) == (4, 5)  # the smallest legal map
    r32, r64 = spoc_ref.head_forward(x4, head, torch.float32), spoc_ref.head_forward(x4, head, torch.float64)
    e = np.abs(r32["out"].numpy() - fx[tag + "_out"]).max()
    d = (r32["out"].double() - r64["out"]).abs().max().item()
    print(tag, "descriptor: vs reference", e, "; float32 vs float64 restatement", d)
    assert e <= max(2e-6, 4 * d)


def test_restatement_reproduces_the_no_context_fixture(fx):
    head = W.spoc_head_from_state_dict(W.synthetic_spoc_head(int(fx["head_seed"]), 512, 8, use_context=False))
    assert "ce0_w" not in head and "att_b" not in head
    x4 = _head_input(1, 5, 9)
    r32, r64 = spoc_ref.head_forward(x4, head, torch.float32), spoc_ref.head_forward(x4, head, torch.float64)
    e = np.abs(r32["out"].numpy() - fx["nocontext_b1_5x9_out"]).max()
    d = (r32["out"].double() - r64["out"]).abs().max().item()
    print("use_context=False descriptor: vs reference", e, "; float32 vs float64 restatement", d)
    assert e <= max(2e-6, 4 * d)
    assert torch.equal(r32["refined"], x4.permute(0, 2, 3, 1))


@pytest.mark.parametrize("case", [(2, 7, 7), (1, 5, 9)])
def test_head_fixture_is_sensitive_to_every_piece(raw, head, refs, case):
    """A condition on the fixture: each degenerate replacement moves the
    float64 descriptor by at least 100 x the descriptor bar of this case: a = 1;
    the context half of the refine dropped; each pyramid level dropped in turn;
    ceil-mode windows (on (1, 5, 9), where floor mode drops a row and a column);
    the BatchNorm1d left unfolded; the max over regions replaced by the mean;
    the aggregation's ReLU dropped; zero pad rows admitted to the max (on
    (1, 5, 9) as well: a pad row gives relu(bias), which wins only where every
    true region's product is negative under a positive bias; among 25 regions
    that happens in some columns, among the 54 of a 7 x 7 map in none — measured
    0.0 — so the 7 x 7 case cannot show it, and tests/test_gpu_spoc.py plants
    such a column in every kernel case)."""
    r64, r32 = refs[case][torch.float64], refs[case][torch.float32]
    x = _head_input(*case)
    bar = max(2e-6, 4 * (r32["out"].double() - r64["out"]).abs().max().item())
    unfolded = dict(head)
    unfolded["agg_w"] = raw["feature_aggregation.0.weight"].reshape(2048, 2048)
    unfolded["agg_b"] = raw["feature_aggregation.0.bias"]
    variants = [("a = 1", head, dict(gate=False)), ("no context half", head, dict(ctx_half=False)),
                ("BatchNorm1d unfolded", unfolded, {}), ("mean over regions", head, dict(agg="mean")),
                ("no ReLU", head, dict(relu=False))]
    variants += [(f"level {lv} dropped", head, dict(levels=[v for v in LEVELS if v != lv])) for lv in LEVELS]
    if case == (1, 5, 9):
        variants += [("ceil mode", head, dict(ceil_mode=True)), ("zero pad rows", head, dict(pad_rows=True))]
    for name, hd, kw in variants:
        moved = (spoc_ref.head_forward(x, hd, torch.float64, **kw)["out"] - r64["out"]).abs().max().item()
        print(_tag(*case), name, "moves the descriptor by", moved, "=", moved / bar, "x the bar", bar)
        assert moved >= 100 * bar, name


class _Unfolded(nn.Module):
    """The reference's module layout (models/spoc.py:61-74, :131-147) from plain torch.nn, BNs unfolded."""

    def __init__(self, dc, fd, classes):
        super().__init__()
        ca = nn.Module()
        ca.context_encoder = nn.Sequential(nn.Conv2d(2048, dc, 3, padding=1), nn.BatchNorm2d(dc), nn.ReLU(),
                                           nn.Conv2d(dc, dc, 3, padding=1), nn.BatchNorm2d(dc), nn.ReLU())
        ca.attention_conv = nn.Conv2d(dc, 1, 1)
        ca.feature_refine = nn.Conv2d(2048 + dc, 2048, 1)
        self.contextual_attention = ca
        self.feature_aggregation = nn.Sequential(nn.Conv1d(2048, fd, 1), nn.BatchNorm1d(fd), nn.ReLU(),
                                                 nn.AdaptiveMaxPool1d(1))
        self.feature_proj = nn.Sequential(nn.Linear(fd, fd), nn.ReLU(), nn.Dropout(0.5), nn.Linear(fd, fd))
        self.classifier = nn.Linear(fd, classes)

    def forward(self, x, levels):
        ca = self.contextual_attention
        ctx = ca.context_encoder(x)
        a = torch.sigmoid(ca.attention_conv(ctx))
        refined = ca.feature_refine(torch.cat([x * a, ctx], dim=1))
        agg = self.feature_aggregation(spoc_ref.spp(refined, levels)).squeeze(2)
        return a, refined, agg, F.normalize(self.feature_proj(agg), p=2, dim=1)


def test_folds_match_unfolded_modules_in_float64():
    """Non-trivial BN statistics and conv biases: the folded head through the
    restatement against eval-mode torch.nn modules on the raw state dict, both
    in float64 (the fold rounds each weight to float32 once: 6e-8 relative)."""
    dc, fd = 32, 64
    sd = W.synthetic_spoc_head(31, dc, 8, True, fd)
    for bn in ("contextual_attention.context_encoder.1", "contextual_attention.context_encoder.4",
               "feature_aggregation.1"):
        assert float(sd[bn + ".running_mean"].abs().max()) > 0.05 and float(sd[bn + ".bias"].abs().max()) > 0.05
        assert float((sd[bn + ".running_var"] - 1).abs().max()) > 0.2
    assert float(sd["contextual_attention.context_encoder.0.bias"].abs().max()) > 0
    net = _Unfolded(dc, fd, 8)
    missing, unexpected = net.load_state_dict(sd, strict=False)
    assert not unexpected and all(k.endswith("num_batches_tracked") for k in missing)
    net = net.double().eval()
    head = W.spoc_head_from_state_dict(sd)
    assert head["ce0_w"].shape == (dc, 3, 3, 2048) and head["ce1_w"].shape == (dc, 3, 3, dc)
    assert head["refine_wx"].shape == (2048, 1, 1, 2048) and head["refine_wc"].shape == (2048, dc)
    assert head["agg_w"].shape == (fd, 2048) and isinstance(head["att_b"], float)
    x = torch.from_numpy(I.feature_map(5, 2, 2048, 5, 6))
    with torch.no_grad():
        a, refined, agg, out = net(x.double(), [1, 2])
    got = spoc_ref.head_forward(x, head, torch.float64, levels=[1, 2])
    e = {"att": (got["att"] - a.reshape(2, 30)).abs().max().item(),
         "refined": _row_err(got["refined"], refined.permute(0, 2, 3, 1)), "agg": _row_err(got["agg"], agg),
         "out": (got["out"] - out).abs().max().item()}
    print("folded vs unfolded, float64:", e)
    assert all(v <= BAR for v in e.values()), e
    # fold_bn's bias-free form on the same conv would drop the conv's own bias
    wf, bf = W.fold_bn(sd["contextual_attention.context_encoder.0.weight"],
                       {k: sd[f"contextual_attention.context_encoder.1.{k}"]
                        for k in ("weight", "bias", "running_mean", "running_var")})
    assert torch.equal(wf, head["ce0_w"]) and not torch.allclose(bf, head["ce0_b"])


def _checkpoint(seed, lead, use_context=True):
    """A reference-shaped checkpoint: index-named nn.Sequential trunk keys
    under `lead`backbone., head keys under `lead`."""
    tv = W.synthetic_resnet_state_dict("resnet50", seed)
    inv = {"conv1": "0", "bn1": "1", "layer1": "4", "layer2": "5", "layer3": "6", "layer4": "7"}
    sd = collections.OrderedDict()
    for k, v in tv.items():
        first, rest = k.split(".", 1)
        sd[f"{lead}backbone.{inv[first]}.{rest}"] = v
    for k, v in W.synthetic_spoc_head(seed + 1, 32, 8, use_context, 64).items():
        sd[lead + k] = v
    return sd, tv


@pytest.mark.parametrize("use_context", [True, False])
@pytest.mark.parametrize("lead", ["", "backbone.", "module.backbone."])
def test_head_from_state_dict_round_trips(lead, use_context):
    sd, tv = _checkpoint(5, lead, use_context)
    raw = W.synthetic_spoc_head(6, 32, 8, use_context, 64)
    h = W.spoc_head_from_state_dict(sd)
    assert set(raw) == set(W.SPOC_HEAD_KEYS + (W.SPOC_CTX_KEYS if use_context else ()))
    assert all(v.dtype == torch.float32 and v.is_contiguous() for k, v in h.items() if k != "att_b")
    assert ("ce0_w" in h) == use_context == ("att_b" in h) == ("refine_wc" in h)
    assert torch.equal(h["fp0_w"], raw["feature_proj.0.weight"]) and torch.equal(h["fp3_b"], raw["feature_proj.3.bias"])
    assert torch.equal(h["cls_w"], raw["classifier.weight"]) and torch.equal(h["cls_b"], raw["classifier.bias"])
    assert h["agg_w"].shape == (64, 2048) and h["agg_b"].shape == (64,)
    if use_context:
        pre = "contextual_attention."
        wr = raw[pre + "feature_refine.weight"].reshape(2048, 2048 + 32)
        assert torch.equal(h["refine_wx"].reshape(2048, 2048), wr[:, :2048]) and torch.equal(h["refine_wc"], wr[:, 2048:])
        assert torch.equal(h["refine_b"], raw[pre + "feature_refine.bias"])
        assert torch.equal(h["att_w"], raw[pre + "attention_conv.weight"].reshape(32))
        assert h["att_b"] == float(raw[pre + "attention_conv.bias"][0])
        # the attention conv is drawn wide and zero-sum, not PyTorch's default +-1/sqrt(32)
        assert float(h["att_w"].abs().max()) > 1.0 and abs(float(h["att_w"].double().sum())) < 1e-3
    back = W.to_torchvision_keys(sd)
    assert set(back) == set(tv) and all(torch.equal(back[k], tv[k]) for k in tv)


def test_head_rejects_missing_keys_and_bad_shapes():
    sd = W.synthetic_spoc_head(7, 32, 8, True, 64)
    for k in W.SPOC_HEAD_KEYS + W.SPOC_CTX_KEYS[:1] + W.SPOC_CTX_KEYS[-1:]:
        bad = dict(sd)
        bad.pop(k)
        with pytest.raises(ValueError, match=k.replace(".", r"\.")):
            W.spoc_head_from_state_dict(bad)
    ca = "contextual_attention."
    for k, shape in ((ca + "context_encoder.0.weight", (32, 2048, 1, 1)), (ca + "context_encoder.3.weight", (32, 16, 3, 3)),
                     (ca + "context_encoder.1.running_var", (16,)), (ca + "context_encoder.3.bias", (16,)),
                     (ca + "attention_conv.weight", (1, 16, 1, 1)), (ca + "feature_refine.weight", (2048, 2048, 1, 1)),
                     (ca + "feature_refine.bias", (64,)), ("feature_aggregation.0.weight", (64, 2048)),
                     ("feature_aggregation.1.weight", (32,)), ("feature_aggregation.0.bias", (32,)),
                     ("feature_proj.0.weight", (64, 32)), ("feature_proj.3.weight", (32, 64)),
                     ("feature_proj.3.bias", (32,)), ("classifier.weight", (8, 32))):
        bad = dict(sd)
        bad[k] = torch.zeros(shape)
        with pytest.raises(ValueError, match=k.rsplit(".", 1)[0].replace(".", r"\.")):
            W.spoc_head_from_state_dict(bad)


def test_constructor_order_and_argument_errors():
    names = list(inspect.signature(models.SpoCModel.__init__).parameters)[1:]
    assert names == ["backbone", "pretrained", "num_classes", "feature_dim", "pyramid_levels", "context_dim",
                     "use_context", "state_dict", "seed", "device", "conv_math", "stride_on"]
    assert list(inspect.signature(models.SpoCWrapper.__init__).parameters)[1:7] == [
        "num_classes", "backbone", "feature_dim", "pyramid_levels", "context_dim", "use_context"]
    p = inspect.signature(models.SpoCModel.__init__).parameters
    assert p["context_dim"].default == 512 and list(p["pyramid_levels"].default) == [1, 2, 4]
    # argument errors come before any device work (this container has no device)
    with pytest.raises(ValueError, match="pretrained"):
        models.SpoCModel(pretrained=True)
    with pytest.raises(ValueError, match="backbone"):
        models.get_spoc_model(10, backbone="resnet18")
    for dc in (16, 48, 2080, 0):
        with pytest.raises(ValueError, match="context_dim"):
            models.get_spoc_model(10, context_dim=dc)
    for lv in ([], [1] * 9, [0, 1]):
        with pytest.raises(ValueError, match="pyramid_levels"):
            models.get_spoc_model(10, pyramid_levels=lv)
    small = W.synthetic_spoc_head(3, 32, 8, True, 64)
    with pytest.raises(ValueError, match="use_context"):
        models.SpoCModel(context_dim=32, feature_dim=64, use_context=False, state_dict=small)
    with pytest.raises(ValueError, match="feature_dim"):
        models.SpoCModel(context_dim=32, state_dict=small)
    with pytest.raises(ValueError, match="context_dim"):
        models.SpoCModel(context_dim=64, feature_dim=64, state_dict=small)


def test_ops_reject_bad_shapes_before_the_call():
    z = torch.zeros
    for bad in (z(1, 7, 7, 6), z(7, 7, 8), z(1, 7, 7, 16)[..., ::2], z(1, 7, 7, 8).double()):
        with pytest.raises((ValueError, TypeError)):
            ops.spp_max(bad, LEVELS)
    with pytest.raises(ValueError, match="stride should not be zero"):
        ops.spp_max(z(1, 3, 7, 8), LEVELS)
    with pytest.raises(ValueError, match="ROCm"):   # a good shape reaches the device check, not the library
        ops.spp_max(z(1, 4, 4, 8), LEVELS)
    good = dict(u=z(5, 8), ctx=z(5, 32), w_att=z(32), b_att=0.0, w_c=z(8, 32), bias=z(8))
    for kw in (dict(ctx=z(5, 48), w_att=z(48), w_c=z(8, 48)), dict(ctx=z(5, 2080), w_att=z(2080), w_c=z(8, 2080)),
               dict(u=z(5, 6), w_c=z(6, 32), bias=z(6)), dict(ctx=z(4, 32)), dict(w_att=z(16)), dict(w_c=z(32, 8)),
               dict(bias=z(4)), dict(out=z(5, 8)), dict(u=z(5, 16)[:, ::2])):
        with pytest.raises(ValueError):
            ops.spoc_refine(**{**good, **kw})
    with pytest.raises(ValueError, match="ROCm"):
        ops.spoc_refine(**good)
    for x, w, b, act in ((z(2, 65, 8), z(3, 8), None, 0), (z(2, 0, 8), z(3, 8), None, 0), (z(2, 4, 6), z(3, 6), None, 0),
                         (z(8, 8), z(3, 8), None, 0), (z(2, 4, 8), z(3, 4), None, 0), (z(2, 4, 8), z(3, 8), z(2), 0),
                         (z(2, 4, 8), z(3, 8), None, 2), (z(2, 4, 8), z(0, 8), None, 0)):
        with pytest.raises(ValueError):
            ops.linear_groupmax(x, w, b, act)
    with pytest.raises(ValueError, match="ROCm"):
        ops.linear_groupmax(z(2, 4, 8), z(3, 8), z(3), 1)


def test_registry_does_not_serve_spoc_yet():
    assert not [k for k in models.MODEL_REGISTRY if k.startswith("spoc")]
    assert "spoc_r50" in models.OUT_OF_SCOPE and "spoc_r101" in models.OUT_OF_SCOPE
    with pytest.raises(NotImplementedError):
        models.get_model("spoc_r50", 10)
