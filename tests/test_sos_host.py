"""SoSNet without a GPU: the two new C-ABI entries, the head-weight loader, the
constructor's checks, and the torch restatements (tests/sos_ref.py) pinned to
the reference's own SoSNetModel / SimilarityAttention / SecondOrderPooling
output (tests/golden/sos.npz, make_golden_sos.py)."""
import collections
import ctypes
import inspect
import os
import sys

import numpy as np
import pytest
import torch

from research_image_retrieval_amd import _lib, models, ops
from research_image_retrieval_amd import weights as W

HERE = os.path.dirname(os.path.abspath(__file__))
GOLD = os.path.join(HERE, "golden")
sys.path.insert(0, GOLD)
sys.path.insert(0, HERE)
import inputs as I  # noqa: E402
import sos_ref  # noqa: E402

TAGS = ("b2_224", "b1_odd")
HEAD_CASES = ((2, 7, 7), (1, 5, 9), (1, 17, 19))
BAR = 1e-6
# each degenerate replacement of a piece of the head (sos_ref.head_forward's switches)
SWITCHES = ({"attend": False}, {"center": False}, {"order": "tril"}, {"order": "colmajor"}, {"unbiased": False},
            {"relu": False})


def _tag(b, h, w):
    return f"head_b{b}_{h}x{w}"


def _head_input(b, h, w):
    return torch.from_numpy(I.feature_map(12000 + h * w, b, 2048, h, w))


def _row_err(got, ref):
    got, ref = torch.as_tensor(got).double(), torch.as_tensor(ref).double()
    return ((got - ref).abs().amax(dim=-1) / ref.norm(dim=-1)).max().item()


@pytest.fixture(scope="module")
def fx():
    return np.load(os.path.join(GOLD, "sos.npz"))


@pytest.fixture(scope="module")
def head(fx):
    return W.sos_head_from_state_dict(W.synthetic_sos_head(int(fx["head_seed"]), int(fx["second_order_dim"]), 8))


@pytest.fixture(scope="module")
def refs(head):
    """The float64 and float32 literal restatements of every group-(b) case, computed once."""
    return {c: {dt: sos_ref.head_forward(_head_input(*c), head, dt) for dt in (torch.float64, torch.float32)}
            for c in HEAD_CASES}


def test_symbols_and_abi():
    L = ctypes.CDLL(_lib.LIB_PATH)
    for name in ("rr_sos_cov", "rr_linear_splitk"):
        assert hasattr(L, name) and name in _lib.SIGNATURES
    L = _lib.lib()
    assert L.rr_sos_cov(None, None, 1, 2, 32, None, 0, None, 0.0, None, None, None, None) == _lib.RR_EINVAL
    assert L.rr_linear_splitk(None, None, 1, 4, None, 1, None, None, 0, None, None) == _lib.RR_EINVAL


def test_fixture_is_smaller_than_the_how_fixture(fx):
    assert os.path.getsize(os.path.join(GOLD, "sos.npz")) < os.path.getsize(os.path.join(GOLD, "how.npz"))
    assert int(fx["second_order_dim"]) == 32


@pytest.mark.parametrize("case", HEAD_CASES)
def test_float32_restatement_reproduces_head_fixture(fx, refs, case):
    """Every stored array of the head group against the float32 literal
    restatement: max(1e-6, 4 x the float32-vs-float64 restatement error) of the
    row norm, the bar of the other heads' tests.  Both are printed."""
    tag = _tag(*case)
    r32, r64 = refs[case][torch.float32], refs[case][torch.float64]
    stored = {"out": "out"}
    if case == (1, 5, 9):
        stored.update(att="att", vhat="vhat", features="features")
    a = r64["att"]
    print(tag, "a in", float(a.min()), float(a.max()))
    assert float(a.min()) <= 0.2 and float(a.max()) >= 0.8
    for key, k in stored.items():
        ref = fx[f"{tag}_{key}"]
        assert ref.shape == tuple(r32[k].shape), key
        e, d = _row_err(r32[k], ref), _row_err(r32[k], r64[k])
        print(f"  {tag} {key}: vs reference {e:.3e} of the row norm; float32 vs float64 restatement {d:.3e}")
        assert e <= max(BAR, 4 * d), key
    assert fx[tag + "_out"].shape == (case[0], 2048)
    if case == (1, 5, 9):
        assert fx[tag + "_att"].shape == (1, 45) and fx[tag + "_vhat"].shape == (1, 528)


@pytest.mark.parametrize("tag", TAGS)
def test_restatement_reproduces_end_to_end_fixture(fx, head, tag):
    """Group (a), from the reference trunk's saved x4 (wiring)."""
    tr = np.load(os.path.join(GOLD, "resnet_dolg_v15.npz"))
    assert int(tr["weight_seed"]) == int(fx["weight_seed"])
    assert list(tr[tag + "_case"]) == list(fx[tag + "_case"])
    x4 = torch.from_numpy(tr[tag + "_x4"])
    r32, r64 = sos_ref.head_forward(x4, head, torch.float32), sos_ref.head_forward(x4, head, torch.float64)
    e, d = _row_err(r32["out"], fx[tag + "_out"]), _row_err(r32["out"], r64["out"])
    print(tag, "descriptor: vs reference", e, "; float32 vs float64 restatement", d)
    assert e <= max(BAR, 4 * d)


@pytest.mark.parametrize("case", HEAD_CASES)
def test_head_fixture_is_sensitive_to_every_piece(head, refs, case):
    """A condition on the fixture: each degenerate replacement (a = 1, no
    centring, lower-triangle or column-major packing, / N for / (N - 1), no ReLU
    in feature_proj) moves the float64 descriptor by at least 100 x the bar the
    restatement is held to on this case.

    / N for / (N - 1) is the exception, and no synthetic head can change that:
    it scales the whole packed vector by (N - 1) / N, which the F.normalize that
    follows removes exactly (measured: the descriptor moves by 4e-17).  That
    switch is held to the same 100 x bar on the array where the divisor shows,
    the un-normalised packed covariance that rr_sos_cov writes and
    tests/test_gpu_sos.py compares with float64."""
    r64, r32 = refs[case][torch.float64], refs[case][torch.float32]
    x = _head_input(*case)
    for sw in SWITCHES:
        key = "cov" if "unbiased" in sw else "out"
        bar = max(BAR, 4 * _row_err(r32[key], r64[key]))
        moved = _row_err(sos_ref.head_forward(x, head, torch.float64, **sw)[key], r64[key])
        print(_tag(*case), sw, "moves", key, "by", moved, "=", moved / bar, "x the bar", bar)
        assert moved >= 100 * bar, sw


@pytest.mark.parametrize("case", HEAD_CASES)
def test_rearranged_form_stays_within_the_bar(head, refs, case):
    """The three identities the kernels use (the projection of the RAW rows
    times a_p, no projection bias, the L2 applied after the first Linear), in
    float32, against the float64 literal form."""
    r64, r32 = refs[case][torch.float64], refs[case][torch.float32]
    x = _head_input(*case)
    g32, g64 = sos_ref.head_rearranged(x, head, torch.float32), sos_ref.head_rearranged(x, head, torch.float64)
    for key in ("att", "vhat", "hidden", "features", "out"):
        bar = max(BAR, 4 * _row_err(r32[key], r64[key]))
        e32, e64 = _row_err(g32[key], r64[key]), _row_err(g64[key], r64[key])
        print(f"{_tag(*case)} {key}: rearranged float32 {e32:.3e}, float64 {e64:.3e}; bar {bar:.3e}")
        assert e64 <= 1e-12 and e32 <= bar, key


@pytest.mark.parametrize("c", [32, 96, 512])
def test_triu_offset_formula(c):
    i = torch.triu_indices(c, c, offset=0)
    off = torch.tensor([sos_ref.triu_offset(int(a), int(b), c) for a, b in zip(i[0][::7], i[1][::7])])
    assert torch.equal(off, torch.arange(i.shape[1])[::7])
    assert sos_ref.triu_offset(c - 1, c - 1, c) == c * (c + 1) // 2 - 1
    m = torch.arange(c * c, dtype=torch.float64).reshape(1, c, c)
    p = sos_ref.pack(m)
    for a, b in ((0, 0), (0, c - 1), (1, 1), (c // 2, c // 2 + 3), (c - 1, c - 1)):
        assert float(p[0, sos_ref.triu_offset(a, b, c)]) == a * c + b


def _checkpoint(seed, lead, use_attention=True):
    """A reference-shaped checkpoint: index-named nn.Sequential trunk keys
    under `lead`backbone., head keys under `lead`."""
    tv = W.synthetic_resnet_state_dict("resnet50", seed)
    inv = {v: k for k, v in {"0": "conv1", "1": "bn1", "4": "layer1", "5": "layer2", "6": "layer3",
                             "7": "layer4"}.items()}
    sd = collections.OrderedDict()
    for k, v in tv.items():
        first, rest = k.split(".", 1)
        sd[f"{lead}backbone.{inv[first]}.{rest}"] = v
    for k, v in W.synthetic_sos_head(seed + 1, 64, 8, use_attention).items():
        sd[lead + k] = v
    return sd, tv


@pytest.mark.parametrize("use_attention", [True, False])
@pytest.mark.parametrize("lead", ["", "backbone.", "module.backbone."])
def test_head_from_state_dict_round_trips(lead, use_attention):
    sd, tv = _checkpoint(5, lead, use_attention)
    raw = W.synthetic_sos_head(6, 64, 8, use_attention)
    h = W.sos_head_from_state_dict(sd)
    assert all(v.dtype == torch.float32 and v.is_contiguous() for v in h.values())
    assert ("att_w1" in h) == use_attention == ("att_w3" in h)
    assert h["proj_w"].shape == (64, 2048)
    assert torch.equal(h["proj_w"], raw["second_order_pool.proj.weight"].reshape(64, 2048))
    assert torch.equal(h["proj_b"], raw["second_order_pool.proj.bias"])
    assert h["fp0_w"].shape == (2048, 64 * 65 // 2) and torch.equal(h["fp0_w"], raw["feature_proj.0.weight"])
    assert torch.equal(h["fp0_b"], raw["feature_proj.0.bias"])
    assert torch.equal(h["fp3_w"], raw["feature_proj.3.weight"]) and torch.equal(h["fp3_b"], raw["feature_proj.3.bias"])
    assert torch.equal(h["cls_w"], raw["classifier.weight"]) and torch.equal(h["cls_b"], raw["classifier.bias"])
    if use_attention:
        pre = "similarity_attention.attention_net."
        assert h["att_w1"].shape == (512, 2048) and torch.equal(h["att_w1"], raw[pre + "0.weight"])
        assert h["att_w2"].shape == (256, 512) and torch.equal(h["att_b2"], raw[pre + "2.bias"])
        assert h["att_w3"].shape == (256,) and torch.equal(h["att_w3"], raw[pre + "4.weight"].reshape(256))
        assert h["att_b3"].shape == (1,) and torch.equal(h["att_b3"], raw[pre + "4.bias"])
        # the last layer is drawn wide and zero-sum, not PyTorch's default +-1/16
        assert float(h["att_w3"].abs().max()) > 1.0 and abs(float(h["att_w3"].double().sum())) < 1e-3
    back = W.to_torchvision_keys(sd)
    assert set(back) == set(tv) and all(torch.equal(back[k], tv[k]) for k in tv)


def test_head_rejects_missing_keys_and_bad_shapes():
    sd = W.synthetic_sos_head(7, 32, 8)
    for k in W.SOS_HEAD_KEYS + W.SOS_ATT_KEYS[:1]:
        bad = dict(sd)
        bad.pop(k)
        with pytest.raises(ValueError, match=k.replace(".", r"\.")):
            W.sos_head_from_state_dict(bad)
    for k, shape in (("second_order_pool.proj.weight", (32, 2048)), ("feature_proj.0.weight", (2048, 500)),
                     ("feature_proj.3.weight", (2048, 1024)), ("classifier.weight", (8, 512)),
                     ("similarity_attention.attention_net.2.weight", (256, 500))):
        bad = dict(sd)
        bad[k] = torch.zeros(shape)
        with pytest.raises(ValueError, match=k.split(".")[0]):
            W.sos_head_from_state_dict(bad)


def test_constructor_order_and_argument_errors():
    names = list(inspect.signature(models.SoSNetModel.__init__).parameters)[1:]
    assert names == ["backbone", "pretrained", "num_classes", "feature_dim", "second_order_dim", "use_attention",
                     "state_dict", "seed", "device", "conv_math", "stride_on"]
    assert list(inspect.signature(models.SoSNetWrapper.__init__).parameters)[1:6] == [
        "num_classes", "backbone", "feature_dim", "second_order_dim", "use_attention"]
    assert inspect.signature(models.SoSNetModel.__init__).parameters["second_order_dim"].default == 512
    # argument errors come before any device work (this container has no device)
    with pytest.raises(ValueError, match="pretrained"):
        models.SoSNetModel(pretrained=True)
    with pytest.raises(ValueError, match="backbone"):
        models.get_sosnet_model(10, backbone="resnet18")
    for c in (2048, 16, 48, 544, 0):
        with pytest.raises(ValueError, match="second_order_dim"):
            models.get_sosnet_model(10, second_order_dim=c)
    with pytest.raises(ValueError, match="use_attention"):
        models.SoSNetModel(second_order_dim=32, use_attention=False, state_dict=W.synthetic_sos_head(3, 32, 8))


def test_ops_reject_bad_shapes_before_the_call():
    z = torch.zeros
    for bad_z in (z(1, 4, 48), z(1, 4, 544), z(1, 4, 16), z(4, 64), z(1, 1, 64), z(1, 1, 1, 64),
                  z(1, 4, 128)[:, :, ::2], z(1, 4, 64).double()):
        with pytest.raises((ValueError, TypeError)):
            ops.sos_cov(bad_z, None, None, 0.0)
    with pytest.raises(ValueError, match="NaN"):
        ops.sos_cov(z(2, 1, 64), None, None, 0.0)
    with pytest.raises(ValueError, match="dh"):
        ops.sos_cov(z(1, 4, 64), z(1, 4, 6), z(6), 0.0)
    with pytest.raises(ValueError, match="hid"):
        ops.sos_cov(z(1, 4, 64), z(1, 5, 8), z(8), 0.0)
    with pytest.raises(ValueError, match="ROCm"):   # a good shape reaches the device check, not the library
        ops.sos_cov(z(1, 2, 2, 64), z(1, 2, 2, 8), z(8), 0.0)
    with pytest.raises(ValueError, match="k % 4"):
        ops.linear_splitk(z(2, 6), z(3, 6), None)
    with pytest.raises(ValueError, match="row_scale"):
        ops.linear_splitk(z(2, 8), z(3, 8), None, row_scale=z(3))
    with pytest.raises(ValueError, match="bias"):
        ops.linear_splitk(z(2, 8), z(3, 8), z(2))
    with pytest.raises(ValueError, match="ROCm"):
        ops.linear_splitk(z(2, 8), z(3, 8), z(3), row_scale=z(2), act=1)


def test_registry_does_not_serve_sosnet_yet():
    assert not [k for k in models.MODEL_REGISTRY if k.startswith("sosnet")]
    assert "sosnet_r50" in models.OUT_OF_SCOPE and "sosnet_r101" in models.OUT_OF_SCOPE
    with pytest.raises(NotImplementedError):
        models.get_model("sosnet_r50", 10)
