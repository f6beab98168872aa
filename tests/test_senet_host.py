"""SENet-G2+ without a GPU: the new C-ABI entries, the SE and head weight
loaders, the alpha / beta fold, the constructors' checks, and the torch
restatement (tests/senet_ref.py) pinned to the reference's own SENetG2Wrapper
output (tests/golden/senet_g2.npz, make_golden_senet.py).

Bars, as tests/test_gpu_spoc.py: descriptor bar max(2e-6, 4 x the float32
restatement's distance from the float64 one); gates within 1e-6 absolute."""
import collections
import ctypes
import os
import sys

import numpy as np
import pytest
import torch

from research_image_retrieval_amd import _lib, models, networks, ops
from research_image_retrieval_amd import weights as W

HERE = os.path.dirname(os.path.abspath(__file__))
GOLD = os.path.join(HERE, "golden")
sys.path.insert(0, GOLD)
sys.path.insert(0, HERE)
import inputs as I  # noqa: E402
import senet_ref  # noqa: E402

CASES = (("senet50", "b2_224"), ("senet50", "b1_odd"), ("senet101", "b1_odd"))
GATE_BLOCKS = ("layer1.0", "layer2.0", "layer4.2")
NEW_SYMBOLS = ("rr_se_squeeze", "rr_se_apply")


@pytest.fixture(scope="module")
def fx():
    return np.load(os.path.join(GOLD, "senet_g2.npz"))


@pytest.fixture(scope="module")
def head(fx):
    p, alpha, beta = (float(v) for v in fx["g2"])
    return W.senet_g2_head_from_state_dict(W.synthetic_senet_g2_head(int(fx["head_seed"]), int(fx["num_classes"]),
                                                                      int(fx["feature_dim"]), p, alpha, beta))


@pytest.fixture(scope="module")
def refs(fx, head):
    """The float64 and float32 restatements of every fixture case, computed once:
    {(arch, tag): {dtype: dict(x4, gates, pooled, features, out)}}."""
    torch.set_num_threads(min(16, os.cpu_count() or 1))
    got = {}
    folded = {}
    for arch, tag in CASES:
        if arch not in folded:
            folded[arch] = senet_ref.fold(W.synthetic_senet_state_dict(arch, int(fx["weight_seed"])), arch)
        seed, b, h, w = (int(v) for v in fx[f"{arch}_{tag}_case"])
        x = I.trunk_input(seed, b, h, w)
        got[(arch, tag)] = {}
        for dt in (torch.float64, torch.float32):
            gates = {}
            x4 = senet_ref.trunk_forward(x, folded[arch], dt, gates)
            got[(arch, tag)][dt] = dict(senet_ref.head_forward(x4, head, dt), x4=x4, gates=gates)
    return got


def test_symbols_and_abi():
    L = ctypes.CDLL(_lib.LIB_PATH)
    for name in NEW_SYMBOLS:
        assert hasattr(L, name) and name in _lib.SIGNATURES
    L = _lib.lib()
    assert L.rr_abi_version() == 9
    assert L.rr_se_squeeze(None, None, 1, 1, 256, None, None) == _lib.RR_EINVAL
    assert L.rr_se_apply(None, None, None, None, None, 1, 1, 256, 16, 1, None, None, None, None) == _lib.RR_EINVAL
    assert callable(ops.se_squeeze) and callable(ops.se_apply)


def test_fixture_is_small_and_holds_data_only(fx):
    assert os.path.getsize(os.path.join(GOLD, "senet_g2.npz")) < 400 * 1024
    assert all(fx[k].dtype.kind in "fi" for k in fx.files)
    assert int(fx["weight_seed"]) == I.TRUNK_WEIGHT_SEED
    assert [float(v) for v in fx["g2"]] != [3.0, 1.0, 0.0]
    assert fx["senet50_b1_odd_x4_64"].shape == (1, 4, 5, 64)


@pytest.mark.parametrize("arch,tag", CASES)
def test_restatement_reproduces_the_reference_descriptors(fx, refs, arch, tag):
    r64, r32 = refs[(arch, tag)][torch.float64], refs[(arch, tag)][torch.float32]
    stored = fx[f"{arch}_{tag}_out"]
    d32 = (r32["out"].double() - r64["out"]).abs().max().item()
    err = np.abs(r32["out"].numpy() - stored).max()
    e64 = np.abs(r64["out"].numpy() - stored).max()
    lo = max(float(g.min()) for g in r64["gates"].values())
    hi = min(float(g.max()) for g in r64["gates"].values())
    print(f"{arch} {tag}: float32 restatement vs reference {err:.3e}, float64 vs reference {e64:.3e}; float32 vs "
          f"float64 restatement {d32:.3e}; every block's gates span [<= {lo:.4f}, >= {hi:.4f}]")
    assert stored.shape == tuple(r32["out"].shape) == (int(fx[f"{arch}_{tag}_case"][1]), int(fx["feature_dim"]))
    assert np.allclose(np.linalg.norm(stored, axis=1), 1.0, atol=1e-5)
    assert lo <= 0.2 and hi >= 0.8
    assert err <= max(2e-6, 4 * d32)
    assert e64 <= max(2e-6, 4 * d32)


def test_restatement_reproduces_the_recorded_gates_and_maps(fx, refs, head):
    key = "senet50_b1_odd"
    r64, r32 = refs[("senet50", "b1_odd")][torch.float64], refs[("senet50", "b1_odd")][torch.float32]
    for name in GATE_BLOCKS:
        stored = fx[f"{key}_gate_{name}"]
        for dt, r in (("float64", r64), ("float32", r32)):
            e = np.abs(r["gates"][name].double().numpy() - stored).max()
            print(f"gate {name} {dt}: {e:.3e} absolute; stored range [{stored.min():.4f}, {stored.max():.4f}]")
            assert stored.shape == tuple(r["gates"][name].shape) and e <= 1e-6
    x4 = r64["x4"][:, :64].permute(0, 2, 3, 1)
    e = ((x4 - torch.from_numpy(fx[f"{key}_x4_64"]).double()).abs().amax(dim=-1) / x4.norm(dim=-1)).max().item()
    d = ((x4 - r32["x4"][:, :64].permute(0, 2, 3, 1).double()).abs().amax(dim=-1) / x4.norm(dim=-1)).max().item()
    print(f"x4[..., :64]: float64 restatement vs reference {e:.3e} of the row norm; float32 vs float64 {d:.3e}")
    assert e <= max(1e-6, 4 * d)
    g2 = head["alpha"] * r64["pooled"] + head["beta"]
    e = ((g2 - torch.from_numpy(fx[f"{key}_pooled"]).double()).abs().amax(dim=-1) / g2.norm(dim=-1)).max().item()
    d = ((r64["pooled"] - r32["pooled"].double()).abs().amax(dim=-1) / r64["pooled"].norm(dim=-1)).max().item()
    print(f"pooled: float64 restatement vs reference {e:.3e} of the row norm; float32 vs float64 {d:.3e}")
    assert e <= max(1e-6, 4 * d)


def test_block_forward_matches_its_parts():
    """block_forward's taps are consistent: the gate is the sigmoid of fc.2 on
    relu(fc.0 mean(conv3)), and out = relu(conv3 * gate + identity)."""
    sd = W.synthetic_senet_state_dict("senet50", 5)
    folded = senet_ref.fold(sd, "senet50")
    p, stride, bw = folded["blocks"][4]
    assert (p, stride) == ("layer2.1", 1) and "downsample" not in bw
    x = torch.from_numpy(I.feature_map(7, 2, 512, 9, 7))
    got = senet_ref.block_forward(x, bw, stride)
    assert got["mean"].shape == (2, 512) and got["hidden"].shape == (2, 32) and got["gate"].shape == (2, 512)
    assert torch.equal(got["mean"], got["conv3"].mean(dim=(2, 3)))
    ref = torch.relu(got["conv3"] * got["gate"][:, :, None, None] + x.double())
    assert torch.equal(got["out"], ref)
    assert float(got["conv3"].min()) < 0 < float(got["conv3"].max())  # signed: no clamp may serve
    p, stride, bw = folded["blocks"][3]
    assert (p, stride) == ("layer2.0", 2) and bw["downsample"][0].shape == (512, 1, 1, 256)
    assert senet_ref.block_forward(torch.from_numpy(I.feature_map(8, 1, 256, 9, 7)), bw, stride)["out"].shape == \
        (1, 512, 5, 4)


def _prefixed(sd, pre):
    return collections.OrderedDict((pre + k, v) for k, v in sd.items())


def test_loaders_accept_wrapper_model_and_module_keys():
    trunk = W.synthetic_senet_state_dict("senet50", 3)
    hd = W.synthetic_senet_g2_head(4, 8, 64, 2.5, 1.3, 0.07)
    model_sd = collections.OrderedDict(_prefixed(trunk, "backbone."), **hd)
    wrapper_sd = _prefixed(model_sd, "backbone.")
    module_sd = _prefixed(wrapper_sd, "module.")
    module_model_sd = _prefixed(model_sd, "module.")
    assert "backbone.backbone.layer1.0.se.fc.0.weight" in wrapper_sd and "backbone.g2_pool.alpha" in wrapper_sd
    se0 = W.senet_se_from_state_dict(trunk, "senet50")
    tv0 = W.to_torchvision_keys(trunk)
    h0 = W.senet_g2_head_from_state_dict(hd)
    assert len(se0) == 16 and se0["layer1.0"][0].shape == (16, 256) and se0["layer4.2"][1].shape == (2048, 128)
    assert h0["p"] == 2.5 and h0["alpha"] == float(np.float32(1.3)) and h0["beta"] == float(np.float32(0.07))
    for sd in (model_sd, wrapper_sd, module_sd, module_model_sd):
        se = W.senet_se_from_state_dict(sd, "senet50")
        assert list(se) == list(se0)
        assert all(torch.equal(a, b) for k in se for a, b in zip(se[k], se0[k]))
        tv = W.to_torchvision_keys(sd)
        assert list(tv) == list(tv0) and all(torch.equal(tv[k], tv0[k]) for k in tv)
        h = W.senet_g2_head_from_state_dict(sd)
        assert all(torch.equal(h[k], h0[k]) if torch.is_tensor(h[k]) else h[k] == h0[k] for k in h0)
    # folded_resnet takes the SE keys along without reading them
    assert "layer1.0.se.fc.0.weight" in tv0 and len(W.folded_resnet(tv0, "resnet50")) == 53


def test_loader_rejects_bad_se_weights():
    sd = W.synthetic_senet_state_dict("senet50", 3)
    bad = dict(sd)
    bad["layer2.1.se.fc.0.weight"] = sd["layer2.1.se.fc.0.weight"].t().contiguous()
    with pytest.raises(ValueError, match=r"layer2\.1\.se\.fc\.0\.weight"):
        W.senet_se_from_state_dict(bad, "senet50")
    bad = dict(sd)
    bad["layer3.0.se.fc.2.weight"] = sd["layer3.0.se.fc.2.weight"].t().contiguous()
    with pytest.raises(ValueError, match=r"layer3\.0\.se\.fc\.2\.weight"):
        W.senet_se_from_state_dict(bad, "senet50")
    bad = dict(sd)
    del bad["layer4.2.se.fc.2.weight"]
    with pytest.raises(ValueError, match=r"layer4\.2\.se\.fc\.2\.weight"):
        W.senet_se_from_state_dict(bad, "senet50")
    with pytest.raises(ValueError):  # a reduction-16 checkpoint read as reduction 8
        W.senet_se_from_state_dict(sd, "senet50", 8)
    hd = W.synthetic_senet_g2_head(4, 8, 64)
    del hd["g2_pool.beta"]
    with pytest.raises(ValueError, match="g2_pool.beta"):
        W.senet_g2_head_from_state_dict(hd)


def test_synthetic_se_weights_are_seeded_and_scaled():
    a, b = W.synthetic_senet_state_dict("senet50", 3), W.synthetic_senet_state_dict("senet50", 3)
    assert list(a) == list(b) and all(torch.equal(a[k], b[k]) for k in a)
    plain = W.synthetic_resnet_state_dict("resnet50", 3)
    assert all(torch.equal(a[k], plain[k]) for k in plain)  # the trunk's own stream is untouched
    assert W.SENET_SE_GAIN == 8.0
    w1, w2 = a["layer3.0.se.fc.0.weight"], a["layer3.0.se.fc.2.weight"]
    assert w1.shape == (64, 1024) and w2.shape == (1024, 64)
    assert abs(float(w1.std()) * np.sqrt(1024) / W.SENET_SE_GAIN - 1) < 0.05
    assert abs(float(w2.std()) * np.sqrt(64) / W.SENET_SE_GAIN - 1) < 0.05
    c = W.synthetic_senet_state_dict("senet50", 3, reduction=8)
    assert c["layer1.0.se.fc.0.weight"].shape == (32, 256)
    assert len([k for k in W.synthetic_senet_state_dict("senet101", 3) if k.endswith("se.fc.2.weight")]) == 33


def test_alpha_beta_fold_equals_the_unfolded_head():
    """(alpha W) g + (b + beta W 1) against W (alpha g + beta) + b in float64:
    1e-12 relative on the float64 fold, and the fp32 rounding of the folded
    tensors is one rounding of the exact values."""
    rs = np.random.RandomState(9)
    hd = W.senet_g2_head_from_state_dict(W.synthetic_senet_g2_head(4, 8, 96, 2.5, 1.3, 0.07))
    g = torch.from_numpy(np.abs(rs.standard_normal((5, 2048))))
    w, b = hd["proj_w"].double(), hd["proj_b"].double()
    unfolded = torch.nn.functional.linear(hd["alpha"] * g + hd["beta"], w, b)
    wf64, bf64 = w * hd["alpha"], b + hd["beta"] * w.sum(dim=1)
    folded = torch.nn.functional.linear(g, wf64, bf64)
    rel = ((folded - unfolded).abs().max() / unfolded.abs().max()).item()
    print(f"fold vs unfolded, float64: {rel:.3e} relative")
    assert rel <= 1e-12
    assert torch.equal(hd["proj_wf"], wf64.float()) and torch.equal(hd["proj_bf"], bf64.float())
    wf, bf = W.senet_g2_fold(hd["proj_w"], hd["proj_b"], 1.0, 0.0)
    assert torch.equal(wf, hd["proj_w"]) and torch.equal(bf, hd["proj_b"])


def test_constructor_checks_precede_device_work():
    with pytest.raises(ValueError, match="Unsupported backbone"):
        models.SENetG2Wrapper(8, backbone="senet34")
    with pytest.raises(ValueError, match="Unsupported backbone"):
        models.get_senet_g2_model(8, backbone="resnet50")
    with pytest.raises(ValueError, match="Unsupported backbone"):
        models.SENetG2Model(layers=[2, 2, 2, 2])
    with pytest.raises(ValueError, match="Unsupported backbone"):
        networks.SENet("senet34")
    for r in (0, 3, 128, 2.0):
        with pytest.raises(ValueError, match="reduction"):
            models.SENetG2Wrapper(8, backbone="senet50", reduction=r)
        with pytest.raises(ValueError, match="reduction"):
            networks.SENet("senet50", reduction=r)
    for r in (4, 8, 16, 32, 64):
        assert W.senet_check_reduction(r) == r
    with pytest.raises(ValueError, match="conv_math"):
        networks.SENet("senet50", conv_math="s3")
    with pytest.raises(ValueError, match="feature_dim"):
        models.SENetG2Model(feature_dim=64, state_dict=W.synthetic_senet_g2_head(4, 8, 96))
    assert not hasattr(networks.SENet, "plan")


def test_registry_does_not_serve_senet_g2_yet():
    for name in ("senet_g2_50", "senet_g2_101"):
        assert name in models.OUT_OF_SCOPE and name not in models.MODEL_REGISTRY
        with pytest.raises(NotImplementedError):
            models.get_model(name, 8)


def test_wrappers_check_arguments_before_the_c_call():
    y = torch.zeros(1, 2, 2, 128)
    with pytest.raises(ValueError, match="256"):
        ops.se_squeeze(y)
    with pytest.raises(ValueError):
        ops.se_squeeze(torch.zeros(1, 256))
    y = torch.zeros(1, 2, 2, 256)
    with pytest.raises(ValueError, match="c % 64"):
        ops.se_apply(torch.zeros(1, 2, 2, 96), torch.zeros(1, 8), torch.zeros(96, 8))
    for cr in (6, 516, 0):
        with pytest.raises(ValueError, match="cr"):
            ops.se_apply(y, torch.zeros(1, cr), torch.zeros(256, cr))
    with pytest.raises(ValueError, match="hidden"):
        ops.se_apply(y, torch.zeros(2, 16), torch.zeros(256, 16))
    with pytest.raises(ValueError, match="w2"):
        ops.se_apply(y, torch.zeros(1, 16), torch.zeros(16, 256))
    with pytest.raises(ValueError, match="identity"):
        ops.se_apply(y, torch.zeros(1, 16), torch.zeros(256, 16), identity=torch.zeros(1, 2, 2, 128))
    with pytest.raises(ValueError, match="out must be"):
        ops.se_apply(y, torch.zeros(1, 16), torch.zeros(256, 16), out=torch.zeros_like(y))
    with pytest.raises(ValueError, match="out_amax"):
        ops.se_apply(y, torch.zeros(1, 16), torch.zeros(256, 16), out_amax=torch.zeros(64))
    with pytest.raises(ValueError, match="ROCm device"):  # every check passed: only the device is missing
        ops.se_apply(y, torch.zeros(1, 16), torch.zeros(256, 16))
