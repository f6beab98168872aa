"""HOW without a GPU: the two new C-ABI entries, the registry, the head-weight
loader, and the torch restatement (tests/how_ref.py) pinned to the reference's
own HOWModel / VLADPooling / ASMKPooling output (tests/golden/how.npz,
make_golden_how.py)."""
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
import how_ref  # noqa: E402

TAGS = ("b2_224", "b1_odd")
HEAD_CASES = ((2, 7, 7), (1, 5, 9), (1, 17, 19))
POOLINGS = ("vlad", "asmk")
HOW_NAMES = ("how_vlad_r50", "how_vlad_r101", "how_asmk_r50", "how_asmk_r101")
BAR = 1e-6
# each degenerate replacement of a piece of the head (how_ref's switches)
SWITCHES = {"vlad": ({"hard": True}, {"subtract": False}, {"normalize": False}, {"alpha": 1.0}),
            "asmk": ({"mask": False}, {"ones": True})}


def _tag(b, h, w):
    return f"head_b{b}_{h}x{w}"


def _head_input(b, h, w):
    return torch.from_numpy(I.feature_map(11000 + h * w, b, 2048, h, w))


def _row_err(got, ref):
    got, ref = torch.as_tensor(got).double(), torch.as_tensor(ref).double()
    return ((got - ref).abs().amax(dim=-1) / ref.norm(dim=-1)).max().item()


@pytest.fixture(scope="module")
def fx():
    return np.load(os.path.join(GOLD, "how.npz"))


@pytest.fixture(scope="module")
def heads(fx):
    return {p: W.how_head_from_state_dict(W.synthetic_how_head(int(fx["head_seed"]), p)) for p in POOLINGS}


@pytest.fixture(scope="module")
def refs(heads):
    """The float64 and float32 restatements of every group-(b) case, computed once."""
    return {(p, c): {dt: how_ref.head_forward(_head_input(*c), heads[p], dt) for dt in (torch.float64, torch.float32)}
            for p in POOLINGS for c in HEAD_CASES}


def test_symbols_and_abi():
    L = ctypes.CDLL(_lib.LIB_PATH)
    for name in ("rr_how_vlad", "rr_how_asmk"):
        assert hasattr(L, name) and name in _lib.SIGNATURES
    L = _lib.lib()
    assert L.rr_how_vlad(None, None, 1, 1, 128, None, 64, 100.0, None, None) == _lib.RR_EINVAL
    assert L.rr_how_asmk(None, None, 1, 1, 128, None, None, 64, None, None) == _lib.RR_EINVAL


def test_registry_serves_the_how_family():
    for name in HOW_NAMES:
        assert name in models.MODEL_REGISTRY and name not in models.OUT_OF_SCOPE
    assert set(models.MODEL_REGISTRY) == {"gem_r50", "gem_r101"} | set(HOW_NAMES)
    assert len(models.OUT_OF_SCOPE) == 10 and not set(models.OUT_OF_SCOPE) & set(models.MODEL_REGISTRY)
    with pytest.raises(NotImplementedError):
        models.get_model("spoc_r50", 10)
    with pytest.raises(ValueError):
        models.get_model("how_vlad_r18", 10)
    # the reference's argument order first, the project's keywords after
    for cls in (models.HOWVLADWrapper, models.HOWASMKWrapper):
        assert list(inspect.signature(cls.__init__).parameters)[1:5] == ["num_classes", "backbone", "local_dim",
                                                                         "num_clusters"]
    names = list(inspect.signature(models.HOWModel.__init__).parameters)[1:]
    assert names == ["backbone", "pretrained", "num_classes", "local_dim", "pooling_type", "num_clusters", "state_dict",
                     "seed", "device", "conv_math", "stride_on"]
    assert inspect.signature(models.HOWModel.__init__).parameters["stride_on"].default == "3x3"
    # argument errors come before any device work
    with pytest.raises(ValueError, match="pretrained"):
        models.HOWModel(pretrained=True)
    with pytest.raises(ValueError, match="backbone"):
        models.get_how_vlad_model(10, backbone="resnet18")
    with pytest.raises(ValueError, match="pooling"):
        models.HOWModel(pooling_type="spoc")
    with pytest.raises(ValueError, match="local_dim"):
        models.get_how_asmk_model(10, local_dim=100)
    with pytest.raises(ValueError, match="num_clusters"):
        models.get_how_vlad_model(10, num_clusters=129)


def test_ops_reject_bad_shapes_before_the_call():
    z = torch.zeros
    for bad_x, bad_c in ((z(1, 4, 100), z(64, 100)), (z(1, 4, 288), z(64, 288)), (z(1, 4, 128), z(129, 128)),
                         (z(1, 4, 128), z(64, 64)), (z(4, 128), z(64, 128)), (z(1, 0, 128), z(64, 128)),
                         (z(1, 4, 256)[:, :, ::2], z(64, 128)), (z(1, 4, 128).double(), z(64, 128))):
        with pytest.raises((ValueError, TypeError)):
            ops.how_vlad(bad_x, bad_c)
        with pytest.raises((ValueError, TypeError)):
            ops.how_asmk(bad_x, bad_c, z(bad_c.shape[0]))
    with pytest.raises(ValueError, match="weights"):
        ops.how_asmk(z(1, 4, 128), z(64, 128), z(63))
    with pytest.raises(ValueError, match="65535"):
        ops.how_vlad(z(1, 65536, 32), z(4, 32))
    with pytest.raises(ValueError, match="ROCm"):   # a good shape reaches the device check, not the library
        ops.how_vlad(z(1, 2, 2, 128), z(64, 128))


def test_fixture_is_no_larger_than_the_trunk_fixture():
    assert os.path.getsize(os.path.join(GOLD, "how.npz")) <= os.path.getsize(os.path.join(GOLD, "resnet_dolg.npz"))


@pytest.mark.parametrize("pooling", POOLINGS)
@pytest.mark.parametrize("case", HEAD_CASES)
def test_float32_restatement_reproduces_head_fixture(fx, refs, pooling, case):
    """The float32 restatement against the reference's own float32 output at
    1e-6; the intermediates at 1e-6 of the row norm, or 4 x the float32-vs-
    float64 restatement difference on the same array where that is larger (as
    tests/test_token_host.py): it is for the assignment, whose logits are 100 x
    a distance and carry the descriptors' 1e-7 into the exponent as 1e-5.
    Both are printed.  ASMK's decisions exactly."""
    tag = f"{pooling}_{_tag(*case)}"
    r32, r64 = refs[pooling, case][torch.float32], refs[pooling, case][torch.float64]
    err = np.abs(r32["out"].numpy() - fx[tag + "_out"]).max()
    d = (r32["out"].double() - r64["out"]).abs().max().item()
    print(tag, "descriptor: float32 restatement vs reference", err, "; float32 vs float64 restatement", d)
    assert fx[tag + "_out"].shape == (case[0], 2048)
    assert err <= BAR
    if case == (1, 5, 9):
        stored = ("desc", "pooled", "features") + (("assign",) if pooling == "vlad" else ("mind", "thr"))
        for k in stored:
            ref = fx[f"{tag}_{k}"]
            assert ref.shape == tuple(r32[k].shape), k
            e, d = _row_err(r32[k], ref), _row_err(r32[k], r64[k])
            print(f"  {k}: vs reference {e:.3e} of the row norm; float32 vs float64 restatement {d:.3e}")
            assert e <= max(BAR, 4 * d), k
        if pooling == "asmk":
            assert np.array_equal(r32["nearest"].numpy(), fx[tag + "_nearest"])
            assert np.array_equal(r32["mask"].numpy(), fx[tag + "_mask"])
            assert np.array_equal(r64["nearest"].numpy(), fx[tag + "_nearest"])
            assert np.array_equal(r64["mask"].numpy(), fx[tag + "_mask"])
            assert 0 < int(fx[tag + "_mask"].sum()) < 45
        else:
            assert fx[tag + "_assign"].shape == (1, 45, 64) and fx[tag + "_pooled"].shape == (1, 8192)


@pytest.mark.parametrize("pooling", POOLINGS)
@pytest.mark.parametrize("tag", TAGS)
def test_restatement_reproduces_end_to_end_fixture(fx, heads, pooling, tag):
    """Group (a), from the reference trunk's saved x4 (wiring)."""
    tr = np.load(os.path.join(GOLD, "resnet_dolg_v15.npz"))
    assert int(tr["weight_seed"]) == int(fx["weight_seed"])
    assert list(tr[tag + "_case"]) == list(fx[f"{pooling}_{tag}_case"])
    got = how_ref.head_forward(torch.from_numpy(tr[tag + "_x4"]), heads[pooling], torch.float32)
    err = np.abs(got["out"].numpy() - fx[f"{pooling}_{tag}_out"]).max()
    print(pooling, tag, "descriptor err", err)
    assert err <= BAR


@pytest.mark.parametrize("pooling", POOLINGS)
@pytest.mark.parametrize("case", HEAD_CASES)
def test_head_fixture_is_sensitive_to_every_piece(heads, refs, pooling, case):
    """A condition on the fixture: each degenerate replacement (VLAD: a hard
    argmin for the softmax, sum a x^ without the centroid, no per-position
    normalisation, alpha = 1; ASMK: no threshold mask, all-ones weights) moves
    the float64 descriptor by at least 100 x the bar test_gpu_how.py holds the
    extractor to on this case, max(2e-6, 4 x the float32 restatement's
    distance from the float64 one)."""
    r64, r32 = refs[pooling, case][torch.float64], refs[pooling, case][torch.float32]
    bar = max(2e-6, 4 * (r32["out"].double() - r64["out"]).abs().max().item())
    x = _head_input(*case)
    for sw in SWITCHES[pooling]:
        moved = (how_ref.head_forward(x, heads[pooling], torch.float64, **sw)["out"] - r64["out"]).abs().max().item()
        print(pooling, _tag(*case), sw, "moves the descriptor by", moved, "=", moved / bar, "x the bar", bar)
        assert moved >= 100 * bar


@pytest.mark.parametrize("case", HEAD_CASES)
def test_vlad_assignment_is_soft_on_the_head_cases(refs, case):
    top = refs["vlad", case][torch.float64]["assign"].amax(dim=2).flatten()
    print(_tag(*case), "top assignment weight: median", top.median().item(), "min", top.min().item())
    assert top.median().item() < 0.95


def test_asmk_fixture_cases_are_decided_with_a_margin(heads):
    """The fixture's ASMK decisions are discrete: no position of a head case
    may sit within 1e-5 of a tie between two centroids or of the threshold."""
    for case in HEAD_CASES:
        y = how_ref.local_rows(_head_input(*case), heads["asmk"], torch.float64)
        am, tm = how_ref.margins(y, heads["asmk"]["centroids"])
        print(_tag(*case), "argmin margin", am.min().item(), "threshold margin", tm.min().item())
        assert am.min().item() >= 1e-5 and tm.min().item() >= 1e-5


def test_asmk_restatement_edge_cases():
    """n = 1 (the unbiased std of one value is NaN) and equal minima give zero
    rows; exact distance ties go to the lower index."""
    rs = np.random.RandomState(3)
    cent = torch.from_numpy(I.normed(rs, 8, 32))
    cent[5] = cent[2]
    wts = torch.arange(1.0, 9.0)
    one = how_ref.asmk(torch.from_numpy(rs.standard_normal((1, 1, 32)).astype(np.float32)), cent, wts)
    assert bool(torch.isnan(one["thr"]).all()) and float(one["asmk"].abs().max()) == 0.0
    same = how_ref.asmk(cent[2].repeat(1, 4, 1) * 3.0, cent, wts, torch.float32)
    assert int(same["nearest"][0, 0]) == 2 and float(same["asmk"].abs().max()) == 0.0
    x = torch.from_numpy(rs.standard_normal((1, 40, 32)).astype(np.float32))
    x[0, :6] = cent[2] * 2.0
    r = how_ref.asmk(x, cent, wts)
    assert bool((r["nearest"][0, :6] == 2).all()) and int(r["count"][0, 5]) == 0
    assert float(r["asmk"][0, 2]) == 3.0 * int(r["count"][0, 2]) and int(r["count"][0, 2]) >= 6


def _checkpoint(pooling, seed, lead):
    """A reference-shaped checkpoint: index-named nn.Sequential trunk keys
    under `lead`backbone., head keys under `lead`."""
    tv = W.synthetic_resnet_state_dict("resnet50", seed)
    inv = {v: k for k, v in {"0": "conv1", "1": "bn1", "4": "layer1", "5": "layer2", "6": "layer3",
                             "7": "layer4"}.items()}
    sd = collections.OrderedDict()
    for k, v in tv.items():
        first, rest = k.split(".", 1)
        sd[f"{lead}backbone.{inv[first]}.{rest}"] = v
    for k, v in W.synthetic_how_head(seed + 1, pooling, 64, 32).items():
        sd[lead + k] = v
    return sd, tv


@pytest.mark.parametrize("pooling", POOLINGS)
@pytest.mark.parametrize("lead", ["", "backbone.", "module.backbone."])
def test_head_from_state_dict_round_trips(pooling, lead):
    sd, tv = _checkpoint(pooling, 5, lead)
    raw = W.synthetic_how_head(6, pooling, 64, 32)
    h = W.how_head_from_state_dict(sd)
    assert all(v.dtype == torch.float32 and v.is_contiguous() for v in h.values())
    assert ("weights" in h) == (pooling == "asmk")
    assert h["local_w"].shape == (64, 2048) and torch.equal(h["local_w"], raw["local_proj.weight"].reshape(64, 2048))
    assert torch.equal(h["local_b"], raw["local_proj.bias"])
    assert h["centroids"].shape == (32, 64) and torch.equal(h["centroids"], raw["pooling.centroids"])
    assert h["final_w"].shape == (2048, 32 * 64 if pooling == "vlad" else 32)
    assert torch.equal(h["final_w"], raw["final_proj.weight"]) and torch.equal(h["final_b"], raw["final_proj.bias"])
    assert torch.equal(h["cls_w"], raw["classifier.weight"]) and torch.equal(h["cls_b"], raw["classifier.bias"])
    if pooling == "asmk":
        assert torch.equal(h["weights"], raw["pooling.weights"])
        assert float(h["weights"].min()) >= 0.5 and float(h["weights"].std()) > 0.1  # not the constructor's ones
    assert float((h["centroids"].double().norm(dim=1) - 1).abs().max()) < 1e-6     # unit-norm directions
    # the index-named trunk keys come back as torchvision's
    back = W.to_torchvision_keys(sd)
    assert set(back) == set(tv) and all(torch.equal(back[k], tv[k]) for k in tv)


def test_head_rejects_missing_keys_and_bad_shapes():
    sd = W.synthetic_how_head(7, "asmk", 64, 32)
    for k in W.HOW_HEAD_KEYS:
        bad = dict(sd)
        bad.pop(k)
        with pytest.raises(ValueError, match=k.replace(".", r"\.")):
            W.how_head_from_state_dict(bad)
    for k, shape in (("local_proj.weight", (64, 2048)), ("pooling.centroids", (32, 128)),
                     ("final_proj.weight", (2048, 2048)), ("pooling.weights", (31,)), ("classifier.weight", (8, 512))):
        bad = dict(sd)
        bad[k] = torch.zeros(shape)
        with pytest.raises(ValueError, match=k.split(".")[0]):
            W.how_head_from_state_dict(bad)
    with pytest.raises(ValueError, match="pooling"):
        W.synthetic_how_head(1, "spoc")
