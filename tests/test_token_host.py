"""Token without a GPU: the new C-ABI entries, the head-weight loader, and the
torch restatement (tests/token_ref.py) pinned to the reference's own
Token.forward_test / Token_Refine output (tests/golden/token.npz,
make_golden_token.py)."""
import collections
import ctypes
import inspect
import os
import sys

import numpy as np
import pytest
import torch

from research_image_retrieval_amd import _lib
from research_image_retrieval_amd import weights as W

HERE = os.path.dirname(os.path.abspath(__file__))
GOLD = os.path.join(HERE, "golden")
sys.path.insert(0, GOLD)
sys.path.insert(0, HERE)
import inputs as I  # noqa: E402
import token_ref  # noqa: E402

TAGS = ("b2_224", "b1_odd")
HEAD_CASES = ((2, 7, 7), (1, 5, 9), (1, 17, 19))
STORED = ("X", "A", "tn", "dec0", "dec1")
SWITCHES = ("enc_uniform", "slot_uniform", "cross_uniform", "self_uniform", "quick_gelu")
BAR = 1e-6


def _tag(b, h, w):
    return f"head_b{b}_{h}x{w}"


def _head_input(b, h, w):
    return torch.from_numpy(I.feature_map(9000 + h * w, b, 2048, h, w))


def _row_err(got, ref):
    got, ref = torch.as_tensor(got).double(), torch.as_tensor(ref).double()
    return ((got - ref).abs().amax(dim=-1) / ref.norm(dim=-1)).max().item()


@pytest.fixture(scope="module")
def fx():
    return np.load(os.path.join(GOLD, "token.npz"))


@pytest.fixture(scope="module")
def head(fx):
    return W.token_head_from_state_dict(W.synthetic_token_head(int(fx["head_seed"])))


@pytest.fixture(scope="module")
def refs(head):
    """The float64 and float32 restatements of every group-(b) case, computed once."""
    return {c: {dt: token_ref.head_forward(_head_input(*c), head, dt) for dt in (torch.float64, torch.float32)}
            for c in HEAD_CASES}


def test_symbols_and_abi():
    L = ctypes.CDLL(_lib.LIB_PATH)
    for name in ("rr_attention_hd128", "rr_token_pool", "rr_gelu"):
        assert hasattr(L, name) and name in _lib.SIGNATURES
    L = _lib.lib()
    assert L.rr_attention_hd128(None, None, 128, None, 128, None, 128, 1, 1, 1, 1, None, None) == _lib.RR_EINVAL
    assert L.rr_token_pool(None, None, 1, 1, 256, None, 1, None, None) == _lib.RR_EINVAL
    assert L.rr_gelu(None, None, 1, None, None) == _lib.RR_EINVAL


def test_fixture_is_no_larger_than_the_trunk_fixture():
    assert os.path.getsize(os.path.join(GOLD, "token.npz")) <= os.path.getsize(os.path.join(GOLD, "resnet_dolg.npz"))


@pytest.mark.parametrize("case", HEAD_CASES)
def test_float32_restatement_reproduces_head_fixture(fx, refs, case):
    """The float32 restatement against the reference's own float32 output, at
    1e-6 (of the row norm for the intermediates), or 4 x the float32-vs-float64
    restatement difference on the same array where that is larger: it is for
    the slot weights A, whose logits of ~10 carry 1e-7 relative error into the
    exponent (measured 1.2e-6 against 4 x 5.1e-7).  Both are printed."""
    tag = _tag(*case)
    r32, r64 = refs[case][torch.float32], refs[case][torch.float64]
    err = np.abs(r32["out"].numpy() - fx[tag + "_out"]).max()
    d = (r32["out"].double() - r64["out"]).abs().max().item()
    print(tag, "descriptor: float32 restatement vs reference", err, "; float32 vs float64 restatement", d)
    assert err <= BAR
    if case == (1, 5, 9):
        for k in STORED:
            ref = fx[f"{tag}_{k}"]
            assert ref.shape == tuple(r32[k].shape)
            e, d = _row_err(r32[k], ref), _row_err(r32[k], r64[k])
            print(f"  {k}: vs reference {e:.3e} of the row norm; float32 vs float64 restatement {d:.3e}")
            assert e <= max(BAR, 4 * d)
        assert fx[tag + "_A"].shape == (1, 4, 45) and fx[tag + "_X"].shape == (1, 45, 1024)


@pytest.mark.parametrize("tag", TAGS)
def test_restatement_reproduces_end_to_end_fixture(fx, head, tag):
    """Group (a), from the reference trunk's saved x4 (wiring)."""
    tr = np.load(os.path.join(GOLD, "resnet_dolg.npz"))
    assert int(tr["weight_seed"]) == int(fx["weight_seed"])
    assert list(tr[tag + "_case"]) == list(fx[tag + "_case"])
    got = token_ref.head_forward(torch.from_numpy(tr[tag + "_x4"]), head, torch.float32)
    err = np.abs(got["out"].numpy() - fx[tag + "_out"]).max()
    print(tag, "descriptor err", err)
    assert fx[tag + "_out"].shape[1] == 1024
    assert err <= BAR


@pytest.mark.parametrize("case", HEAD_CASES)
def test_head_fixture_is_sensitive_to_every_piece(fx, head, refs, case):
    """A condition on the fixture: each degenerate replacement (uniform encoder
    / cross / token attention, uniform slot weights, QuickGELU for erf-GELU)
    moves the float64 descriptor by at least 100 x the bar test_gpu_token.py
    holds networks.Token to on this case, max(2e-6, 4 x the float32
    restatement's distance from the float64 one); and the slot softmax is not
    a one-hot at most positions.  Measured when the fixture was made: the
    smallest ratio is QuickGELU's, 417-443 x the bar (8.3e-4 to 8.9e-4);
    uniform token self-attention 917-3871 x; the others > 5000 x; at most 1 %
    of a case's positions have a largest slot weight above 0.999."""
    r64, r32 = refs[case][torch.float64], refs[case][torch.float32]
    bar = max(2e-6, 4 * (r32["out"].double() - r64["out"]).abs().max().item())
    x = _head_input(*case)
    for sw in SWITCHES:
        moved = (token_ref.head_forward(x, head, torch.float64, **{sw: True})["out"] - r64["out"]).abs().max().item()
        print(_tag(*case), sw, "moves the descriptor by", moved, "=", moved / bar, "x the bar", bar)
        assert moved >= 100 * bar
    top = r64["A"].amax(dim=1)
    frac = (top > 0.999).double().mean().item()
    print(_tag(*case), "largest slot weight", top.min().item(), "to", top.max().item(), "; above 0.999:", frac)
    assert frac < 0.5
    assert top.min().item() < 0.5  # and far from one-hot somewhere


def _reference_keyed(seed):
    sd = W.synthetic_token_head(seed)
    for n in ("tr.encoder.0.bn", "tr.conv.1", "tr.proj.1"):
        sd[n + ".num_batches_tracked"] = torch.tensor(0)
    sd["classifier.weight"] = torch.zeros(3, 1024)             # ArcFace head: ignored
    sd["backbone.block1.0.weight"] = torch.zeros(64, 3, 7, 7)  # trunk: ignored here
    return sd


@pytest.fixture(scope="module")
def sd5():
    return _reference_keyed(5)


@pytest.mark.parametrize("prefix", ["", "module."])
def test_head_from_state_dict_shapes_and_stacks(sd5, prefix):
    sd = sd5
    h = W.token_head_from_state_dict(collections.OrderedDict((prefix + k, v) for k, v in sd.items()))
    assert set(W.TOKEN_HEAD_KEYS) <= set(sd) and len(W.TOKEN_HEAD_KEYS) == 79
    assert all(v.dtype == torch.float32 and v.is_contiguous() for v in h.values())
    assert h["conv_w"].shape == (1024, 1, 1, 2048) and h["enc_qkv_w"].shape == (3072, 1, 1, 1024)
    assert h["dec_kv_w"].shape == (4096, 1, 1, 1024) and h["out_w"].shape == (1024, 4096)
    assert h["query"].shape == (4, 1024) and torch.equal(h["query"], sd["tr.query"][0])
    for j, p in enumerate("qkv"):
        assert torch.equal(h["enc_qkv_w"][1024 * j:1024 * (j + 1)].reshape(1024, 1024),
                           sd[f"tr.encoder.0.attn.{p}.weight"])
        assert torch.equal(h["enc_qkv_b"][1024 * j:1024 * (j + 1)], sd[f"tr.encoder.0.attn.{p}.bias"])
    for i in (0, 1):
        for j, p in enumerate("kv"):
            r = 1024 * (2 * i + j)
            assert torch.equal(h["dec_kv_w"][r:r + 1024].reshape(1024, 1024), sd[f"tr.decoder.{i}.cross_attn.{p}.weight"])
            assert torch.equal(h["dec_kv_b"][r:r + 1024], sd[f"tr.decoder.{i}.cross_attn.{p}.bias"])
        for j, p in enumerate("qkv"):
            assert torch.equal(h[f"d{i}_sqkv_w"][1024 * j:1024 * (j + 1)], sd[f"tr.decoder.{i}.self_attn.{p}.weight"])
            assert torch.equal(h[f"d{i}_sqkv_b"][1024 * j:1024 * (j + 1)], sd[f"tr.decoder.{i}.self_attn.{p}.bias"])
        assert torch.equal(h[f"d{i}_fc1_w"], sd[f"tr.decoder.{i}.mlp.fc1.weight"])
        assert torch.equal(h[f"d{i}_cproj_w"], sd[f"tr.decoder.{i}.cross_attn.proj.weight"])
        assert torch.equal(h[f"d{i}_ln2_g"], sd[f"tr.decoder.{i}.bn2.weight"])
        assert float(h[f"d{i}_cproj_w"].abs().max()) > 0 and float(h[f"d{i}_sproj_w"].abs().max()) > 0
    assert float(h["enc_proj_w"].abs().max()) > 0  # the synthetic head's proj is not the reference's zero init


def _bound(x, wf, ref):
    """One fp32 rounding per folded weight (2^-24 relative) over the dot
    product, and of the bias."""
    return 2.0 ** -24 * (x.abs() @ wf.abs().t() + ref.abs() + 1)


def test_folds_equal_the_unfolded_float64_evaluation(sd5):
    sd = sd5
    h = W.token_head_from_state_dict(sd)
    d = lambda k: sd["tr." + k].double()  # noqa: E731
    rs = np.random.RandomState(0)

    def bn(p, y):
        return (y - d(p + ".running_mean")) / torch.sqrt(d(p + ".running_var") + 1e-5) * d(p + ".weight") + d(p + ".bias")

    # conv + BatchNorm2d, the conv's own bias included
    x = torch.from_numpy(rs.standard_normal((7, 2048)))
    ref = bn("conv.1", x @ d("conv.0.weight").reshape(1024, 2048).t() + d("conv.0.bias"))
    wf = h["conv_w"].reshape(1024, 2048).double()
    assert bool(((x @ wf.t() + h["conv_b"].double() - ref).abs() <= _bound(x, wf, ref)).all())
    s = d("conv.1.weight") / torch.sqrt(d("conv.1.running_var") + 1e-5)
    no_bias = (d("conv.1.bias") - d("conv.1.running_mean") * s).float()
    assert (h["conv_b"] - no_bias).abs().max().item() > 1e-2
    # the encoder's BatchNorm1d folded into its mlp: W o s on COLUMNS, b + W t
    x = torch.from_numpy(rs.standard_normal((7, 1024)))
    ref = bn("encoder.0.bn", x) @ d("encoder.0.mlp.weight").t() + d("encoder.0.mlp.bias")
    wf = h["enc_mlp_w"].reshape(1024, 1024).double()
    got = x @ wf.t() + h["enc_mlp_b"].double()
    s = d("encoder.0.bn.weight") / torch.sqrt(d("encoder.0.bn.running_var") + 1e-5)
    t = d("encoder.0.bn.bias") - d("encoder.0.bn.running_mean") * s
    bound = _bound(x, wf, ref) + 2.0 ** -24 * (d("encoder.0.mlp.weight").abs() @ t.abs())
    assert bool(((got - ref).abs() <= bound).all())
    assert (got - (x @ d("encoder.0.mlp.weight").t() + d("encoder.0.mlp.bias"))).abs().max().item() > 1e-2
    # proj + BatchNorm1d
    x = torch.from_numpy(rs.standard_normal((5, 4096)))
    ref = bn("proj.1", x @ d("proj.0.weight").t() + d("proj.0.bias"))
    wf = h["out_w"].double()
    assert bool(((x @ wf.t() + h["out_b"].double() - ref).abs() <= _bound(x, wf, ref)).all())


def test_head_rejects_missing_keys_and_bad_shapes():
    sd = W.synthetic_token_head(7)
    for k in ("tr.query", "tr.encoder.0.bn.running_var", "tr.decoder.1.self_attn.proj.bias", "tr.proj.1.weight"):
        bad = dict(sd)
        bad.pop(k)
        with pytest.raises(ValueError, match=k.replace(".", r"\.")):
            W.token_head_from_state_dict(bad)
    bad = dict(sd)
    bad["tr.decoder.0.mlp.fc1.weight"] = torch.zeros(1024, 1024)
    with pytest.raises(ValueError, match="fc1"):
        W.token_head_from_state_dict(bad)
    bad = dict(sd)
    bad["tr.query"] = torch.zeros(4, 1024)
    with pytest.raises(ValueError, match="query"):
        W.token_head_from_state_dict(bad)
    bad = dict(sd)
    bad["tr.conv.0.weight"] = torch.zeros(1024, 2048)
    with pytest.raises(ValueError, match="conv"):
        W.token_head_from_state_dict(bad)


def test_token_constructor_order_without_gpu():
    from research_image_retrieval_amd.networks import RetrievalNet, Token, Token_Refine
    names = list(inspect.signature(Token.__init__).parameters)[1:]
    assert names == ["outputdim", "classifier_num", "pretrained", "backbone", "state_dict", "seed", "device",
                     "conv_math", "stride_on"]
    assert list(inspect.signature(RetrievalNet.__init__).parameters)[1:2] == ["classifier_num"]
    assert issubclass(RetrievalNet, Token)
    with pytest.raises(ValueError, match="outputdim"):
        Token(outputdim=512)
    with pytest.raises(ValueError, match="outputdim"):
        Token(512, 81313, None, "resnet101")  # the reference's positional order
    with pytest.raises(ValueError, match="pretrained"):
        Token(1024, 81313, "filip", "resnet101")
    with pytest.raises(ValueError, match="mid_dim"):
        Token_Refine(8, 4, 512, 1, 2, head={})
    with pytest.raises(ValueError, match="decoder"):
        Token_Refine(8, 4, 1024, 1, 3, head={})
