"""SOLAR on the GPU: rr_soa_attention against the float64 evaluation of
tests/solar_ref.py (pinned to the reference's own output by
tests/test_solar_host.py), and networks.SOLAR end to end and head-only against
tests/golden/solar.npz (the reference's SOLAR.forward_test and SOABlock_GeM,
make_golden_solar.py).

The kernel bar, per case: max over rows of max|got - ref| / ||ref row||_2 <=
max(1e-6, 4 e32), e32 the same quantity for the float32 torch evaluation of
the restatement (computed here and printed).  1e-6 is the project's row bar
(test_gpu_dolg.py); the 4x margin covers the MFMA's serial fp32 chains against
BLAS's blocked sums, a difference the softmax multiplies by logits of 10-20."""
import ctypes
import os
import sys

import numpy as np
import pytest
import torch

from research_image_retrieval_amd import _lib, ops
from research_image_retrieval_amd import weights as W
from research_image_retrieval_amd.extract import extract_vectors
from research_image_retrieval_amd.networks import SOLAR

pytestmark = pytest.mark.gpu
HERE = os.path.dirname(os.path.abspath(__file__))
GOLD = os.path.join(HERE, "golden")
sys.path.insert(0, GOLD)
sys.path.insert(0, HERE)
import inputs as I  # noqa: E402
import solar_ref  # noqa: E402

BAR = 1e-6
SHAPES = [(1, 1, 256), (2, 15, 256), (2, 16, 512), (1, 17, 1024), (3, 31, 256), (1, 32, 1024), (3, 33, 256),
          (2, 49, 1024), (5, 63, 512), (1, 65, 1024), (2, 130, 1024), (1, 323, 1024), (64, 49, 1024),
          (1, 1024, 1024)]
HEAD_CASES = ((2, 7, 7), (1, 5, 9), (1, 17, 19))


def _case(b, hw, c, plant=True):
    """fgh = N(0,1) with the f and g columns scaled by 2 (logits of 10-20).
    Where hw >= 8: one query whose f is all negative (relu(f) == 0: uniform
    attention, the mean of the h rows), and one key whose g is 3 |f| of another
    query (a dominant logit, 6 sqrt(c) ~ 96-192: the running max jumps and the
    accumulated output is rescaled to nothing), in different images when b > 1."""
    rs = np.random.RandomState(1000 * b + hw + c)
    x = rs.standard_normal((b, hw, 3 * c)).astype(np.float32)
    x[..., :2 * c] *= 2.0
    special = {}
    if plant and hw >= 8:
        zq = (0, hw // 3)
        dq, dk = (1 % b, hw // 2), hw - 2
        x[zq[0], zq[1], :c] = -np.abs(x[zq[0], zq[1], :c]) - 0.01
        x[dq[0], dk, c:2 * c] = 3.0 * np.abs(x[dq[0], dq[1], :c])
        special = {"zero_query": zq, "dominant": (dq, dk)}
    return torch.from_numpy(x), special


def _row_err(got, ref):
    """max over rows of max|got - ref| / ||ref row||_2"""
    return ((got.double() - ref).abs().amax(dim=-1) / ref.norm(dim=-1)).max().item()


@pytest.mark.parametrize("b,hw,c", SHAPES)
def test_soa_attention_vs_float64(cuda, b, hw, c):
    fgh, special = _case(b, hw, c)
    att, ref = solar_ref.attention(fgh, c, torch.float64)
    _, ref32 = solar_ref.attention(fgh, c, torch.float32)
    got = ops.soa_attention(fgh.to(cuda), c).cpu()
    assert got.shape == (b, hw, c) and bool(torch.isfinite(got).all())
    err, e32 = _row_err(got, ref), _row_err(ref32, ref)
    bar = max(BAR, 4 * e32)
    print(f"soa ({b},{hw},{c}): kernel {err:.3e}  float32 torch {e32:.3e}  bar {bar:.3e}  (of the row norm)")
    if special:
        (qi, qq), (di, dq), dk = special["zero_query"], special["dominant"][0], special["dominant"][1]
        # the planted rows do what they were planted for
        assert float(att[qi, qq].max() - att[qi, qq].min()) < 1e-15
        assert float(att[di, dq, dk]) > 0.999
        mean_h = fgh[qi, :, 2 * c:].double().mean(dim=0)
        e_mean = ((got[qi, qq].double() - mean_h).abs().max() / mean_h.norm()).item()
        print(f"   zero query -> mean of h rows: {e_mean:.3e}; dominant key weight {float(att[di, dq, dk]):.6f}")
        assert e_mean <= BAR
    assert err <= bar


@pytest.mark.parametrize("b,hw,c", [(1, 17, 1024), (1, 323, 1024), (1, 1024, 1024), (2, 40, 768)])
def test_soa_attention_unplanted_vs_float64(cuda, b, hw, c):
    """The planted key's g is positive everywhere, so it draws EVERY query of
    its image (with b = 1, the whole case) to itself.  Here nothing is planted:
    every row is a spread softmax over several key tiles, at b = 1; and
    c = 768, the one supported width the planted shapes leave out."""
    fgh, _ = _case(b, hw, c, plant=False)
    att, ref = solar_ref.attention(fgh, c, torch.float64)
    _, ref32 = solar_ref.attention(fgh, c, torch.float32)
    got = ops.soa_attention(fgh.to(cuda), c).cpu()
    err, e32 = _row_err(got, ref), _row_err(ref32, ref)
    bar = max(BAR, 4 * e32)
    print(f"soa unplanted ({b},{hw},{c}): kernel {err:.3e}  float32 torch {e32:.3e}  bar {bar:.3e}; attention row "
          f"maxima {float(att.amax(-1).min()):.3f} to {float(att.amax(-1).max()):.3f}")
    assert float(att.amax(-1).max()) < 0.999  # no row is a one-hot
    assert err <= bar


@pytest.mark.parametrize("b,hw,c", [(2, 130, 1024), (3, 33, 256)])
def test_soa_attention_reruns_bit_identical(cuda, b, hw, c):
    fgh = _case(b, hw, c)[0].to(cuda)
    a = ops.soa_attention(fgh, c)
    bb = ops.soa_attention(fgh, c)
    assert torch.equal(a.view(torch.int32), bb.view(torch.int32))


@pytest.mark.parametrize("hw,c", [(33, 256), (49, 1024)])
def test_soa_attention_image_alone_equals_image_in_batch(cuda, hw, c):
    fgh = _case(3, hw, c)[0].to(cuda)
    whole = ops.soa_attention(fgh, c)
    for i in range(3):
        one = ops.soa_attention(fgh[i:i + 1].contiguous(), c)
        assert torch.equal(one[0].view(torch.int32), whole[i].view(torch.int32))


def test_soa_attention_at_the_position_limit(cuda):
    """hw = 65535, the most rr.h allows: 4096 query tiles of an image, 4096 key
    tiles per query, both ending in a 15-row tile.  The float64 restatement is
    written out for three query rows only (all hw^2 scores would be 4.4 TFLOP on
    the host); same bar as above."""
    hw, c = 65535, 256
    rs = np.random.RandomState(65535)
    fgh = torch.from_numpy(rs.standard_normal((1, hw, 3 * c)).astype(np.float32))
    fgh[..., :2 * c] *= 2.0
    rows = torch.tensor([0, 32767, hw - 1])
    got = ops.soa_attention(fgh.to(cuda), c)[0, rows.to(cuda)].cpu()

    def ref_rows(dt):
        f = torch.relu(fgh[0, rows, :c].to(dt))
        g = torch.relu(fgh[0, :, c:2 * c].to(dt))
        attn = torch.softmax((c ** -.50) * (f @ g.t()), dim=-1)
        return attn @ fgh[0, :, 2 * c:].to(dt)

    ref = ref_rows(torch.float64)
    err, e32 = _row_err(got, ref), _row_err(ref_rows(torch.float32), ref)
    bar = max(BAR, 4 * e32)
    print(f"soa (1,{hw},{c}) rows {rows.tolist()}: kernel {err:.3e}  float32 torch {e32:.3e}  bar {bar:.3e}")
    assert err <= bar


def test_soa_attention_offsets_past_2_31_elements(cuda):
    """58000 images x 49 positions x 768 columns = 2.18e9 input elements: the
    last image lies past 2^31 elements (and 2^33 bytes).  It must come out as
    the same bits as that image alone; so must the first."""
    b, hw, c = 58000, 49, 256
    assert (b - 1) * hw * 3 * c > 2 ** 31
    g = torch.Generator(device=cuda).manual_seed(5)
    fgh = torch.randn((b, hw, 3 * c), device=cuda, generator=g)
    whole = ops.soa_attention(fgh, c)
    for i in (0, b - 1):
        one = ops.soa_attention(fgh[i:i + 1].contiguous(), c)
        assert bool(torch.isfinite(one).all()) and float(one.abs().max()) > 0
        assert torch.equal(one[0].view(torch.int32), whole[i].view(torch.int32))
    del fgh, whole, one
    torch.cuda.empty_cache()  # 11.6 GB back to the device for the tests that follow


def test_soa_attention_accepts_nhwc_maps(cuda):
    fgh = _case(2, 15, 256)[0].to(cuda)
    flat = ops.soa_attention(fgh, 256)
    maps = ops.soa_attention(fgh.reshape(2, 3, 5, 768), 256)
    assert maps.shape == (2, 3, 5, 256)
    assert torch.equal(maps.reshape(2, 15, 256).view(torch.int32), flat.view(torch.int32))
    with pytest.raises(ValueError):
        ops.soa_attention(fgh, 512)


def test_argument_errors(cuda):
    L = _lib.lib()
    hd = _lib.handle(0)
    t = torch.zeros(8192, device=cuda)
    p = ctypes.c_void_p(t.data_ptr())
    assert L.rr_soa_attention(hd, p, 1, 1, 100, p, None) == _lib.RR_EINVAL
    assert L.rr_soa_attention(hd, p, 1, 1, 1280, p, None) == _lib.RR_EINVAL  # c > 1024
    assert L.rr_soa_attention(hd, p, 1, 0, 256, p, None) == _lib.RR_EINVAL
    assert L.rr_soa_attention(hd, p, 1, 65536, 256, p, None) == _lib.RR_EINVAL
    assert L.rr_soa_attention(hd, None, 1, 1, 256, p, None) == _lib.RR_EINVAL
    assert L.rr_soa_attention(hd, p, 1, 1, 256, None, None) == _lib.RR_EINVAL
    assert L.rr_soa_attention(hd, ctypes.c_void_p(t.data_ptr() + 4), 1, 1, 256, p, None) == _lib.RR_EINVAL
    assert L.rr_soa_attention(hd, p, 1, 1, 256, ctypes.c_void_p(t.data_ptr() + 4), None) == _lib.RR_EINVAL
    assert b"rr_soa_attention" in L.rr_last_error(hd)
    assert L.rr_soa_attention(hd, p, 0, 4, 256, p, None) == _lib.RR_OK
    with pytest.raises(_lib.RRError):
        ops.soa_attention(torch.zeros((1, 4, 300), device=cuda), 100)


# ---- end to end ------------------------------------------------------------
@pytest.fixture(scope="module")
def fx():
    return np.load(os.path.join(GOLD, "solar.npz"))


@pytest.fixture(scope="module")
def nets(fx):
    """networks.SOLAR on both conv cores from one reference-keyed checkpoint:
    backbone.* in ResNet_DOLG layout (stride on the 1x1) + the head."""
    sd = {"backbone." + k: v
          for k, v in W.to_dolg_keys(W.synthetic_resnet_state_dict("resnet101", int(fx["weight_seed"]))).items()}
    sd.update(W.synthetic_solar_head(int(fx["head_seed"])))
    made = {}

    def get(conv_math):
        if conv_math not in made:
            made[conv_math] = SOLAR(state_dict=sd, device="cuda:0", conv_math=conv_math, stride_on="1x1")
        return made[conv_math]
    return get


def _e2e_err(net, fx, tag):
    seed, b, h, w = (int(v) for v in fx[tag + "_case"])
    got = net.forward_test(I.trunk_input(seed, b, h, w).to("cuda:0")).cpu().numpy()
    assert got.shape == (b, 2048) == (b, net.outputdim) and net.meta == {"outputdim": 2048}
    return np.abs(got - fx[tag + "_out"]).max()


@pytest.mark.parametrize("tag", ["b2_224", "b1_odd"])
def test_solar_vs_reference(cuda, fx, nets, tag):
    e32 = _e2e_err(nets("f32"), fx, tag)
    eh2 = _e2e_err(nets("h2"), fx, tag)
    print(f"SOLAR {tag}: descriptor max|err| f32 {e32:.3e}  h2 {eh2:.3e}")
    assert e32 <= 1e-6
    assert eh2 <= 1e-6


@pytest.mark.parametrize("case", HEAD_CASES)
def test_solar_head_vs_reference(cuda, fx, nets, case):
    """pooling + tail alone on maps where the attention is far from uniform
    (test_solar_host.py: uniform attention moves these descriptors by >= 1e-4)."""
    b, h, w = case
    tag = f"head_b{b}_{h}x{w}"
    x = torch.from_numpy(I.feature_map(7000 + h * w, b, 2048, h, w)).permute(0, 2, 3, 1).contiguous().to(cuda)
    errs = {}
    for cm in ("f32", "h2"):
        net = nets(cm)
        pooled = net.pooling(x)
        got = net.tail(pooled).cpu().numpy()
        ref_p = torch.from_numpy(fx[tag + "_pooled"]).double()
        errs[cm] = (np.abs(got - fx[tag + "_out"]).max(), _row_err(pooled.cpu(), ref_p))
    print(f"SOLAR {tag}: descriptor max|err| / pooled row err  f32 {errs['f32'][0]:.3e} / {errs['f32'][1]:.3e}  "
          f"h2 {errs['h2'][0]:.3e} / {errs['h2'][1]:.3e}")
    assert errs["f32"][0] <= 1e-6
    assert errs["h2"][0] <= 1e-6


def test_solar_extract_vectors_multiscale(cuda, nets):
    net = nets("h2")
    rs = np.random.RandomState(17)
    imgs = torch.from_numpy(rs.randint(0, 256, size=(4, 96, 128, 3), dtype=np.uint8))
    ms = [1, 2 ** -0.5, 0.5]
    got = extract_vectors(net, [imgs[:2], imgs[2:]], ms=ms, device=cuda, print_freq=0)
    parts = []
    for batch in (imgs[:2], imgs[2:]):
        x = ops.preprocess_u8(batch.to(cuda))
        acc = None
        for s in ms:
            xs = x if s == 1 else ops.resize_bilinear(x, int(96 * s), int(128 * s), scale_factor=s)
            f = net.forward_test_nhwc(xs)
            acc = f.clone() if acc is None else acc.add_(f)
        acc.div_(len(ms))
        parts.append(ops.l2_normalize(acc, 1e-12).cpu())
    ref = torch.cat(parts)
    assert got.shape == (4, 2048)
    assert torch.equal(got.view(torch.int32), ref.view(torch.int32))


def test_solar_streams_bit_identical_to_serial_parts(cuda, nets):
    net = nets("h2")
    rs = np.random.RandomState(23)
    imgs = torch.from_numpy(rs.randint(0, 256, size=(6, 96, 96, 3), dtype=np.uint8)).to(cuda)
    ref = torch.cat([net.forward_test_u8(imgs[:3]), net.forward_test_u8(imgs[3:])])
    streams = [torch.cuda.Stream(cuda) for _ in range(2)]
    for _ in range(2):
        out = net.forward_test_u8_streams(imgs, streams, lag=1)
        assert out.shape == (6, 2048)
        assert torch.equal(out.view(torch.int32), ref.view(torch.int32))
