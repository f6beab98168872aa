"""DOLG on the GPU: rr_dolg_local_pool and rr_dolg_orth_fuse against the
float64 evaluation of tests/dolg_ref.py (pinned to the reference's own output
by tests/test_dolg_host.py), and networks.DOLG end to end against
tests/golden/dolg.npz (the reference's DOLG.forward_test, make_golden_dolg.py).

The pool bar: per image, max-abs error <= 1e-6 * ||reference row||_2 -- the
project's unit-norm descriptor bar (smoke(), test_gpu_e2e.py) applied to the
row scaled to unit norm."""
import ctypes
import os
import sys

import numpy as np
import pytest
import torch

from research_image_retrieval_amd import _lib, ops
from research_image_retrieval_amd import weights as W
from research_image_retrieval_amd.extract import extract_vectors
from research_image_retrieval_amd.networks import DOLG

pytestmark = pytest.mark.gpu
HERE = os.path.dirname(os.path.abspath(__file__))
GOLD = os.path.join(HERE, "golden")
sys.path.insert(0, GOLD)
sys.path.insert(0, HERE)
import dolg_ref  # noqa: E402
import inputs as I  # noqa: E402

BAR = 1e-6
POOL_SHAPES = [(1, 1, 256), (3, 40, 1024), (2, 196, 1024), (5, 63, 512), (1, 4099, 1024),
               # b >= 1024: whole images per workgroup with several pixels per wave (every case
               # above with hw > 1 is split over workgroups); and the widest row, c = 2048
               (1024, 9, 256), (2, 5, 2048)]
B2 = 0.1


def _pool_case(b, hw, c):
    """Distinct random data per image (negative values included, so the ReLU
    matters), and, where the map has room, one all-zero pixel row, one row with
    logit > 20 and one with logit < -30, in different images when b > 1."""
    rs = np.random.RandomState(1000 * b + hw + c)
    y = rs.standard_normal((b, hw, c)).astype(np.float32)
    w2 = (rs.standard_normal(c) * 0.05).astype(np.float32)
    special = {}
    if hw >= 4:
        pos, neg = w2 * (w2 > 0), w2 * (w2 < 0)
        y[0 % b, hw // 3] = 0.0
        hi = (w2 > 0) * np.float32(25.0 / pos.sum())         # relu(y) . w2 = 25
        lo = (w2 < 0) * np.float32(35.0 / -neg.sum())        # relu(y) . w2 = -35
        y[1 % b, hw // 2] = hi
        y[2 % b, hw - 1] = lo
        special = {"hi": (1 % b, hw // 2), "lo": (2 % b, hw - 1)}
    return torch.from_numpy(y), torch.from_numpy(w2), special


def _row_err(got, ref):
    """max over images of max|got - ref| / ||ref row||_2"""
    return ((got.double() - ref).abs().amax(dim=1) / ref.norm(dim=1)).max().item()


@pytest.mark.parametrize("b,hw,c", POOL_SHAPES)
def test_local_pool_vs_float64(cuda, b, hw, c):
    y, w2, special = _pool_case(b, hw, c)
    ref = dolg_ref.local_pool(y, w2, B2, torch.float64)
    if special:
        logit = torch.relu(y.double()) @ w2.double() + B2
        assert logit[special["hi"]] > 20 and logit[special["lo"]] < -30
    got = ops.dolg_local_pool(y.to(cuda), w2.to(cuda), B2).cpu()
    assert got.shape == (b, c) and bool(torch.isfinite(got).all())
    err = _row_err(got, ref)
    err32 = _row_err(dolg_ref.local_pool(y, w2, B2, torch.float32), ref)
    print(f"pool ({b},{hw},{c}): kernel {err:.3e}  float32 torch {err32:.3e}  (of the row norm; bar {BAR:.0e})")
    assert err <= BAR


@pytest.mark.parametrize("hw", [196, 4099])
def test_local_pool_covers_every_pixel_once(cuda, hw):
    """y is zero except at pixels 0, hw - 1 and five seeded positions: the
    output is the sum of those seven terms / hw (a dropped or doubled pixel is
    a 14 % error)."""
    c = 1024
    rs = np.random.RandomState(hw)
    px = np.unique(np.concatenate([[0, hw - 1], rs.choice(np.arange(1, hw - 1), 5, replace=False)]))
    assert len(px) == 7
    rows = torch.from_numpy(rs.standard_normal((1, 7, c)).astype(np.float32))
    w2 = torch.from_numpy((rs.standard_normal(c) * 0.05).astype(np.float32))
    y = torch.zeros((1, hw, c))
    y[0, torch.from_numpy(px)] = rows[0]
    ref = dolg_ref.local_pool(rows, w2, B2, torch.float64) * (7.0 / hw)
    got = ops.dolg_local_pool(y.to(cuda), w2.to(cuda), B2).cpu()
    err = _row_err(got, ref)
    print(f"coverage hw={hw}: {err:.3e}")
    assert err <= BAR


@pytest.mark.parametrize("b,hw,c", [(1, 4099, 1024), (3, 40, 1024)])
def test_local_pool_reruns_bit_identical(cuda, b, hw, c):
    y, w2, _ = _pool_case(b, hw, c)
    y, w2 = y.to(cuda), w2.to(cuda)
    a = ops.dolg_local_pool(y, w2, B2)
    bb = ops.dolg_local_pool(y, w2, B2)
    assert torch.equal(a.view(torch.int32), bb.view(torch.int32))


@pytest.mark.parametrize("c", [256, 1024])
@pytest.mark.parametrize("b", [1, 5])
def test_orth_fuse(cuda, b, c):
    """fg = 0.7 m + noise, so the removed component is large."""
    rs = np.random.RandomState(b * 10000 + c)
    m = rs.standard_normal((b, c)).astype(np.float32)
    fg = (0.7 * m + 0.7 * rs.standard_normal((b, c))).astype(np.float32)
    m, fg = torch.from_numpy(m), torch.from_numpy(fg)
    out = ops.dolg_orth_fuse(fg.to(cuda), m.to(cuda)).cpu()
    assert out.shape == (b, 2 * c)
    assert torch.equal(out[:, :c].view(torch.int32), fg.view(torch.int32))
    fo = out[:, c:]
    ref = dolg_ref.orth_pool(fg.double(), m.double().unsqueeze(1))
    assert (ref.norm(dim=1) < 0.8 * m.double().norm(dim=1)).all()  # a large component was removed
    err = _row_err(fo, ref)
    # fo . fg = m . fg - k fg . fg with k = (m . fg) / (fg . fg) from two fp32
    # dot products of c terms: rounding leaves about sqrt(c) 2^-24 |m . fg|, and
    # |m . fg| <= ||fo|| ||fg|| cot(angle) with cot near 1 here; 8x margin
    cos = (fo.double() * fg.double()).sum(1).abs() / (fo.double().norm(dim=1) * fg.double().norm(dim=1))
    print(f"orth ({b},{c}): err {err:.3e}  |cos(fo, fg)| {cos.max().item():.3e}")
    assert err <= BAR
    assert cos.max().item() <= 8 * np.sqrt(c) * 2.0 ** -24


def test_argument_errors(cuda):
    L = _lib.lib()
    hd = _lib.handle(0)
    t = torch.zeros(4096, device=cuda)
    p = ctypes.c_void_p(t.data_ptr())
    assert L.rr_dolg_local_pool(hd, p, 1, 4, 100, p, 0.0, p, None) == _lib.RR_EINVAL
    assert L.rr_dolg_local_pool(hd, p, 1, 1, 2304, p, 0.0, p, None) == _lib.RR_EINVAL  # c > 2048
    assert L.rr_dolg_local_pool(hd, p, 1, 0, 256, p, 0.0, p, None) == _lib.RR_EINVAL
    assert L.rr_dolg_local_pool(hd, None, 1, 1, 256, p, 0.0, p, None) == _lib.RR_EINVAL
    assert L.rr_dolg_local_pool(hd, ctypes.c_void_p(t.data_ptr() + 4), 1, 1, 256, p, 0.0, p, None) == _lib.RR_EINVAL
    assert L.rr_dolg_local_pool(hd, p, 0, 4, 256, p, 0.0, p, None) == _lib.RR_OK
    assert L.rr_dolg_orth_fuse(hd, p, p, 0, 256, p, None) == _lib.RR_OK
    assert L.rr_dolg_orth_fuse(hd, p, None, 1, 256, p, None) == _lib.RR_EINVAL
    with pytest.raises(_lib.RRError):
        ops.dolg_local_pool(torch.zeros((1, 4, 100), device=cuda), torch.zeros(100, device=cuda), 0.0)


# ---- end to end ------------------------------------------------------------
@pytest.fixture(scope="module")
def fx():
    return np.load(os.path.join(GOLD, "dolg.npz"))


@pytest.fixture(scope="module")
def nets(fx):
    """networks.DOLG on both conv cores from one reference-keyed checkpoint:
    globalmodel.* in ResNet_DOLG layout (stride on the 1x1) + the head."""
    sd = {"globalmodel." + k: v
          for k, v in W.to_dolg_keys(W.synthetic_resnet_state_dict("resnet101", int(fx["weight_seed"]))).items()}
    sd.update(W.synthetic_dolg_head(int(fx["head_seed"])))
    made = {}

    def get(conv_math):
        if conv_math not in made:
            made[conv_math] = DOLG(state_dict=sd, device="cuda:0", conv_math=conv_math, stride_on="1x1")
        return made[conv_math]
    return get


def _e2e_err(net, fx, tag):
    seed, b, h, w = (int(v) for v in fx[tag + "_case"])
    got = net.forward_test(I.trunk_input(seed, b, h, w).to("cuda:0")).cpu().numpy()
    assert got.shape == (b, 512) == (b, net.outputdim) and net.meta == {"outputdim": 512}
    return np.abs(got - fx[tag + "_out"]).max()


@pytest.mark.parametrize("tag", ["b2_224", "b1_odd"])
def test_dolg_vs_reference(cuda, fx, nets, tag):
    e32 = _e2e_err(nets("f32"), fx, tag)
    eh2 = _e2e_err(nets("h2"), fx, tag)
    print(f"DOLG {tag}: descriptor max|err| f32 {e32:.3e}  h2 {eh2:.3e}")
    assert e32 <= 1e-6
    assert eh2 <= 1e-6 and eh2 <= 2 * e32


def test_dolg_local_mean_vs_reference(cuda, fx, nets):
    net = nets("f32")
    seed, b, h, w = (int(v) for v in fx["b1_odd_case"])
    x = I.trunk_input(seed, b, h, w).permute(0, 2, 3, 1).contiguous().to(cuda)
    x3, _ = net.globalmodel(x, return_x3=True)
    m = net.local_mean(x3).cpu()
    err = _row_err(m, torch.from_numpy(fx["b1_odd_m"]).double())
    print(f"DOLG b1_odd: m err {err:.3e} of the row norm")
    assert err <= BAR


def test_dolg_extract_vectors_multiscale(cuda, nets):
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
    assert got.shape == (4, 512)
    assert torch.equal(got.view(torch.int32), ref.view(torch.int32))


def test_dolg_streams_bit_identical_to_serial_parts(cuda, nets):
    net = nets("h2")
    rs = np.random.RandomState(23)
    imgs = torch.from_numpy(rs.randint(0, 256, size=(6, 96, 96, 3), dtype=np.uint8)).to(cuda)
    ref = torch.cat([net.forward_test_u8(imgs[:3]), net.forward_test_u8(imgs[3:])])
    streams = [torch.cuda.Stream(cuda) for _ in range(2)]
    for _ in range(2):
        out = net.forward_test_u8_streams(imgs, streams, lag=1)
        assert out.shape == (6, 512)
        assert torch.equal(out.view(torch.int32), ref.view(torch.int32))
