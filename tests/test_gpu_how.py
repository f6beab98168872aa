"""HOW on the GPU: rr_how_vlad and rr_how_asmk against the float64 evaluation
of tests/how_ref.py (pinned to the reference's own output by
tests/test_how_host.py), and models.HOWVLADWrapper / HOWASMKWrapper end to end
and head-only against tests/golden/how.npz (the reference's HOWModel with its
VLADPooling / ASMKPooling, make_golden_how.py).

The kernel bar, per case: max over images of max|got - ref| / ||ref row||_2 <=
max(1e-6, 4 e32), e32 the same quantity for the float32 torch evaluation
(computed here and printed), as tests/test_gpu_token.py; a row is an image's
whole output.  The descriptor bar: max(2e-6, 4 x the float32 restatement's
distance from the float64 one).

ASMK decides per position, so its cases carry a condition checked here first,
in float64: NO position's argmin margin (second-nearest minus nearest distance)
or threshold margin (|min-dist - threshold|) is under 1e-5 (float32 cdist is off
by < 1e-6 on such inputs).  Each case's seed was picked by a CPU scan for that
condition and is recorded in ASMK_SEEDS."""
import ctypes
import os
import sys

import numpy as np
import pytest
import torch

from research_image_retrieval_amd import _lib, models, ops
from research_image_retrieval_amd import weights as W
from research_image_retrieval_amd.extract import extract_vectors
from research_image_retrieval_amd.networks import ConvDimReduction, GeMPCAw

pytestmark = pytest.mark.gpu
HERE = os.path.dirname(os.path.abspath(__file__))
GOLD = os.path.join(HERE, "golden")
sys.path.insert(0, GOLD)
sys.path.insert(0, HERE)
import inputs as I  # noqa: E402
import how_ref  # noqa: E402

BAR = 1e-6
MARGIN = 1e-5
# (b, n, d, k): one position; the 7x7 map; a ragged last step; several chunks of
# one image (323 = 6 x 54); 16 chunks; many images; 64 chunks (the position
# split's adding kernel at its widest here); a narrow head; both limits; k no
# multiple of anything; one centroid; widths that are no power of two, in the
# narrow instance (6 channel tiles over 4 waves) and in the wide one (16
# positions a step, 40 16-B groups a row over 16 threads)
SHAPES = [(1, 1, 128, 64), (2, 49, 128, 64), (3, 50, 128, 64), (1, 323, 128, 64), (1, 1024, 128, 64),
          (64, 49, 128, 64), (1, 4096, 128, 64), (2, 33, 64, 32), (1, 17, 256, 128), (1, 45, 128, 37), (2, 7, 32, 1),
          (2, 20, 96, 20), (1, 40, 160, 70)]
# ASMK: the seed of each shape's case, the first from 0 at which every position's
# float64 margins are >= 2e-5 (scanned on the CPU with how_ref.margins; the
# smallest found: 2.4e-5 argmin and 2.4e-5 threshold, both at (64, 49))
ASMK_SEEDS = {(1, 1, 128, 64): 0, (2, 49, 128, 64): 0, (3, 50, 128, 64): 0, (1, 323, 128, 64): 0,
              (1, 1024, 128, 64): 4, (64, 49, 128, 64): 3, (1, 4096, 128, 64): 10, (2, 33, 64, 32): 0,
              (1, 17, 256, 128): 0, (1, 45, 128, 37): 0, (2, 7, 32, 1): 0, (2, 20, 96, 20): 1, (1, 40, 160, 70): 0}
HEAD_CASES = ((2, 7, 7), (1, 5, 9), (1, 17, 19))
POOLINGS = ("vlad", "asmk")


def _row_err(got, ref):
    """max over rows of max|got - ref| / ||ref row||_2"""
    return ((got.double() - ref.double()).abs().amax(dim=-1) / ref.double().norm(dim=-1)).max().item()


def _bits_equal(a, b):
    return a.shape == b.shape and torch.equal(a.contiguous().view(torch.int32), b.contiguous().view(torch.int32))


def _rows(b, n, d, k, seed):
    """Raw rows N(0,1) x a per-row gain in [0.5, 2) (so the normalisation
    matters) and unit-norm random centroids, as trained ones of unit-norm
    descriptors."""
    rs = np.random.RandomState(seed)
    x = rs.standard_normal((b, n, d)) * rs.uniform(0.5, 2.0, (b, n, 1))
    c = rs.standard_normal((k, d))
    c /= np.linalg.norm(c, axis=1, keepdims=True)
    return x.astype(np.float32), c.astype(np.float32)


# ---- rr_how_vlad -----------------------------------------------------------
def _vlad_case(b, n, d, k):
    """Planted where n >= 8: an all-zero raw row (x^ = 0); centroids 0 and k - 1
    identical (k >= 2); one row equal to centroid k // 2 (its weight > 0.999)."""
    x, c = _rows(b, n, d, k, 1000000 * b + 1000 * n + d + k)
    special = {}
    if n >= 8:
        x[0, n // 3] = 0.0
        x[b - 1, n // 2] = c[k // 2]
        if k >= 2:
            c[k - 1] = c[0]
        special = {"zero": (0, n // 3), "equal": (b - 1, n // 2, k // 2), "twins": k >= 2}
    return torch.from_numpy(x), torch.from_numpy(c), special


@pytest.mark.parametrize("b,n,d,k", SHAPES)
def test_how_vlad_vs_float64(cuda, b, n, d, k):
    x, c, special = _vlad_case(b, n, d, k)
    r64, r32 = how_ref.vlad(x, c, dtype=torch.float64), how_ref.vlad(x, c, dtype=torch.float32)
    xd, cd = x.to(cuda), c.to(cuda)
    got = ops.how_vlad(xd, cd)
    assert got.shape == (b, k * d)
    assert _bits_equal(got, ops.how_vlad(xd, cd))  # reruns
    got = got.cpu()
    assert bool(torch.isfinite(got).all())
    err, e32 = _row_err(got, r64["vlad"]), _row_err(r32["vlad"], r64["vlad"])
    bar = max(BAR, 4 * e32)
    top = r64["assign"].amax(dim=2)
    print(f"how_vlad ({b},{n},{d},{k}): kernel {err:.3e}  float32 torch {e32:.3e}  bar {bar:.3e}  (of the row norm); "
          f"top weight median {top.median().item():.3f}")
    if k == 1:  # every weight is exactly 1: out = sum_p x^_p - n c
        assert bool((r64["assign"] == 1.0).all())
    if special:
        bi, pi, ci = special["equal"]
        w_eq = float(r64["assign"][bi, pi, ci])
        print(f"   the row equal to centroid {ci} has weight {w_eq:.6f}")
        assert w_eq > 0.999
        assert float(r64["desc"][special["zero"]].abs().max()) == 0.0
        if special["twins"]:
            rows = got.view(b, k, d)
            assert _bits_equal(rows[:, 0], rows[:, k - 1])
    assert err <= bar


def test_how_vlad_one_hot_assignments_of_the_constructor_centroids(cuda):
    """The constructor's U(0,1) centroids (models/how_vlad.py:24-28): distances
    of about 6.6 whose logits spread over tens of units, so most assignments
    are one-hots (on these rows the median top weight is 0.974 against 0.79
    with unit-norm centroids, and 22 % of the positions are above 0.999);
    the kernel must still match."""
    b, n, d, k = 2, 49, 128, 64
    rs = np.random.RandomState(5)
    x = torch.from_numpy(rs.standard_normal((b, n, d)).astype(np.float32))
    c = torch.from_numpy(rs.uniform(0, 1, (k, d)).astype(np.float32))
    r64, r32 = how_ref.vlad(x, c, dtype=torch.float64), how_ref.vlad(x, c, dtype=torch.float32)
    got = ops.how_vlad(x.to(cuda), c.to(cuda)).cpu()
    err, e32 = _row_err(got, r64["vlad"]), _row_err(r32["vlad"], r64["vlad"])
    bar = max(BAR, 4 * e32)
    top = r64["assign"].amax(dim=2)
    print(f"how_vlad U(0,1) centroids: kernel {err:.3e}  float32 torch {e32:.3e}  bar {bar:.3e}; top weight median "
          f"{top.median().item():.4f}, above 0.999: {(top > 0.999).double().mean().item():.3f}")
    assert top.median().item() > 0.95 and (top > 0.999).double().mean().item() > 0.2
    assert err <= bar


@pytest.mark.parametrize("n,d,k", [(49, 128, 64), (50, 128, 64), (33, 64, 32)])
def test_how_vlad_image_alone_equals_image_in_batch(cuda, n, d, k):
    """The position split is a function of (b, n); at n <= 64 nothing is split."""
    x, c, _ = _vlad_case(3, n, d, k)
    xd, cd = x.to(cuda), c.to(cuda)
    whole = ops.how_vlad(xd, cd)
    for i in range(3):
        assert _bits_equal(ops.how_vlad(xd[i:i + 1].contiguous(), cd)[0], whole[i])
    assert _bits_equal(ops.how_vlad(xd.reshape(3, 1, n, d), cd), whole)  # an NHWC map


def test_how_vlad_offsets_past_2_31_elements(cuda):
    """350000 images x 49 positions x 128 = 2.2e9 input elements and 350000 x
    8192 = 2.9e9 output elements (20 GB together): the first and the last image
    must come out as the same bits as the image alone."""
    b, n, d, k = 350000, 49, 128, 64
    assert b * n * d > 2 ** 31 and b * k * d > 2 ** 31
    g = torch.Generator(device=cuda).manual_seed(11)
    x = torch.randn((b, n, d), device=cuda, generator=g)
    c = torch.nn.functional.normalize(torch.randn((k, d), device=cuda, generator=g), dim=1)
    whole = ops.how_vlad(x, c)
    for i in (0, b - 1):
        one = ops.how_vlad(x[i:i + 1].contiguous(), c)
        assert bool(torch.isfinite(one).all()) and float(one.abs().max()) > 0
        assert _bits_equal(one[0], whole[i])
    del x, whole, one
    torch.cuda.empty_cache()  # 20 GB back to the device for the tests that follow


def _argument_errors(f, with_weights, name, cuda):
    L = _lib.lib()
    hd = _lib.handle(0)
    t = torch.zeros(65536, device=cuda)
    out = torch.full((32768,), 7.0, device=cuda)
    p, po = ctypes.c_void_p(t.data_ptr()), ctypes.c_void_p(out.data_ptr())
    p4, po4 = ctypes.c_void_p(t.data_ptr() + 4), ctypes.c_void_p(out.data_ptr() + 4)

    def call(x=p, b=1, n=4, d=128, c=p, w=p, k=64, o=po):
        if with_weights:
            return f(hd, x, b, n, d, c, w, k, o, None)
        return f(hd, x, b, n, d, c, k, 100.0, o, None)

    for kw in (dict(k=0), dict(k=129), dict(d=0), dict(d=16), dict(d=100), dict(d=288), dict(n=0), dict(n=65536),
               dict(b=-1), dict(x=None), dict(c=None), dict(o=None), dict(x=p4), dict(c=p4), dict(o=po4)):
        assert call(**kw) == _lib.RR_EINVAL, kw
    if with_weights:
        assert call(w=None) == _lib.RR_EINVAL and call(w=p4) == _lib.RR_EINVAL
    assert name.encode() in L.rr_last_error(hd)
    assert call(b=0) == _lib.RR_OK
    torch.cuda.synchronize()
    assert bool((out == 7.0).all())  # out untouched


def test_how_vlad_argument_errors(cuda):
    _argument_errors(_lib.lib().rr_how_vlad, False, "rr_how_vlad", cuda)
    with pytest.raises(ValueError):
        ops.how_vlad(torch.zeros((1, 4, 100), device=cuda), torch.zeros((64, 100), device=cuda))
    with pytest.raises(ValueError):
        ops.how_vlad(torch.zeros((1, 4, 128), device=cuda), torch.zeros((129, 128), device=cuda))
    with pytest.raises(ValueError):
        ops.how_vlad(torch.zeros((1, 4, 256), device=cuda)[:, :, :128], torch.zeros((64, 128), device=cuda))
    assert ops.how_vlad(torch.zeros((0, 4, 128), device=cuda), torch.zeros((64, 128), device=cuda)).shape == (0, 8192)


# ---- rr_how_asmk -----------------------------------------------------------
def _asmk_case(b, n, d, k):
    x, c = _rows(b, n, d, k, ASMK_SEEDS[b, n, d, k])
    rs = np.random.RandomState(77 + k)
    return torch.from_numpy(x), torch.from_numpy(c), torch.from_numpy((0.5 + rs.uniform(0, 1, k)).astype(np.float32))


@pytest.mark.parametrize("b,n,d,k", SHAPES)
def test_how_asmk_vs_float64(cuda, b, n, d, k):
    x, c, w = _asmk_case(b, n, d, k)
    am, tm = how_ref.margins(x, c)
    print(f"how_asmk ({b},{n},{d},{k}) seed {ASMK_SEEDS[b, n, d, k]}: smallest argmin margin {am.min().item():.3e}, "
          f"threshold margin {tm.min().item():.3e}")
    assert int((am < MARGIN).sum()) == 0 and int((tm < MARGIN).sum()) == 0  # the case's condition: no position left out
    r64 = how_ref.asmk(x, c, w, torch.float64)
    xd, cd, wd = x.to(cuda), c.to(cuda), w.to(cuda)
    got = ops.how_asmk(xd, cd, wd)
    assert got.shape == (b, k)
    assert _bits_equal(got, ops.how_asmk(xd, cd, wd))  # reruns
    ones = ops.how_asmk(xd, cd, torch.ones_like(wd)).cpu()  # all-ones weights: the kept counts themselves
    assert torch.equal(ones, r64["count"].float())
    got = got.cpu()
    if n == 1:
        assert float(got.abs().max()) == 0.0  # the std of one value is NaN: nothing is kept
        return
    assert int(r64["count"].sum()) > 0
    err = _row_err(got, r64["asmk"])
    print(f"   kept {int(r64['count'].sum())} of {b * n}; output {err:.3e} of the row norm")
    assert err <= BAR


def test_how_asmk_planted_rows(cuda):
    """Duplicate centroids: everything goes to the lower index, the higher gets
    0.  All positions identical (std 0) and n = 1 (std NaN) give zero rows."""
    b, n, d, k = 2, 49, 128, 64
    x, c = _rows(b, n, d, k, 4243)  # a seed at which a kept position's nearest centroid is centroid 0
    am, tm = how_ref.margins(torch.from_numpy(x[:1]), torch.from_numpy(np.delete(c, [40, k - 1], axis=0)))
    assert am.min().item() >= MARGIN and tm.min().item() >= MARGIN  # apart from the planted ties
    c[k - 1] = c[0]
    c[40] = c[7]
    x[1] = x[1, 5]  # image 1: 49 identical rows
    x, c = torch.from_numpy(x), torch.from_numpy(c)
    w = torch.from_numpy(np.random.RandomState(1).uniform(0.5, 1.5, k).astype(np.float32))
    r64 = how_ref.asmk(x[:1], c, w, torch.float64)
    assert int(r64["count"][0, 0]) > 0 and int(r64["count"][0, k - 1]) == 0
    got = ops.how_asmk(x.to(cuda), c.to(cuda), w.to(cuda)).cpu()
    assert float(got[0, k - 1]) == 0.0 and float(got[0, 40]) == 0.0
    assert torch.equal(got[0], (w.double() * r64["count"][0]).float())
    assert float(got[1].abs().max()) == 0.0
    one = ops.how_asmk(x[:1, :1].contiguous().to(cuda), c.to(cuda), w.to(cuda)).cpu()
    assert float(one.abs().max()) == 0.0


@pytest.mark.parametrize("n,d,k", [(49, 128, 64), (323, 128, 64), (33, 64, 32)])
def test_how_asmk_image_alone_equals_image_in_batch(cuda, n, d, k):
    x, c = _rows(3, n, d, k, 31)
    xd, cd = torch.from_numpy(x).to(cuda), torch.from_numpy(c).to(cuda)
    wd = torch.linspace(0.5, 1.5, k, device=cuda)
    whole = ops.how_asmk(xd, cd, wd)
    assert float(whole.abs().max()) > 0
    for i in range(3):
        assert _bits_equal(ops.how_asmk(xd[i:i + 1].contiguous(), cd, wd)[0], whole[i])
    assert _bits_equal(ops.how_asmk(xd.reshape(3, n, 1, d), cd, wd), whole)


def test_how_asmk_argument_errors(cuda):
    _argument_errors(_lib.lib().rr_how_asmk, True, "rr_how_asmk", cuda)
    z = lambda *s: torch.zeros(s, device=cuda)  # noqa: E731
    with pytest.raises(ValueError):
        ops.how_asmk(z(1, 4, 128), z(64, 128), z(63))
    with pytest.raises(ValueError):
        ops.how_asmk(z(1, 4, 96), z(64, 128), z(64))
    assert ops.how_asmk(z(0, 4, 128), z(64, 128), z(64)).shape == (0, 64)


# ---- models.HOWVLADWrapper / HOWASMKWrapper --------------------------------
@pytest.fixture(scope="module")
def fx():
    return np.load(os.path.join(GOLD, "how.npz"))


@pytest.fixture(scope="module")
def nets(fx):
    """One wrapper per (pooling, conv core) over one reference-shaped
    checkpoint: the trunk under the wrapper's backbone.backbone.{0..7}
    nn.Sequential indices, the head under backbone."""
    inv = {"conv1": "0", "bn1": "1", "layer1": "4", "layer2": "5", "layer3": "6", "layer4": "7"}
    trunk = {}
    for key, v in W.synthetic_resnet_state_dict("resnet101", int(fx["weight_seed"])).items():
        first, rest = key.split(".", 1)
        trunk[f"backbone.backbone.{inv[first]}.{rest}"] = v
    made = {}

    def get(pooling, conv_math):
        if (pooling, conv_math) not in made:
            sd = dict(trunk)
            sd.update({"backbone." + key: v for key, v in W.synthetic_how_head(int(fx["head_seed"]), pooling).items()})
            cls = models.HOWVLADWrapper if pooling == "vlad" else models.HOWASMKWrapper
            made[pooling, conv_math] = cls(8, backbone="resnet101", state_dict=sd, device="cuda:0",
                                           conv_math=conv_math)
        return made[pooling, conv_math]
    return get


@pytest.fixture(scope="module")
def head_refs(fx):
    """float64 and float32 restatements of the head-only cases, computed once."""
    out = {}
    for p in POOLINGS:
        head = W.how_head_from_state_dict(W.synthetic_how_head(int(fx["head_seed"]), p))
        for c in HEAD_CASES:
            x = torch.from_numpy(I.feature_map(11000 + c[1] * c[2], c[0], 2048, c[1], c[2]))
            out[p, c] = (x, how_ref.head_forward(x, head, torch.float64), how_ref.head_forward(x, head, torch.float32))
    return out


@pytest.mark.parametrize("pooling", POOLINGS)
@pytest.mark.parametrize("case", HEAD_CASES)
def test_how_head_vs_reference(cuda, fx, nets, head_refs, pooling, case):
    """local_proj -> pooling -> final_proj -> F.normalize alone on maps where
    every piece matters (test_how_host.py: each degenerate piece moves these
    descriptors by >= 100 x this bar).  Measured on the MI355X: see DESIGN.md,
    "HOW head"."""
    b, h, w = case
    tag = f"{pooling}_head_b{b}_{h}x{w}"
    x4, r64, r32 = head_refs[pooling, case]
    d32 = (r32["out"].double() - r64["out"]).abs().max().item()
    bar = max(2e-6, 4 * d32)
    x = x4.permute(0, 2, 3, 1).contiguous().to(cuda)
    for cm in ("f32", "h2"):
        net = nets(pooling, cm).backbone
        taps = {}
        f = net.head(x, taps=taps)
        got = ops.l2_normalize(f, 1e-12).cpu()
        err = np.abs(got.numpy() - fx[tag + "_out"]).max()
        e64 = (got.double() - r64["out"]).abs().max().item()
        print(f"HOW {tag} {cm}: descriptor max|err| vs the reference {err:.3e}, vs float64 {e64:.3e}; float32 "
              f"restatement vs float64 {d32:.3e}; bar {bar:.3e}")
        taps["desc"] = ops.l2_normalize(taps["local"].reshape(-1, taps["local"].shape[-1]).contiguous(), 1e-12) \
            .view(taps["local"].shape)
        rows = {}
        for key in ("local", "desc", "pooled", "features"):
            e32k = _row_err(r32[key], r64[key])
            rows[key] = (_row_err(taps[key].cpu(), r64[key]), max(BAR, 4 * e32k))
            stored = f"{tag}_{key}"
            if stored in fx.files:
                es = _row_err(taps[key].cpu(), torch.from_numpy(fx[stored]))
                print(f"   {key}: vs the stored reference {es:.3e}, vs float64 {rows[key][0]:.3e}, bar {rows[key][1]:.3e}")
                assert es <= rows[key][1], key
            else:
                print(f"   {key}: vs float64 {rows[key][0]:.3e}, bar {rows[key][1]:.3e}")
        assert got.shape == (b, 2048)
        assert err <= bar
        if case == (1, 5, 9):
            for key, (e, kb) in rows.items():
                assert e <= kb, key


def _e2e_err(net, fx, pooling, tag):
    seed, b, h, w = (int(v) for v in fx[f"{pooling}_{tag}_case"])
    got = net.extract_global_descriptor(I.trunk_input(seed, b, h, w).to("cuda:0")).cpu().numpy()
    assert got.shape == (b, 2048) == (b, net.outputdim)
    return np.abs(got - fx[f"{pooling}_{tag}_out"]).max()


@pytest.mark.parametrize("pooling", POOLINGS)
@pytest.mark.parametrize("tag", ["b2_224", "b1_odd"])
def test_how_vs_reference(cuda, fx, nets, pooling, tag):
    """End to end (wiring).  The bar's float32 term comes from the head
    restatement on the reference trunk's saved x4."""
    tr = np.load(os.path.join(GOLD, "resnet_dolg_v15.npz"))
    head = W.how_head_from_state_dict(W.synthetic_how_head(int(fx["head_seed"]), pooling))
    x4 = torch.from_numpy(tr[tag + "_x4"])
    d32 = (how_ref.head_forward(x4, head, torch.float32)["out"].double() -
           how_ref.head_forward(x4, head, torch.float64)["out"]).abs().max().item()
    bar = max(2e-6, 4 * d32)
    e32 = _e2e_err(nets(pooling, "f32"), fx, pooling, tag)
    eh2 = _e2e_err(nets(pooling, "h2"), fx, pooling, tag)
    print(f"HOW {pooling} {tag}: descriptor max|err| f32 {e32:.3e}  h2 {eh2:.3e}; float32 restatement vs float64 "
          f"{d32:.3e}; bar {bar:.3e}")
    assert e32 <= bar
    assert eh2 <= bar


@pytest.mark.parametrize("pooling", POOLINGS)
def test_how_entry_points_agree(cuda, nets, pooling):
    """forward_test == forward_test_u8 == extract_vectors (batches of 2,
    multi-scale) on 4 images of 96 x 128; forward's logits and the callers'
    local descriptors have their shapes."""
    net = nets(pooling, "h2")
    rs = np.random.RandomState(17)
    imgs = torch.from_numpy(rs.randint(0, 256, size=(4, 96, 128, 3), dtype=np.uint8))
    x = ops.preprocess_u8(imgs.to(cuda))
    xn = x.permute(0, 3, 1, 2).contiguous()
    a = net.forward_test(xn)
    assert a.shape == (4, 2048)
    u8 = net.forward_test_u8(imgs.to(cuda))
    assert _bits_equal(a, u8)
    assert _bits_equal(net.backbone.forward_test_u8(imgs.to(cuda)), u8)  # the model's own, not only the wrapper's
    assert _bits_equal(a, net.extract_global_descriptor(xn)) and _bits_equal(a, net.extract_descriptor(xn))
    assert _bits_equal(extract_vectors(net, [imgs[:2], imgs[2:]], ms=[1], device=cuda, print_freq=0).to(cuda),
                       torch.cat([net.forward_test_u8(imgs[:2].to(cuda)), net.forward_test_u8(imgs[2:].to(cuda))]))
    ms = [1, 2 ** -0.5, 0.5]
    got = extract_vectors(net, [imgs[:2], imgs[2:]], ms=ms, device=cuda, print_freq=0)
    parts = []
    for batch in (imgs[:2], imgs[2:]):
        xb = ops.preprocess_u8(batch.to(cuda))
        acc = None
        for s in ms:
            xs = xb if s == 1 else ops.resize_bilinear(xb, int(96 * s), int(128 * s), scale_factor=s)
            f = net.forward_test_nhwc(xs)
            acc = f.clone() if acc is None else acc.add_(f)
        acc.div_(len(ms))
        parts.append(ops.l2_normalize(acc, 1e-12).cpu())
    assert got.shape == (4, 2048)
    assert _bits_equal(got.cpu(), torch.cat(parts))
    none, logits = net(xn)
    assert none is None and logits.shape == (4, 8) and bool(torch.isfinite(logits).all())
    feats = net.extract_features(xn)
    assert _bits_equal(ops.l2_normalize(feats, 1e-12), a)
    loc = net.extract_local_descriptors(xn)
    assert loc.shape == (4, 3 * 4, 128)
    assert bool(((loc.double().norm(dim=2) - 1.0).abs() < 1e-5).all())


def test_gempcaw_on_how(cuda, nets):
    net = nets("vlad", "h2")
    pw = ConvDimReduction(2048, 256, device=cuda)
    w, b = W.synthetic_linear(256, 2048, 8, scale=1.0 / np.sqrt(2048))
    pw.set_params(w, b)
    ext = GeMPCAw(net, pw)
    rs = np.random.RandomState(31)
    imgs = torch.from_numpy(rs.randint(0, 256, size=(2, 96, 128, 3), dtype=np.uint8)).to(cuda)
    f = ext.forward_test_u8(imgs)
    assert f.shape == (2, 256) == (2, ext.outputdim)
    assert bool(((f.double().norm(dim=1) - 1.0).abs() < 1e-5).all())


def test_get_model_builds_the_four_names(cuda):
    """r101 differs from r50 only in the trunk: the same seed gives the same
    head weights."""
    made = {name: models.get_model(name, 8, seed=5, device="cuda:0") for name in
            ("how_vlad_r50", "how_vlad_r101", "how_asmk_r50", "how_asmk_r101")}
    x = I.trunk_input(3, 1, 64, 96).to(cuda)
    for name, net in made.items():
        assert isinstance(net, models.HOWVLADWrapper if "vlad" in name else models.HOWASMKWrapper)
        assert net.backbone.backbone.name == ("resnet50" if name.endswith("r50") else "resnet101")
        f = net.extract_global_descriptor(x)
        assert f.shape == (1, 2048) == (1, net.outputdim)
        assert abs(float(f.double().norm()) - 1.0) < 1e-5
    for p in POOLINGS:
        a, b = made[f"how_{p}_r50"].backbone, made[f"how_{p}_r101"].backbone
        assert set(a.w) == set(b.w) and all(torch.equal(a.w[key], b.w[key]) for key in a.w)
        assert len(a.backbone.convs) < len(b.backbone.convs)


@pytest.mark.parametrize("pooling", POOLINGS)
def test_how_non_default_widths_match_the_restatement(cuda, pooling):
    """local_dim = 64, num_clusters = 32 on a 5 x 9 map, head only, both cores."""
    cls = models.HOWVLADWrapper if pooling == "vlad" else models.HOWASMKWrapper
    x4 = torch.from_numpy(I.feature_map(12045, 1, 2048, 5, 9))
    x = x4.permute(0, 2, 3, 1).contiguous().to(cuda)
    for cm in ("f32", "h2"):
        net = cls(8, backbone="resnet50", local_dim=64, num_clusters=32, seed=21, device="cuda:0", conv_math=cm)
        head = W.how_head_from_state_dict(W.synthetic_how_head(22, pooling, 64, 32, 8))
        assert all(torch.equal(net.backbone.w[key].cpu(), head[key]) for key in head)
        r64, r32 = how_ref.head_forward(x4, head, torch.float64), how_ref.head_forward(x4, head, torch.float32)
        if pooling == "asmk":
            am, tm = how_ref.margins(r64["local"], head["centroids"])
            assert am.min().item() >= MARGIN and tm.min().item() >= MARGIN
        bar = max(2e-6, 4 * (r32["out"].double() - r64["out"]).abs().max().item())
        got = ops.l2_normalize(net.backbone.head(x), 1e-12).cpu()
        err = (got.double() - r64["out"]).abs().max().item()
        print(f"HOW {pooling} local_dim 64, 32 clusters, {cm}: descriptor vs float64 {err:.3e}; bar {bar:.3e}")
        assert got.shape == (1, 2048) and err <= bar
