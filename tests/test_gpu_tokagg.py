"""The token aggregator on the GPU: rr_cls_attn_pool (and rr_linear_splitk_ex,
the split-K linear with a residual) against the float64 evaluation of
tests/tokagg_ref.py (pinned to the reference's own output by
tests/test_tokagg_host.py), and models.TokenWrapper end to end and head-only
against tests/golden/tokagg.npz (the reference's TokenModel with its
TokenAggregator, make_golden_tokagg.py).

The kernel bar, per case: max over rows of max|got - ref| / ||ref row||_2 <=
max(1e-6, 4 e32), e32 the same quantity for the float32 torch evaluation of the
same case (computed here and printed), as tests/test_gpu_sos.py; a row is one
(image, head) row of d values.  p gets the absolute bar max(1e-6, 4 x its
float32 error).  The descriptor bar: max(2e-6, 4 x the float32 restatement's
distance from the float64 one)."""
import ctypes
import math
import os
import sys

import numpy as np
import pytest
import torch
import torch.nn.functional as F

from research_image_retrieval_amd import _lib, models, ops
from research_image_retrieval_amd import weights as W
from research_image_retrieval_amd.extract import extract_vectors

pytestmark = pytest.mark.gpu
HERE = os.path.dirname(os.path.abspath(__file__))
GOLD = os.path.join(HERE, "golden")
sys.path.insert(0, GOLD)
sys.path.insert(0, HERE)
import inputs as I  # noqa: E402
import tokagg_ref  # noqa: E402

BAR = 1e-6
HEADS = 8
# (b, seq, d, heads): one row; two rows; the 7 x 7 map at the defaults; a ragged
# row step, d / 4 below a wave, two heads; the 14 x 14 map; rr_attention's limit;
# d no multiple of 256 with three heads (idle threads in the last step); the
# widest row and every head slot; many images
SHAPES = [(1, 1, 64, 1), (1, 2, 64, 1), (2, 50, 512, 8), (3, 65, 128, 2), (1, 197, 512, 8), (1, 256, 512, 8),
          (1, 50, 192, 3), (2, 17, 1024, 16), (64, 50, 512, 8)]
HEAD_CASES = ((2, 7, 7), (1, 5, 9), (1, 14, 14), (1, 1, 1))


def _row_err(got, ref):
    """max over rows of max|got - ref| / ||ref row||_2"""
    return ((got.double() - ref.double()).abs().amax(dim=-1) / ref.double().norm(dim=-1)).max().item()


def _bits_equal(a, b):
    return a.shape == b.shape and torch.equal(a.contiguous().view(torch.int32), b.contiguous().view(torch.int32))


# ---- rr_cls_attn_pool ----------------------------------------------------------
def _pool_case(b, seq, d, heads, seed=None, shift=0.0):
    """x ~ N(0,1) x a per-row gain in [0.5, 2) (with a shift: 1 + a quarter of
    that); qt_h = N(0,1) / sqrt(d)
    (scores of spread about 1) plus g v / (v . x_j), v = x_j - the rows' mean, for
    one planted row j per (image, head), g chosen for max_j p of about 0.5, 0.8
    or 0.95 in turn, plus shift x the rows' mean direction (every score moves
    by about `shift`)."""
    rs = np.random.RandomState(1000000 * b + 1000 * seq + d + heads if seed is None else seed)
    x = rs.standard_normal((b, seq, d)) * rs.uniform(0.5, 2.0, (b, seq, 1))
    if shift:
        x = 1.0 + 0.25 * x
    qt = rs.standard_normal((b, heads, d)) / np.sqrt(d)
    for i in range(b if seq > 1 else 0):  # one row: nothing to plant
        for h in range(heads):
            j = rs.randint(seq)
            target = (0.5, 0.8, 0.95)[(i + h) % 3]
            g = math.log(max(seq - 1, 1)) + math.log(target / (1 - target)) + 1.0
            dev = x[i, j] - x[i].mean(axis=0)
            qt[i, h] += g * dev / (dev @ x[i, j])
    if shift:
        mu = x.mean(axis=1)
        qt += shift * (mu / (mu * mu).sum(axis=1, keepdims=True))[:, None, :]
    return torch.from_numpy(x.astype(np.float32)), torch.from_numpy(qt.astype(np.float32))


def _check_pool(tag, x, qt, cuda):
    b, seq, d = x.shape
    heads = qt.shape[1]
    o64, p64 = tokagg_ref.cls_attn_pool(x, qt, torch.float64)
    o32, p32 = tokagg_ref.cls_attn_pool(x, qt, torch.float32)
    pm = p64.amax(dim=-1).reshape(-1)
    lo, hi = float((pm >= 0.2).double().mean()), float((pm <= 0.99).double().mean())
    if seq > 2:
        assert lo >= 0.5 and hi >= 0.5, (lo, hi)
    xd, qd = x.to(cuda), qt.to(cuda)
    out, p = ops.cls_attn_pool(xd, qd, want_p=True)
    assert out.shape == (b, heads, d) and p.shape == (b, heads, seq)
    again = ops.cls_attn_pool(xd, qd, want_p=True)
    assert _bits_equal(out, again[0]) and _bits_equal(p, again[1])                 # reruns
    assert _bits_equal(out, ops.cls_attn_pool(xd, qd))                             # p == NULL
    alone = ops.cls_attn_pool(xd[:1].contiguous(), qd[:1].contiguous(), want_p=True)
    assert _bits_equal(alone[0], out[:1]) and _bits_equal(alone[1], p[:1])         # image 0 alone
    out, p = out.cpu(), p.cpu()
    assert bool(torch.isfinite(out).all()) and bool(torch.isfinite(p).all())
    e32, err = _row_err(o32, o64), _row_err(out, o64)
    ep32, ep = (p32.double() - p64).abs().max().item(), (p.double() - p64).abs().max().item()
    bar, barp = max(BAR, 4 * e32), max(BAR, 4 * ep32)
    print(f"cls_attn_pool {tag} ({b},{seq},{d},{heads}): out {err:.3e} (float32 torch {e32:.3e}, bar {bar:.3e}); p "
          f"{ep:.3e} (float32 torch {ep32:.3e}, bar {barp:.3e}); max_j p in [{float(pm.min()):.3f}, "
          f"{float(pm.max()):.3f}], {lo:.2f} >= 0.2, {hi:.2f} <= 0.99")
    assert err <= bar and ep <= barp
    assert float((p.double().sum(dim=-1) - 1).abs().max()) <= 1e-5
    return out, p, err, bar


@pytest.mark.parametrize("b,seq,d,heads", SHAPES)
def test_cls_attn_pool_vs_float64(cuda, b, seq, d, heads):
    x, qt = _pool_case(b, seq, d, heads)
    out, p, _, _ = _check_pool("", x, qt, cuda)
    if seq == 1:  # softmax over one row: p = 1 and out is that row, exactly
        assert bool((p == 1.0).all()) and torch.equal(out[:, 0], x[:, 0])


def test_cls_attn_pool_scores_near_100_stay_finite(cuda):
    """Every score shifted by about +100 (a component of qt along the rows'
    mean): finite and within the bar.  exp(100) is past float32's range, so the
    form without the maximum subtracted overflows (evaluated here, printed)."""
    x, qt = _pool_case(2, 50, 512, 8, seed=78, shift=100.0)
    s = torch.einsum("bhd,bjd->bhj", qt.double(), x.double())
    print(f"scores in [{float(s.min()):.1f}, {float(s.max()):.1f}]")
    assert float(s.min()) > 60 and float(s.max()) > 100
    _, _, err, bar = _check_pool("shift 100", x, qt, cuda)
    naive, _ = tokagg_ref.cls_attn_pool(x, qt, torch.float32, subtract_max=False)
    print(f"   kernel {err:.3e}, bar {bar:.3e}; float32 without the maximum subtracted: "
          f"{int((~torch.isfinite(naive)).sum())} of {naive.numel()} values not finite")
    assert not bool(torch.isfinite(naive).all())


def test_cls_attn_pool_argument_errors(cuda):
    L = _lib.lib()
    hd = _lib.handle(0)
    t = torch.zeros(262144, device=cuda)
    out = torch.full((16384,), 7.0, device=cuda)
    pb = torch.full((4096,), 7.0, device=cuda)
    p, po, pp = (ctypes.c_void_p(v.data_ptr()) for v in (t, out, pb))
    p4, po4, pp4 = (ctypes.c_void_p(v.data_ptr() + 4) for v in (t, out, pb))

    def call(x=p, b=1, seq=4, d=64, qt=p, heads=2, pr=pp, o=po):
        return L.rr_cls_attn_pool(hd, x, b, seq, d, qt, heads, pr, o, None)

    for kw in (dict(d=32), dict(d=0), dict(d=96), dict(d=1088), dict(d=2048), dict(heads=0), dict(heads=17),
               dict(seq=0), dict(seq=257), dict(b=-1), dict(x=None), dict(qt=None), dict(o=None), dict(x=p4),
               dict(qt=p4), dict(o=po4), dict(pr=pp4)):
        assert call(**kw) == _lib.RR_EINVAL, kw
    assert b"rr_cls_attn_pool" in L.rr_last_error(hd)
    assert call(b=0) == _lib.RR_OK
    torch.cuda.synchronize()
    assert bool((out == 7.0).all()) and bool((pb == 7.0).all())  # untouched, by the errors too
    assert call(pr=None) == _lib.RR_OK                            # p is optional
    assert call(seq=256, d=1024, heads=16) == _lib.RR_OK          # every limit at once
    torch.cuda.synchronize()
    assert bool((pb[:4096] == 7.0).sum() == 0) and bool(torch.isfinite(out).all())
    got = ops.cls_attn_pool(torch.zeros((0, 4, 64), device=cuda), torch.zeros((0, 2, 64), device=cuda), want_p=True)
    assert got[0].shape == (0, 2, 64) and got[1].shape == (0, 2, 4)
    # all-zero rows and queries: a uniform softmax over zero rows
    o, pr = ops.cls_attn_pool(torch.zeros((1, 4, 64), device=cuda), torch.zeros((1, 2, 64), device=cuda), want_p=True)
    assert float(o.abs().max()) == 0.0 and bool((pr == 0.25).all())


def test_cls_attn_pool_on_two_streams(cuda):
    """Two calls of different shapes on two streams, enqueued together: each
    result is the bits of the same call alone on the default stream (nothing is
    shared between calls: no scratch)."""
    xa, qa = (t.to(cuda) for t in _pool_case(4, 197, 512, 8))
    xb, qb = (t.to(cuda) for t in _pool_case(3, 65, 128, 2))
    alone_a, alone_b = ops.cls_attn_pool(xa, qa, want_p=True), ops.cls_attn_pool(xb, qb, want_p=True)
    torch.cuda.synchronize(cuda)
    sa, sb = torch.cuda.Stream(cuda), torch.cuda.Stream(cuda)
    with torch.cuda.stream(sa):
        got_a = ops.cls_attn_pool(xa, qa, want_p=True)
    with torch.cuda.stream(sb):
        got_b = ops.cls_attn_pool(xb, qb, want_p=True)
    sa.synchronize()
    sb.synchronize()
    assert all(_bits_equal(u, v) for u, v in zip(got_a + got_b, alone_a + alone_b))


# ---- rr_linear_splitk_ex ---------------------------------------------------------
# (m, k, n): the folded layer's M at the defaults; its linear2 for one image; k no
# multiple of the slice, n % 4 != 0 (the core's scalar store path)
SPLITK_SHAPES = [(64, 4096, 512), (1, 2048, 512), (3, 260, 7)]


@pytest.mark.parametrize("m,k,n", SPLITK_SHAPES)
def test_linear_splitk_ex_vs_float64(cuda, m, k, n):
    """act(row_scale (x w^T) + bias + residual) against float64 torch, the kernel
    bar; without a residual the entry gives rr_linear_splitk's bits."""
    rs = np.random.RandomState(1000 * m + k + n)
    x, w = (torch.from_numpy(rs.standard_normal(sh).astype(np.float32)) for sh in ((m, k), (n, k)))
    bias, res = (torch.from_numpy(rs.standard_normal(sh).astype(np.float32)) for sh in ((n,), (m, n)))
    res = res * float(np.sqrt(k))  # as large as the product
    scale = torch.from_numpy(rs.uniform(0.5, 2.0, m).astype(np.float32))
    xd, wd, bd, rd, sd = (t.to(cuda) for t in (x, w, bias, res, scale))
    for act in (0, 1):
        def ref(dt):
            y = F.linear(x.to(dt), w.to(dt)) * scale.to(dt).unsqueeze(1) + bias.to(dt) + res.to(dt)
            return torch.relu(y) if act else y
        r64, r32 = ref(torch.float64), ref(torch.float32)
        got = ops.linear_splitk(xd, wd, bd, row_scale=sd, act=act, residual=rd)
        assert _bits_equal(got, ops.linear_splitk(xd, wd, bd, row_scale=sd, act=act, residual=rd))
        e32, err = _row_err(r32, r64), _row_err(got.cpu(), r64)
        bar = max(BAR, 4 * e32)
        print(f"linear_splitk_ex ({m},{k},{n}) act {act}: {err:.3e} (float32 torch {e32:.3e}, bar {bar:.3e})")
        assert got.shape == (m, n) and err <= bar
    plain = ops.linear_splitk(xd, wd, bd, row_scale=sd, act=1)
    y = torch.empty_like(plain)
    hd = _lib.handle(0)
    p = lambda t: ctypes.c_void_p(t.data_ptr())  # noqa: E731
    rc = _lib.lib().rr_linear_splitk_ex(hd, p(xd), m, k, p(wd), n, p(sd), p(bd), None, 1, p(y), None)
    torch.cuda.synchronize()
    assert rc == _lib.RR_OK and _bits_equal(y, plain)
    assert _lib.lib().rr_linear_splitk_ex(hd, p(xd), m, 6, p(wd), n, None, None, None, 0, p(y), None) == _lib.RR_EINVAL
    assert b"rr_linear_splitk_ex" in _lib.lib().rr_last_error(hd)
    with pytest.raises(ValueError, match="residual"):
        ops.linear_splitk(xd, wd, bd, residual=rd[:, :-1].contiguous() if n > 1 else rd)


# ---- models.TokenWrapper --------------------------------------------------------
@pytest.fixture(scope="module")
def fx():
    return np.load(os.path.join(GOLD, "tokagg.npz"))


@pytest.fixture(scope="module")
def head(fx):
    return W.tokagg_head_from_state_dict(W.synthetic_tokagg_head(int(fx["head_seed"]), 512, HEADS, 2, 8, 2048))


@pytest.fixture(scope="module")
def nets(fx):
    """One wrapper per conv core over one reference-shaped checkpoint: the
    trunk under the wrapper's backbone.backbone.{0..7} nn.Sequential indices,
    the head under backbone."""
    inv = {"conv1": "0", "bn1": "1", "layer1": "4", "layer2": "5", "layer3": "6", "layer4": "7"}
    sd = {}
    for key, v in W.synthetic_resnet_state_dict("resnet101", int(fx["weight_seed"])).items():
        first, rest = key.split(".", 1)
        sd[f"backbone.backbone.{inv[first]}.{rest}"] = v
    sd.update({"backbone." + key: v for key, v in W.synthetic_tokagg_head(int(fx["head_seed"]), 512, HEADS, 2, 8,
                                                                           2048).items()})
    made = {}

    def get(conv_math):
        if conv_math not in made:
            made[conv_math] = models.TokenWrapper(8, backbone="resnet101", state_dict=sd, device="cuda:0",
                                                  conv_math=conv_math)
        return made[conv_math]
    return get


@pytest.fixture(scope="module")
def head_refs(head):
    """float64 and float32 literal restatements of the head-only cases, computed once."""
    out = {}
    for c in HEAD_CASES:
        x = torch.from_numpy(I.feature_map(13000 + c[1] * c[2], c[0], 2048, c[1], c[2]))
        out[c] = (x, tokagg_ref.head_forward(x, head, HEADS, torch.float64),
                  tokagg_ref.head_forward(x, head, HEADS, torch.float32))
    return out


@pytest.mark.parametrize("case", HEAD_CASES)
def test_tokagg_head_vs_reference(cuda, fx, nets, head_refs, case):
    """input_proj -> tokens -> encoder (last layer folded) -> output_proj ->
    feature_proj -> F.normalize alone on maps where every piece matters
    (test_tokagg_host.py: each degenerate piece moves these descriptors by >=
    100 x the bar), on both conv cores; and the same with the last layer
    unfolded (fold_last=False), held to the same bar and to the folded result.
    Measured on the MI355X: see DESIGN.md, "The token aggregator"."""
    b, h, w = case
    tag = f"head_b{b}_{h}x{w}"
    x4, r64, r32 = head_refs[case]
    d32 = (r32["out"].double() - r64["out"]).abs().max().item()
    bar = max(2e-6, 4 * d32)
    x = x4.permute(0, 2, 3, 1).contiguous().to(cuda)
    for cm in ("f32", "h2"):
        net = nets(cm).backbone
        taps = {}
        got = ops.l2_normalize(net.head(x, taps=taps), 1e-12).cpu()
        unf = ops.l2_normalize(net.head(x, fold_last=False), 1e-12).cpu()
        err = np.abs(got.numpy() - fx[tag + "_out"]).max()
        e64 = (got.double() - r64["out"]).abs().max().item()
        eu, efu = (unf.double() - r64["out"]).abs().max().item(), (unf.double() - got.double()).abs().max().item()
        print(f"TokenModel {tag} {cm}: descriptor max|err| vs the reference {err:.3e}, vs float64 {e64:.3e}; unfolded vs "
              f"float64 {eu:.3e}, vs folded {efu:.3e}; float32 restatement vs float64 {d32:.3e}; bar {bar:.3e}")
        rows = {}
        for key in ("tokens", "layer_out", "p", "pooled", "agg", "features"):
            e32k = _row_err(r32[key], r64[key])
            rows[key] = (_row_err(taps[key].cpu(), r64[key]), max(BAR, 4 * e32k))
            stored = f"{tag}_{'layer0' if key == 'layer_out' else key}"
            if stored in fx.files:
                es = _row_err(taps[key].cpu(), torch.from_numpy(fx[stored]))
                print(f"   {key}: vs the stored reference {es:.3e}, vs float64 {rows[key][0]:.3e}, bar {rows[key][1]:.3e}")
                assert es <= rows[key][1], key
            else:
                print(f"   {key}: vs float64 {rows[key][0]:.3e}, bar {rows[key][1]:.3e}")
        assert got.shape == (b, 2048) and taps["p"].shape == (b, HEADS, 1 + h * w)
        assert err <= bar and e64 <= bar
        assert eu <= bar and efu <= bar
        if case == (1, 5, 9):
            for key, (e, kb) in rows.items():
                assert e <= kb, key


@pytest.mark.parametrize("tag", ["b2_224", "b1_odd"])
def test_tokagg_vs_reference(cuda, fx, nets, head, tag):
    """End to end.  The model's descriptor against the float64 restatement on
    the GPU trunk's OWN x4, at the head bar; its distance to the stored
    reference descriptor is printed and bounded by the triangle inequality:
    the head bar + max|ref64(x4 gpu) - ref64(x4 fixture)| + max|ref64(x4
    fixture) - stored|, all three computed here (as
    test_gpu_sos.py::test_sos_vs_reference)."""
    tr = np.load(os.path.join(GOLD, "resnet_dolg_v15.npz"))
    seed, b, h, w = (int(v) for v in fx[tag + "_case"])
    stored = torch.from_numpy(fx[tag + "_out"]).double()
    f64_fix = tokagg_ref.head_forward(torch.from_numpy(tr[tag + "_x4"]), head, HEADS, torch.float64)["out"]
    t_fix = (f64_fix - stored).abs().max().item()
    for cm in ("f32", "h2"):
        net = nets(cm).backbone
        x = net._input(I.trunk_input(seed, b, h, w).to(cuda))
        x4, x4a = net.trunk_map(x)
        got = ops.l2_normalize(net.head(x4, x4a), 1e-12).cpu().double()
        x4c = x4.permute(0, 3, 1, 2).contiguous().cpu()
        r64 = tokagg_ref.head_forward(x4c, head, HEADS, torch.float64)
        r32 = tokagg_ref.head_forward(x4c, head, HEADS, torch.float32)
        bar = max(2e-6, 4 * (r32["out"].double() - r64["out"]).abs().max().item())
        e_head = (got - r64["out"]).abs().max().item()
        t_trunk = (r64["out"] - f64_fix).abs().max().item()
        dist = (got - stored).abs().max().item()
        print(f"TokenModel {tag} {cm}: descriptor vs float64 on the GPU trunk's x4 {e_head:.3e} (bar {bar:.3e}); "
              f"distance to the stored reference {dist:.3e} <= {bar:.3e} + {t_trunk:.3e} (trunk) + {t_fix:.3e} (fixture)")
        assert got.shape == (b, 2048) == (b, nets(cm).outputdim)
        assert _bits_equal(nets(cm).extract_global_descriptor(I.trunk_input(seed, b, h, w).to(cuda)).cpu(),
                           got.float())
        assert e_head <= bar
        assert dist <= bar + t_trunk + t_fix


def test_tokagg_entry_points_agree(cuda, nets):
    """forward_test == forward_test_u8 == extract_vectors (batches of 2,
    multi-scale) on 4 images of 96 x 128; forward's logits have their shape;
    more than 196 positions raise."""
    net = nets("h2")
    rs = np.random.RandomState(17)
    imgs = torch.from_numpy(rs.randint(0, 256, size=(4, 96, 128, 3), dtype=np.uint8))
    x = ops.preprocess_u8(imgs.to(cuda))
    xn = x.permute(0, 3, 1, 2).contiguous()
    a = net.forward_test(xn)
    assert a.shape == (4, 2048)
    assert bool(((a.double().norm(dim=1) - 1.0).abs() < 1e-5).all())
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
    with pytest.raises(ValueError, match="max_len = 196"):  # a 14 x 15 map
        net.backbone.head(torch.zeros((1, 14, 15, 2048), device=cuda))


@pytest.mark.parametrize("layers,d,heads", [(1, 256, 2), (3, 512, 8)])
def test_tokagg_other_depths_match_the_restatement(cuda, layers, d, heads):
    """num_layers = 1 (the folded layer alone, at head width 128, which
    rr_attention does not take) and num_layers = 3, on a 5 x 9 map, head only,
    both cores."""
    x4 = torch.from_numpy(I.feature_map(13045, 1, 2048, 5, 9))
    x = x4.permute(0, 2, 3, 1).contiguous().to(cuda)
    head = W.tokagg_head_from_state_dict(W.synthetic_tokagg_head(22, d, heads, layers, 8, 2048))
    r64 = tokagg_ref.head_forward(x4, head, heads, torch.float64)
    r32 = tokagg_ref.head_forward(x4, head, heads, torch.float32)
    bar = max(2e-6, 4 * (r32["out"].double() - r64["out"]).abs().max().item())
    for cm in ("f32", "h2"):
        net = models.get_token_model(8, backbone="resnet50", hidden_dim=d, num_heads=heads, num_layers=layers, seed=21,
                                     device="cuda:0", conv_math=cm)
        assert isinstance(net, models.TokenWrapper) and net.backbone.backbone.name == "resnet50"
        assert all(torch.equal(net.backbone.w[key].cpu(), head[key]) for key in head if key != "pe")
        taps = {}
        got = ops.l2_normalize(net.backbone.head(x, taps=taps), 1e-12).cpu()
        err = (got.double() - r64["out"]).abs().max().item()
        print(f"TokenModel {layers} layers, width {d}, {heads} heads, {cm}: descriptor vs float64 {err:.3e}; bar "
              f"{bar:.3e}")
        assert got.shape == (1, 2048) and err <= bar
        assert taps["pooled"].shape == (1, heads, d) and taps["layer_out"].shape == (1, 46, d)
        if layers == 1:
            assert _bits_equal(taps["layer_out"], taps["tokens"])
