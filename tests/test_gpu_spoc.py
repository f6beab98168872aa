"""SpoC on the GPU: rr_spp_max, rr_spoc_refine and rr_linear_groupmax against
torch on the CPU (F.max_pool2d by value; the float64 evaluation of the two
GEMM kernels), and models.SpoCWrapper end to end and head-only against
tests/golden/spoc.npz (the reference's SpoCModel with its ContextualAttention /
SpatialPyramidPooling, make_golden_spoc.py) and the float64 restatement of
tests/spoc_ref.py (pinned to the reference's own output by
tests/test_spoc_host.py).

The kernel bar, per case: max over rows of max|got - ref| / ||ref row||_2 <=
max(1e-6, 4 e32), e32 the same quantity for the float32 torch evaluation of the
same case (computed here and printed), as tests/test_gpu_sos.py.  The
descriptor bar: max(2e-6, 4 x the float32 restatement's distance from the
float64 one).

No new entry uses the per-stream scratch (rr_linear_groupmax does not split k:
an image alone and in a batch give the same bits, asserted below), so there is
no two-stream test here; the head's two rr_linear_splitk calls are covered by
tests/test_gpu_sos.py's."""
import ctypes
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
import spoc_ref  # noqa: E402

BAR = 1e-6
LEVELS = [1, 2, 4]
HEAD_CASES = ((2, 7, 7), (1, 5, 9), (1, 17, 19), (1, 4, 4))


def _row_err(got, ref):
    """max over rows of max|got - ref| / ||ref row||_2"""
    return ((got.double() - ref.double()).abs().amax(dim=-1) / ref.double().norm(dim=-1)).max().item()


def _bits_equal(a, b):
    return a.shape == b.shape and torch.equal(a.contiguous().view(torch.int32), b.contiguous().view(torch.int32))


def _vp(t, off=0):
    return ctypes.c_void_p(t.data_ptr() + off)


# ---- rr_spp_max ----------------------------------------------------------------
# (b, h, w, c, levels): one 16-B group; the 7x7 map at full width (level 4 has 1x1
# windows); floor mode dropping a row and a column; large windows; c no multiple
# of 64 with a wide level-4 row; h and w swapped; many positions; further level
# sets (one level; a level that divides neither side; a repeated level; four
# levels, the last with 1x1 windows)
SPP_CASES = [(1, 4, 4, 4, LEVELS), (2, 7, 7, 2048, LEVELS), (1, 5, 9, 64, LEVELS), (1, 17, 19, 32, LEVELS),
             (3, 4, 7, 132, LEVELS), (1, 7, 4, 8, LEVELS), (1, 32, 32, 256, LEVELS), (1, 7, 9, 64, [1]),
             (1, 7, 9, 64, [3]), (1, 7, 9, 64, [2, 2]), (1, 7, 9, 64, [1, 2, 3, 6])]


def _check_spp(cuda, x_nhwc, levels):
    b, h, w, c = x_nhwc.shape
    want = spoc_ref.spp(x_nhwc.permute(0, 3, 1, 2), levels).transpose(1, 2).contiguous()
    r = spoc_ref.regions(h, w, levels)
    assert ops.spp_regions(h, w, levels) == r == want.shape[1]
    xd = x_nhwc.to(cuda)
    got = ops.spp_max(xd, levels)
    assert got.shape == (b, r, c)
    assert _bits_equal(got, ops.spp_max(xd, levels))  # reruns
    assert torch.equal(got.cpu(), want)


@pytest.mark.parametrize("b,h,w,c,levels", SPP_CASES)
def test_spp_max_equals_max_pool2d(cuda, b, h, w, c, levels):
    rs = np.random.RandomState(1000 * h + 10 * w + c + len(levels))
    _check_spp(cuda, torch.from_numpy(rs.standard_normal((b, h, w, c)).astype(np.float32)), levels)


def test_spp_max_of_all_negative_values(cuda):
    """N(0,1) - 4: a max that started from 0 would return zeros."""
    rs = np.random.RandomState(3)
    x = torch.from_numpy((rs.standard_normal((2, 5, 9, 64)) - 4.0).clip(max=-0.01).astype(np.float32))
    _check_spp(cuda, x, LEVELS)
    assert float(ops.spp_max(x.to(cuda), LEVELS).max()) < 0


def test_spp_max_argument_errors(cuda):
    L = _lib.lib()
    hd = _lib.handle(0)
    t = torch.zeros(8192, device=cuda)
    out = torch.full((8192,), 7.0, device=cuda)
    lv = (ctypes.c_int * 9)(1, 2, 4, 1, 1, 1, 1, 1, 1)
    big = (ctypes.c_int * 3)(1, 2, 8)
    neg = (ctypes.c_int * 3)(1, 0, 2)
    p, po, plv = _vp(t), _vp(out), ctypes.cast(lv, ctypes.c_void_p)

    def call(x=p, b=1, h=7, w=7, c=8, levels=plv, nl=3, o=po):
        return L.rr_spp_max(hd, x, b, h, w, c, levels, nl, o, None)

    for kw in (dict(h=3), dict(w=3), dict(levels=ctypes.cast(big, ctypes.c_void_p)),
               dict(levels=ctypes.cast(neg, ctypes.c_void_p)), dict(c=6), dict(c=0), dict(nl=0), dict(nl=9),
               dict(b=-1), dict(x=None), dict(o=None), dict(levels=None), dict(x=_vp(t, 4)), dict(o=_vp(out, 4)),
               dict(h=0)):
        assert call(**kw) == _lib.RR_EINVAL, kw
    assert b"rr_spp_max" in L.rr_last_error(hd)
    assert call(b=0) == _lib.RR_OK
    torch.cuda.synchronize()
    assert bool((out == 7.0).all())  # untouched
    assert call(nl=8) == _lib.RR_OK  # eight levels is the most
    torch.cuda.synchronize()
    assert ops.spp_max(torch.zeros((0, 4, 4, 8), device=cuda), LEVELS).shape == (0, 21, 8)
    with pytest.raises(ValueError, match="stride should not be zero"):
        ops.spp_max(torch.zeros((1, 3, 4, 8), device=cuda), LEVELS)


# ---- rr_spoc_refine ------------------------------------------------------------
# (m, dc, c): one ragged tile; the 7x7 map of one image and of two at the model's
# widths; the 5x9 map; several row tiles with a ragged last one, dc no multiple
# of 64 and c no multiple of 64; one row, the widest dc, one 16-B group
REFINE_SHAPES = [(2, 32, 64), (49, 512, 2048), (98, 512, 2048), (45, 512, 2048), (323, 96, 132), (1, 2048, 4)]
REFINE_B_ATT = 0.125


def _refine_case(m, dc, c):
    """u ~ N(0,1) x a per-row gain in [0.5, 2); ctx = relu(N(0,1)); w_att zero-sum,
    scaled for logits of about +-2; row 0 is planted at logit +3 and row 1 at -3
    (both with ctx >= 0); w_c ~ N(0,1) / sqrt(dc); bias ~ N(0,1)."""
    rs = np.random.RandomState(100000 * m + 10 * dc + c)
    u = rs.standard_normal((m, c)) * rs.uniform(0.5, 2.0, (m, 1))
    ctx = np.maximum(rs.standard_normal((m, dc)), 0)
    wa = rs.standard_normal(dc)
    wa = (wa - wa.mean()) * (2.0 / np.sqrt(0.34 * dc))
    pos, neg = np.maximum(wa, 0), np.maximum(-wa, 0)
    ctx[0] = (3.0 - REFINE_B_ATT) * pos / (pos @ pos)
    if m > 1:
        ctx[1] = (3.0 + REFINE_B_ATT) * neg / (neg @ neg)
    wc = rs.standard_normal((c, dc)) / np.sqrt(dc)
    bias = rs.standard_normal(c)
    return tuple(torch.from_numpy(v.astype(np.float32)) for v in (u, ctx, wa, wc, bias))


def _refine_ref(u, ctx, wa, wc, bias, dtype):
    a = torch.sigmoid(ctx.to(dtype) @ wa.to(dtype) + REFINE_B_ATT)
    return a.unsqueeze(1) * u.to(dtype) + ctx.to(dtype) @ wc.to(dtype).t() + bias.to(dtype), a


@pytest.mark.parametrize("m,dc,c", REFINE_SHAPES)
def test_spoc_refine_vs_float64(cuda, m, dc, c):
    u, ctx, wa, wc, bias = _refine_case(m, dc, c)
    y64, a64 = _refine_ref(u, ctx, wa, wc, bias, torch.float64)
    y32, a32 = _refine_ref(u, ctx, wa, wc, bias, torch.float32)
    assert abs(float(torch.logit(a64[0])) - 3.0) < 1e-4 and (m == 1 or abs(float(torch.logit(a64[1])) + 3.0) < 1e-4)
    ud, cd, wad, wcd, bd = (t.to(cuda) for t in (u, ctx, wa, wc, bias))
    y, att = ops.spoc_refine(ud, cd, wad, REFINE_B_ATT, wcd, bd, want_att=True)
    assert y.shape == (m, c) and att.shape == (m,) and _bits_equal(ud.cpu(), u)  # out of place: u untouched
    y2, att2 = ops.spoc_refine(ud, cd, wad, REFINE_B_ATT, wcd, bd, want_att=True)
    assert _bits_equal(y, y2) and _bits_equal(att, att2)  # reruns
    assert _bits_equal(y, ops.spoc_refine(ud, cd, wad, REFINE_B_ATT, wcd, bd))  # att = NULL
    inplace = ud.clone()
    got = ops.spoc_refine(inplace, cd, wad, REFINE_B_ATT, wcd, bd, out=inplace)
    assert got is inplace and _bits_equal(inplace, y)  # y = u: the same bits
    y, att = y.cpu(), att.cpu()
    assert bool(torch.isfinite(y).all()) and bool(torch.isfinite(att).all())
    err, e32 = _row_err(y, y64), _row_err(y32, y64)
    ea, ea32 = (att.double() - a64).abs().max().item(), (a32.double() - a64).abs().max().item()
    bar = max(BAR, 4 * e32)
    print(f"spoc_refine ({m},{dc},{c}): y {err:.3e} of the row norm (float32 torch {e32:.3e}, bar {bar:.3e}); att "
          f"{ea:.3e} (float32 torch {ea32:.3e}); a in [{float(a64.min()):.3f}, {float(a64.max()):.3f}]")
    assert err <= bar
    assert ea <= max(BAR, 4 * ea32)


def test_spoc_refine_argument_errors(cuda):
    L = _lib.lib()
    hd = _lib.handle(0)
    t = torch.zeros(65536, device=cuda)
    y = torch.full((4096,), 7.0, device=cuda)
    p, py = _vp(t), _vp(y)
    p4, py4 = _vp(t, 4), _vp(y, 4)

    def call(u=p, ctx=p, m=2, c=8, dc=32, wa=p, wc=p, bias=p, att=None, out=py):
        return L.rr_spoc_refine(hd, u, ctx, m, c, dc, wa, 0.0, wc, bias, att, out, None)

    for kw in (dict(dc=48), dict(dc=0), dict(dc=2080), dict(dc=16), dict(c=6), dict(c=0), dict(m=-1), dict(u=None),
               dict(ctx=None), dict(wa=None), dict(wc=None), dict(bias=None), dict(out=None), dict(u=p4), dict(ctx=p4),
               dict(wa=p4), dict(wc=p4), dict(bias=p4), dict(att=p4), dict(out=py4)):
        assert call(**kw) == _lib.RR_EINVAL, kw
    assert b"rr_spoc_refine" in L.rr_last_error(hd)
    assert call(m=0) == _lib.RR_OK
    torch.cuda.synchronize()
    assert bool((y == 7.0).all())  # untouched
    assert call(dc=2048) == _lib.RR_OK  # the widest dc
    torch.cuda.synchronize()
    e = torch.zeros((0, 8), device=cuda)
    got = ops.spoc_refine(e, torch.zeros((0, 32), device=cuda), t[:32], 0.0, t[:256].view(8, 32), t[:8], want_att=True)
    assert got[0].shape == (0, 8) and got[1].shape == (0,)


# ---- rr_linear_groupmax ----------------------------------------------------------
# (b, r, k, n): one row (rr_linear_ex's result); a 21-region image and two
# 54-region images at the model's widths; ragged k (132 = 4 steps + 4) and n; a
# full 64-row tile; several images with 33 rows; n % 4 != 0 below one tile with a
# ragged k; many images
GROUPMAX_SHAPES = [(1, 1, 64, 8), (1, 21, 2048, 2048), (2, 54, 2048, 2048), (3, 25, 132, 100), (1, 64, 256, 64),
                   (5, 33, 2048, 256), (3, 54, 260, 7), (64, 54, 64, 64)]
COL_TRAP, COL_FIRST, COL_LAST = 0, 1, 2
MEAN_ABS = float(np.sqrt(2.0 / np.pi))  # E|N(0,1)|


@pytest.fixture(scope="module")
def groupmax_cases():
    """Per shape (x, w, bias, the float64 and float32 products [b,r,n]), computed
    once.  x = |N(0,1)|; w ~ N(0,1) / sqrt(k), except three planted columns:
    COL_TRAP w = -1 / sqrt(k) with bias +0.5 (every pre-activation below -0.5:
    with ReLU the result is exactly 0, and a zero pad row would give 0.5; without
    bias and activation it is negative in every row), COL_FIRST w = x[0][0] -
    E|x| (its maximum sits in row 0 of image 0) and COL_LAST w = x[b-1][r-1] -
    E|x| made orthogonal to image 1's row 0 (its maximum sits in row r - 1 of the
    last image).  With b >= 2, image 1's row 0 is then scaled by 1e6."""
    out = {}
    for b, r, k, n in GROUPMAX_SHAPES:
        rs = np.random.RandomState(b + 100 * r + k + n)
        x = np.abs(rs.standard_normal((b, r, k)))
        w = rs.standard_normal((n, k)) / np.sqrt(k)
        bias = rs.standard_normal(n)
        w[COL_TRAP] = -1.0 / np.sqrt(k)
        bias[COL_TRAP] = 0.5
        w[COL_FIRST] = (x[0, 0] - MEAN_ABS) / np.sqrt(k)
        w[COL_LAST] = (x[b - 1, r - 1] - MEAN_ABS) / np.sqrt(k)
        if b >= 2:
            w[COL_LAST] -= (w[COL_LAST] @ x[1, 0]) / (x[1, 0] @ x[1, 0]) * x[1, 0]
            x[1, 0] *= 1e6
        x, w, bias = (torch.from_numpy(v.astype(np.float32)) for v in (x, w, bias))
        out[b, r, k, n] = (x, w, bias, x.double() @ w.double().t(), x @ w.t())
    return out


def _groupmax_ref(p, bias, act):
    y = p if bias is None else p + bias.to(p.dtype)
    return (F.relu(y) if act else y).amax(dim=1)


@pytest.mark.parametrize("b,r,k,n", GROUPMAX_SHAPES)
def test_linear_groupmax_vs_float64(cuda, groupmax_cases, b, r, k, n):
    x, w, bias, p64, p32 = groupmax_cases[b, r, k, n]
    xd, wd, bd = (t.to(cuda) for t in (x, w, bias))
    pre = p64 + bias.double()
    assert float(pre[:, :, COL_TRAP].max()) < -0.5  # the pad-row trap: act(bias) = 0.5 must not win
    assert int(p64[0, :, COL_FIRST].argmax()) == 0 and int(p64[b - 1, :, COL_LAST].argmax()) == r - 1
    assert int(pre[0, :, COL_FIRST].argmax()) == 0 and int(pre[b - 1, :, COL_LAST].argmax()) == r - 1
    assert float(p64[:, :, COL_TRAP].max()) < 0
    for use_bias, act in ((True, 1), (False, 1), (True, 0), (False, 0)):
        r64 = _groupmax_ref(p64, bias if use_bias else None, act)
        r32 = _groupmax_ref(p32, bias if use_bias else None, act)
        got = ops.linear_groupmax(xd, wd, bd if use_bias else None, act=act)
        assert got.shape == (b, n)
        assert _bits_equal(got, ops.linear_groupmax(xd, wd, bd if use_bias else None, act=act))  # reruns
        alone = ops.linear_groupmax(xd[:1].contiguous(), wd, bd if use_bias else None, act=act)
        assert _bits_equal(alone, got[:1])  # no split over k: image 0 alone is image 0 in the batch, to the bit
        got = got.cpu()
        assert bool(torch.isfinite(got).all())
        err, e32 = _row_err(got, r64), _row_err(r32, r64)
        bar = max(BAR, 4 * e32)
        e1 = _row_err(alone.cpu(), r64[:1])
        print(f"linear_groupmax ({b},{r},{k},{n}) bias {use_bias} act {act}: {err:.3e} of the row norm (float32 torch "
              f"{e32:.3e}, bar {bar:.3e}); image 0 alone {e1:.3e}")
        assert err <= bar and e1 <= bar  # every image against its own row norm: image 1's 1e6 row stays its own
        if act == 1:
            assert bool((got[:, COL_TRAP] == 0.0).all())  # exactly 0: no zero pad row took part
        if act == 0 and not use_bias:
            assert bool((got[:, COL_TRAP] < 0).all())  # negative in every row: the max starts at -inf
        # the planted maxima are the planted rows' own products
        lo = 0.0 if act else -np.inf
        first = max(float(p64[0, 0, COL_FIRST] + (bias[COL_FIRST] if use_bias else 0)), lo)
        last = max(float(p64[b - 1, r - 1, COL_LAST] + (bias[COL_LAST] if use_bias else 0)), lo)
        scale0, scale1 = float(r64[0].norm()), float(r64[b - 1].norm())
        assert abs(float(got[0, COL_FIRST]) - first) <= bar * scale0
        assert abs(float(got[b - 1, COL_LAST]) - last) <= bar * scale1
    if (b, r, k, n) == (1, 1, 64, 8):  # one row per image: rr_linear_ex with ReLU, to the bar
        lin = ops.linear_ex(xd.view(1, 64), wd, bd, act=1).cpu()
        r64 = _groupmax_ref(p64, bias, 1)
        bar = max(BAR, 4 * _row_err(_groupmax_ref(p32, bias, 1), r64))
        got = ops.linear_groupmax(xd, wd, bd, act=1).cpu()
        assert _row_err(lin, r64) <= bar and _row_err(got, lin) <= bar


def test_linear_groupmax_argument_errors(cuda):
    L = _lib.lib()
    hd = _lib.handle(0)
    t = torch.zeros(65536, device=cuda)
    y = torch.full((64,), 7.0, device=cuda)
    p, py = _vp(t), _vp(y)
    p4, py4 = _vp(t, 4), _vp(y, 4)

    def call(x=p, b=2, r=4, k=64, w=p, bias=None, n=8, act=0, out=py):
        return L.rr_linear_groupmax(hd, x, b, r, k, w, bias, n, act, out, None)

    for kw in (dict(r=0), dict(r=65), dict(k=6), dict(k=0), dict(act=2), dict(act=-1), dict(n=0), dict(b=-1),
               dict(x=None), dict(w=None), dict(out=None), dict(x=p4), dict(w=p4), dict(bias=p4), dict(out=py4)):
        assert call(**kw) == _lib.RR_EINVAL, kw
    assert b"rr_linear_groupmax" in L.rr_last_error(hd)
    assert call(b=0) == _lib.RR_OK
    torch.cuda.synchronize()
    assert bool((y == 7.0).all())  # untouched
    assert call(r=64, b=1) == _lib.RR_OK  # 64 rows is the most
    torch.cuda.synchronize()
    assert ops.linear_groupmax(torch.zeros((0, 4, 8), device=cuda), torch.zeros((3, 8), device=cuda), None).shape == (0, 3)


# ---- models.SpoCWrapper --------------------------------------------------------
@pytest.fixture(scope="module")
def fx():
    return np.load(os.path.join(GOLD, "spoc.npz"))


@pytest.fixture(scope="module")
def head(fx):
    return W.spoc_head_from_state_dict(W.synthetic_spoc_head(int(fx["head_seed"]), 512, 8))


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
    sd.update({"backbone." + key: v for key, v in W.synthetic_spoc_head(int(fx["head_seed"]), 512, 8).items()})
    made = {}

    def get(conv_math):
        if conv_math not in made:
            made[conv_math] = models.SpoCWrapper(8, backbone="resnet101", state_dict=sd, device="cuda:0",
                                                 conv_math=conv_math)
        return made[conv_math]
    return get


@pytest.fixture(scope="module")
def head_refs(head):
    """float64 and float32 literal restatements of the head-only cases, computed once."""
    out = {}
    for c in HEAD_CASES:
        x = torch.from_numpy(I.feature_map(13000 + c[1] * c[2], c[0], 2048, c[1], c[2]))
        out[c] = (x, spoc_ref.head_forward(x, head, torch.float64), spoc_ref.head_forward(x, head, torch.float32))
    return out


TAPS = ("att", "refined", "pooled", "agg", "hidden", "features")


@pytest.mark.parametrize("case", HEAD_CASES)
def test_spoc_head_vs_reference(cuda, fx, nets, head_refs, case):
    """contextual attention -> pyramid -> aggregation -> feature_proj ->
    F.normalize alone on maps where every piece matters (test_spoc_host.py: each
    degenerate piece moves these descriptors by >= 100 x the bar).  Measured on
    the MI355X: see DESIGN.md, "SpoC head"."""
    b, h, w = case
    tag = f"head_b{b}_{h}x{w}"
    x4, r64, r32 = head_refs[case]
    d32 = (r32["out"].double() - r64["out"]).abs().max().item()
    bar = max(2e-6, 4 * d32)
    x = x4.permute(0, 2, 3, 1).contiguous().to(cuda)
    for cm in ("f32", "h2"):
        net = nets(cm).backbone
        taps = {}
        f = net.head(x, taps=taps)
        got = ops.l2_normalize(f, 1e-12).cpu()
        err = np.abs(got.numpy() - fx[tag + "_out"]).max()
        e64 = (got.double() - r64["out"]).abs().max().item()
        print(f"SpoC {tag} {cm}: descriptor max|err| vs the reference {err:.3e}, vs float64 {e64:.3e}; float32 "
              f"restatement vs float64 {d32:.3e}; bar {bar:.3e}")
        assert taps["pooled"].shape == (b, spoc_ref.regions(h, w, LEVELS), 2048) and taps["att"].shape == (b, h * w)
        rows = {}
        for key in TAPS:
            e32k = _row_err(r32[key], r64[key])
            rows[key] = (_row_err(taps[key].cpu(), r64[key]), max(BAR, 4 * e32k))
            stored = f"{tag}_{key}"
            if stored in fx.files:
                es = _row_err(taps[key].cpu(), torch.from_numpy(fx[stored]))
                print(f"   {key}: vs the stored reference {es:.3e}, vs float64 {rows[key][0]:.3e}, bar {rows[key][1]:.3e}")
                assert es <= rows[key][1], key
            else:
                print(f"   {key}: vs float64 {rows[key][0]:.3e}, bar {rows[key][1]:.3e}")
        if case == (1, 5, 9):
            p64 = torch.from_numpy(fx[tag + "_pooled64"])
            es = _row_err(taps["pooled"][:, :, :64].cpu(), p64)
            kb = max(BAR, 4 * _row_err(r32["pooled"][:, :, :64], r64["pooled"][:, :, :64]))
            print(f"   pooled[..., :64]: vs the stored reference {es:.3e}, bar {kb:.3e}")
            assert es <= kb
            # the kernel's pyramid on the reference's own refined slice IS the reference's pooled slice
            assert torch.equal(ops.spp_max(torch.from_numpy(fx[tag + "_refined64"]).to(cuda), LEVELS).cpu(), p64)
        assert got.shape == (b, 2048)
        assert err <= bar
        if case == (1, 5, 9):
            for key, (e, kb) in rows.items():
                assert e <= kb, key


@pytest.mark.parametrize("tag", ["b2_224", "b1_odd"])
def test_spoc_vs_reference(cuda, fx, nets, head, tag):
    """End to end.  The model's descriptor against the float64 restatement on
    the GPU trunk's OWN x4, at the head bar; its distance to the stored
    reference descriptor is printed and bounded by the triangle inequality:
    the head bar + max|ref64(x4 gpu) - ref64(x4 fixture)| + max|ref64(x4
    fixture) - stored|, all three computed here (the trunk's own error gets no
    invented number)."""
    tr = np.load(os.path.join(GOLD, "resnet_dolg_v15.npz"))
    seed, b, h, w = (int(v) for v in fx[tag + "_case"])
    stored = torch.from_numpy(fx[tag + "_out"]).double()
    f64_fix = spoc_ref.head_forward(torch.from_numpy(tr[tag + "_x4"]), head, torch.float64)["out"]
    t_fix = (f64_fix - stored).abs().max().item()
    for cm in ("f32", "h2"):
        net = nets(cm).backbone
        x = net._input(I.trunk_input(seed, b, h, w).to(cuda))
        x4, x4a = net.trunk_map(x)
        got = ops.l2_normalize(net.head(x4, x4a), 1e-12).cpu().double()
        x4c = x4.permute(0, 3, 1, 2).contiguous().cpu()
        r64, r32 = spoc_ref.head_forward(x4c, head, torch.float64), spoc_ref.head_forward(x4c, head, torch.float32)
        bar = max(2e-6, 4 * (r32["out"].double() - r64["out"]).abs().max().item())
        e_head = (got - r64["out"]).abs().max().item()
        t_trunk = (r64["out"] - f64_fix).abs().max().item()
        dist = (got - stored).abs().max().item()
        print(f"SpoC {tag} {cm}: descriptor vs float64 on the GPU trunk's x4 {e_head:.3e} (bar {bar:.3e}); distance "
              f"to the stored reference {dist:.3e} <= {bar:.3e} + {t_trunk:.3e} (trunk) + {t_fix:.3e} (fixture)")
        assert got.shape == (b, 2048) == (b, nets(cm).outputdim)
        assert _bits_equal(nets(cm).extract_global_descriptor(I.trunk_input(seed, b, h, w).to(cuda)).cpu(),
                           got.float())
        assert e_head <= bar
        assert dist <= bar + t_trunk + t_fix


def test_spoc_entry_points_agree(cuda, nets):
    """forward_test == forward_test_u8 == extract_vectors (batches of 2,
    multi-scale) on 4 images of 224 x 256, whose half-scale map is 4 x 4, the
    smallest the default pyramid takes; forward's logits have their shape; a
    3 x 3 map raises from the head, citing the reference's own error."""
    net = nets("h2")
    rs = np.random.RandomState(17)
    imgs = torch.from_numpy(rs.randint(0, 256, size=(4, 224, 256, 3), dtype=np.uint8))
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
            xs = xb if s == 1 else ops.resize_bilinear(xb, int(224 * s), int(256 * s), scale_factor=s)
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
    with pytest.raises(ValueError, match="stride should not be zero"):  # a 3 x 3 map
        net.backbone.head(torch.zeros((1, 3, 3, 2048), device=cuda))
    with pytest.raises(ValueError, match="stride should not be zero"):  # 48 x 64 pixels (96 x 128 at half scale): 2 x 2
        net.forward_test_nhwc(ops.preprocess_u8(imgs[:1, :48, :64].contiguous().to(cuda)))


@pytest.mark.parametrize("kw", [dict(use_context=False), dict(context_dim=64),
                                dict(feature_dim=132, pyramid_levels=[1, 3])])
def test_spoc_other_heads_match_the_restatement(cuda, kw):
    """use_context=False; context_dim = 64; feature_dim = 132 with pyramid
    levels [1, 3] (16 regions, n % 64 != 0, k = 132 in feature_proj): on a 5 x 9
    map, head only, both cores."""
    x4 = torch.from_numpy(I.feature_map(13045, 1, 2048, 5, 9))
    x = x4.permute(0, 2, 3, 1).contiguous().to(cuda)
    levels = kw.get("pyramid_levels", LEVELS)
    fd = kw.get("feature_dim", 2048)
    head = W.spoc_head_from_state_dict(W.synthetic_spoc_head(22, kw.get("context_dim", 512), 8,
                                                             kw.get("use_context", True), fd))
    r64 = spoc_ref.head_forward(x4, head, torch.float64, levels=levels)
    r32 = spoc_ref.head_forward(x4, head, torch.float32, levels=levels)
    bar = max(2e-6, 4 * (r32["out"].double() - r64["out"]).abs().max().item())
    for cm in ("f32", "h2"):
        net = models.get_spoc_model(8, backbone="resnet50", seed=21, device="cuda:0", conv_math=cm, **kw)
        assert isinstance(net, models.SpoCWrapper) and net.backbone.backbone.name == "resnet50"
        assert all(torch.equal(net.backbone.w[key].cpu(), head[key]) for key in head if key != "att_b")
        taps = {}
        got = ops.l2_normalize(net.backbone.head(x, taps=taps), 1e-12).cpu()
        err = (got.double() - r64["out"]).abs().max().item()
        print(f"SpoC {kw}, {cm}: descriptor vs float64 {err:.3e}; bar {bar:.3e}")
        assert got.shape == (1, fd) == (1, net.outputdim) and err <= bar
        assert taps["pooled"].shape == (1, spoc_ref.regions(5, 9, levels), 2048)
        for key in ("pooled", "agg", "features"):
            assert _row_err(taps[key].cpu(), r64[key]) <= max(BAR, 4 * _row_err(r32[key], r64[key])), key
        if not kw.get("use_context", True):
            assert taps["att"] is None and torch.equal(taps["pooled"].cpu(), r32["pooled"])


def test_spoc_more_than_64_regions_raise(cuda):
    """Levels [1, 2, 4, 8] on an 8 x 8 map give 85 regions: rr_linear_groupmax takes 64."""
    net = models.get_spoc_model(8, backbone="resnet50", pyramid_levels=[1, 2, 4, 8], use_context=False, seed=21,
                                device="cuda:0")
    assert spoc_ref.regions(8, 8, [1, 2, 4, 8]) == 85
    with pytest.raises(ValueError, match="64"):
        net.backbone.head(torch.zeros((1, 8, 8, 2048), device=cuda))
    with pytest.raises(ValueError):
        ops.linear_groupmax(torch.zeros((1, 85, 8), device=cuda), torch.zeros((4, 8), device=cuda), None)
