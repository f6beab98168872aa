"""The stored-C GEMM epilogue's ragged-shape paths (csrc/gemm_epilogue.hpp
epilogue_store) under every forced tile config of the fp32 core (rr_linear_ex)
and the bf16 core (rr_linear_bf16), against float64.

epilogue_store writes 16-B vectors when N % 4 == 0 and element by element
otherwise.  Every linear in the rest of the suite has N % 4 == 0 and, for
bf16, K % 64 == 0; the product does not: GeMModel's classifier has num_classes
columns, the PCA-whitening apply any width.  Here N in {1, 3, 66, 129, 258,
1001} takes the per-element branch and N in {68, 132, 260} the vector branch
with a ragged last tile, at M = 1 / 130 / 257, with K that ends in a partial
k-tile, under every epilogue flag set the run-time-flag instance (EPI = -1)
can see, for fp32 and bf16 output.

Bars (tests/test_gpu_tile_configs.py's, K <= 320 < its 576): with scale =
sum |x||w| + |bias| + |residual| per output, |y - ref| < 2e-6 scale before the
activation (ReLU is 1-Lipschitz: the same bar after it); QuickGELU is
1.1-Lipschitz: 1.1 2e-6 scale + 2^-21 |ref|; bf16 output adds 2^-8 (|ref| +
that bar).  bf16 operands: the reference is float64 on the bf16-rounded values.

(The bf16-output term was first written 2^-9 |ref|, and every bf16-output case
with more than a handful of outputs failed it at err / bar = 1.75 .. 1.98,
flag set "none" first: bf16 has 8 significand bits, so RNE is off by up to half
a spacing, 2^(e-8) for y in [2^e, 2^(e+1)), i.e. 2^-8 |y| just above a power of
two; 2^-9 |y| is the bound only at the top of a binade.  And the value rounded
is the kernel's y, |y| <= |ref| + bar.  The kernels' stores are RNE:
test_gpu_attention_instances.py and test_gpu_vit.py check them bit for bit
against torch's rounding of the fp32 output.)

y sits between sentinels and bias / residual between NaNs in every call."""
import contextlib
import ctypes
import functools

import pytest
import torch

from research_image_retrieval_amd import _lib, ops

pytestmark = pytest.mark.gpu

# (name, bias, residual, act)
FLAG_SETS = [("none", 0, 0, 0), ("bias", 1, 0, 0), ("bias+res", 1, 1, 0), ("bias+relu", 1, 0, 1),
             ("bias+gelu", 1, 0, 2), ("res", 0, 1, 0), ("bias+res+gelu", 1, 1, 2)]
N_ELEMENT = (1, 3, 66, 129, 258, 1001)  # N % 4 != 0: the per-element branch
N_VECTOR = (68, 132, 260)               # N % 4 == 0, no multiple of a tile width
# (M, N, K): every listed M, N and K appears under every config
F32_SHAPES = [(1, 1, 100), (130, 3, 36), (257, 66, 260), (130, 129, 4), (1, 258, 260), (257, 1001, 100),
              (257, 68, 36), (1, 132, 4), (130, 260, 260)]
BF16_SHAPES = [(1, 1, 200), (130, 3, 72), (257, 66, 264), (130, 129, 8), (1, 258, 320), (257, 1001, 200),
               (257, 68, 72), (1, 132, 8), (130, 260, 320)]
# (K = 320 at N = 258 and N = 260: the 256x256 tile of lp_cfg 3 itself on both epilogue branches)
assert {s[1] for s in F32_SHAPES} == {s[1] for s in BF16_SHAPES} == set(N_ELEMENT + N_VECTOR)
assert {s[0] for s in F32_SHAPES} == {s[0] for s in BF16_SHAPES} == {1, 130, 257}
assert {s[2] for s in F32_SHAPES} == {4, 36, 100, 260} and {s[2] for s in BF16_SHAPES} == {8, 72, 200, 264, 320}
F32_CFGS = [(22, 16), (22, 32), (41, 16), (41, 32), (88, 32), None]  # None: the library's pick
LP_CFGS = [1, 2, 3, 0]                                               # 0: the library's pick
# the persistent-tile boundary (gemm_lpp.hip by default, the one-tile kernel under lp_cfg 3)
LPP_SHAPES = [(1, 256, 320), (257, 256, 320), (1, 512, 320), (257, 512, 320)]

GUARD_VAL = -768.0  # exact in bf16
FRONT, BACK = 72, 264  # guard elements: whole 16-B units for fp32 and bf16, and no more aligned than that


def _p(t):
    return None if t is None else ctypes.c_void_p(t.data_ptr())


def _stream(dev):
    return ctypes.c_void_p(torch.cuda.current_stream(dev).cuda_stream)


def _guarded(t, fill, dev):
    """t's values between FRONT and BACK elements of `fill` on the device: (buffer, view)."""
    buf = torch.full((FRONT + t.numel() + BACK,), fill, dtype=t.dtype, device=dev)
    mid = buf[FRONT:FRONT + t.numel()].view(t.shape)
    mid.copy_(t)
    return buf, mid


def _guards_intact(buf, n, fill):
    g = torch.cat([buf[:FRONT], buf[FRONT + n:]])
    return bool(torch.isnan(g).all()) if fill != fill else bool((g == fill).all())


@functools.lru_cache(maxsize=None)
def _case(m, n, k, bf16):
    """Operands and the float64 pieces of the reference, once per shape."""
    g = torch.Generator().manual_seed(100003 * m + 101 * n + k + int(bf16))
    x = torch.randn(m, k, generator=g)
    w = torch.randn(n, k, generator=g) * k ** -0.5
    bias = torch.randn(n, generator=g)
    res = torch.randn(m, n, generator=g)
    if bf16:
        x, w = x.bfloat16(), w.bfloat16()
    xd, wd = x.double(), w.double()
    return x, w, bias, res, xd @ wd.t(), xd.abs() @ wd.abs().t()


def _ref_and_bar(case, has_bias, has_res, act, out_bf16):
    _, _, bias, res, prod, sprod = case
    z, scale = prod.clone(), sprod.clone()
    if has_bias:
        z += bias.double()
        scale += bias.double().abs()
    if has_res:
        z += res.double()
        scale += res.double().abs()
    ref = torch.relu(z) if act == 1 else z * torch.sigmoid(1.702 * z) if act == 2 else z
    bar = 2e-6 * scale if act != 2 else 1.1 * 2e-6 * scale + 2.0 ** -21 * ref.abs()
    if out_bf16:
        bar = bar + 2.0 ** -8 * (ref.abs() + bar)
    return ref, bar


class _Dev:
    """One shape's operands on the device, bias / residual between NaNs."""

    def __init__(self, case, dev):
        x, w, bias, res = case[:4]
        self.dev, self.m, self.k, self.n = dev, x.shape[0], x.shape[1], w.shape[0]
        self.x, self.w = x.to(dev), w.to(dev)
        self.bbuf, self.bias = _guarded(bias, float("nan"), dev)
        self.rbuf, self.res = _guarded(res, float("nan"), dev)
        self.bf16 = x.dtype == torch.bfloat16

    def run(self, has_bias, has_res, act, out_bf16=False, expect=_lib.RR_OK, m=None, k=None):
        """One call into a fresh sentinel-guarded y; the guards are checked here."""
        dt = torch.bfloat16 if out_bf16 else torch.float32
        ybuf = torch.full((FRONT + self.m * self.n + BACK,), GUARD_VAL, dtype=dt, device=self.dev)
        y = ybuf[FRONT:FRONT + self.m * self.n].view(self.m, self.n)
        L, h = _lib.lib(), _lib.handle(self.dev.index)
        b, r = (self.bias if has_bias else None), (self.res if has_res else None)
        m, k = self.m if m is None else m, self.k if k is None else k
        if self.bf16:
            rc = L.rr_linear_bf16(h, _p(self.x), m, k, _p(self.w), _p(b), self.n, _p(r), act, int(out_bf16), _p(y),
                                  _stream(self.dev))
        else:
            assert not out_bf16
            rc = L.rr_linear_ex(h, _p(self.x), m, k, _p(self.w), _p(b), self.n, _p(r), act, _p(y), _stream(self.dev))
        assert rc == expect, (rc, expect)
        assert _guards_intact(ybuf, self.m * self.n, GUARD_VAL), "y sentinels overwritten"
        assert _guards_intact(self.bbuf, self.n, float("nan")) and _guards_intact(self.rbuf, self.m * self.n,
                                                                                  float("nan"))
        return y


def _check_all_flag_sets(case, d, out_types, tag):
    outs = {}
    for name, hb, hr, act in FLAG_SETS:
        for ob in out_types:
            y = d.run(hb, hr, act, ob)
            ref, bar = _ref_and_bar(case, hb, hr, act, ob)
            err = (y.cpu().double() - ref).abs()
            worst = (err / (bar + 1e-300)).max().item()
            assert bool((err < bar).all()), (tag, name, "bf16 out" if ob else "fp32 out", f"err / bar = {worst:.3f}")
            outs[name, ob] = y
        if len(out_types) == 2:  # the bf16 store is the fp32 result rounded RNE
            assert torch.equal(outs[name, True].view(torch.int16), outs[name, False].bfloat16().view(torch.int16)), \
                (tag, name)
    return outs


@pytest.mark.parametrize("shape", F32_SHAPES, ids=lambda s: "m%d_n%d_k%d" % s)
@pytest.mark.parametrize("cfg", F32_CFGS, ids=lambda c: "pick" if c is None else "cfg%d_bk%d" % c)
def test_f32_linear_ragged_shapes_every_config(cuda, cfg, shape):
    """rr_linear_ex on the forced (gemm_cfg, gemm_bk) tiles and the default
    pick: both epilogue_store branches (N % 4 != 0 and N % 4 == 0 with a
    ragged last tile), M = 1 / 130 / 257, K down to one float4 and ending in a
    partial k-tile, the seven flag sets each."""
    case = _case(*shape, False)
    d = _Dev(case, cuda)
    ctx = contextlib.nullcontext() if cfg is None else ops.tuning(cuda.index, gemm_cfg=cfg[0], gemm_bk=cfg[1])
    with ctx:
        _check_all_flag_sets(case, d, (False,), (cfg, shape))


@pytest.mark.parametrize("shape", BF16_SHAPES, ids=lambda s: "m%d_n%d_k%d" % s)
@pytest.mark.parametrize("cfg", LP_CFGS, ids=lambda c: "lp%d" % c)
def test_bf16_linear_ragged_shapes_every_config(cuda, cfg, shape):
    """rr_linear_bf16 on lp_cfg 1 / 2 / 3 and the default pick, fp32 and bf16
    output: the same N and M as the fp32 core; K in {8, 72, 200, 264} ends in
    a partial 64-deep k-tile (lp_cfg 3 falls to the 128x128 tile there), 320
    does not: N = 258 and N = 260 run the 256x256 tile with a second column
    tile of two and four columns."""
    case = _case(*shape, True)
    d = _Dev(case, cuda)
    with ops.tuning(cuda.index, lp_cfg=cfg):
        _check_all_flag_sets(case, d, (False, True), (cfg, shape))


@pytest.mark.parametrize("shape", LPP_SHAPES, ids=lambda s: "m%d_n%d_k%d" % s)
def test_bf16_linear_persistent_tile_boundary(cuda, shape):
    """N = 256 / 512 at K = 320, one ragged row tile (M = 1) and fewer tiles
    than blocks (M = 257): the default (the persistent k-stream of
    gemm_lpp.hip, at K = 320 its three-A-stage form, for its flag sets: bias -> bf16, bias + residual -> fp32,
    bias + QuickGELU -> bf16) and the one-tile kernel (lp_cfg 3) both meet
    the float64 bar on every flag set and output type, and agree bit for bit
    on the persistent kernel's flag sets."""
    case = _case(*shape, True)
    d = _Dev(case, cuda)
    dflt = _check_all_flag_sets(case, d, (False, True), ("pick", shape))
    with ops.tuning(cuda.index, lp_cfg=3):
        one = _check_all_flag_sets(case, d, (False, True), ("lp3", shape))
    for key in (("bias", True), ("bias+res", False), ("bias+gelu", True)):
        a, b = dflt[key], one[key]
        assert torch.equal(a.view(torch.int16 if key[1] else torch.int32),
                           b.view(torch.int16 if key[1] else torch.int32)), key


def test_linear_argument_checks_and_empty(cuda):
    """m = 0 is RR_OK and writes nothing; k = 6 (fp32), k = 12 (bf16) and
    act = 3 are RR_EINVAL -- y, bias and residual guards intact throughout."""
    for bf16 in (False, True):
        d = _Dev(_case(130, 66, 72, bf16), cuda)
        outs = (False, True) if bf16 else (False,)
        for ob in outs:
            for _, hb, hr, act in FLAG_SETS:
                y = d.run(hb, hr, act, ob, m=0)
                assert bool((y == GUARD_VAL).all())
            y = d.run(1, 1, 0, ob, expect=_lib.RR_EINVAL, k=12 if bf16 else 6)
            assert bool((y == GUARD_VAL).all())
            y = d.run(1, 1, 3, ob, expect=_lib.RR_EINVAL)
            assert bool((y == GUARD_VAL).all())


def test_gem_model_classifier_call_site(cuda):
    """GeMModel(num_classes=1001, feature_dim=130).forward's classifier call,
    ops.linear(feats, cls_w, cls_b) on a 5 x 130 feature matrix, without the
    trunk: N = 1001 stores per element and K = 130 is no multiple of 4.  This
    case exposed a bug: rr_linear returned RR_EINVAL ("rr_linear: bad
    argument") for every k % 4 != 0, so forward() of a GeMModel with such a
    feature_dim raised; rr_linear now runs those on the generic gather."""
    from research_image_retrieval_amd.models import GeMModel
    net = GeMModel(num_classes=1001, feature_dim=130, device=cuda)
    assert tuple(net.cls_w.shape) == (1001, 130) and tuple(net.cls_b.shape) == (1001,)
    feats = torch.randn(5, 130, generator=torch.Generator().manual_seed(130))
    y = ops.linear(feats.to(cuda), net.cls_w, net.cls_b).cpu().double()
    w, b = net.cls_w.cpu().double(), net.cls_b.cpu().double()
    ref = feats.double() @ w.t() + b
    scale = feats.double().abs() @ w.abs().t() + b.abs()
    e = ((y - ref).abs() / scale).max().item()
    assert e < 2e-6, e
    # the same path on the vector epilogue, more than one row tile, no bias, unaligned rows (K = 38 floats)
    x, w = _case(257, 68, 36, False)[:2]
    g = torch.Generator().manual_seed(38)
    x, w = torch.cat([x, torch.randn(257, 2, generator=g)], 1), torch.cat([w, torch.randn(68, 2, generator=g)], 1)
    y = ops.linear(x.to(cuda), w.to(cuda)).cpu().double()
    e = ((y - x.double() @ w.double().t()).abs() / (x.double().abs() @ w.double().abs().t())).max().item()
    assert e < 2e-6, e
