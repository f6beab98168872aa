"""Which fp32, bf16 or fp8 kernel instance serves which GEMM: the table of record.

gemm_route (csrc/gemm_route.hpp) is the one place that decides it, and
rr_gemm_route reports its result without a GPU.  The kernels of one precision
compute the same numbers, so no parity test notices a GEMM that moves from one
to another; this table does.  The expected routes are what the dispatch before
gemm_route launched (its text with recorders for the launch templates, run on
these cases), with one deliberate exception, `test_partial_k_tile_after_the_8_phase_fallback`;
a change here is a deliberate re-routing and wants a measurement.

The GPU tests that force tuning values say in prose which kernel each
parameter set reaches; `test_claims_of_the_gpu_tests` asserts those claims.
"""
import itertools
import json
import os

import pytest

from research_image_retrieval_amd import _lib, ops
from research_image_retrieval_amd import weights as W

R = ops.GemmRoute
B, RES, GELU, BF, ST, LN = ops.EP_BIAS, ops.EP_RES, ops.EP_GELU, ops.EP_BF16, ops.EP_STATS, ops.EP_LNFOLD
# family, cfg, wm, wn, fm, fn, bk, minb, gl, mf16, il, epi
ROUTES = {
    "none": R(-1, 0, 0, 0, 0, 0, 0, 0, 0, 0, 0, -1),
    # the exact-fp32 core (gemm_f32.hip)
    "f32 22, 128x128, BK 16": R(0, 22, 2, 2, 2, 2, 16, 3, 0, 0, 0, -1),
    "f32 41, 256x64, BK 16": R(0, 41, 4, 1, 2, 2, 16, 3, 0, 0, 0, -1),
    "f32 22, 128x128, BK 32": R(0, 22, 2, 2, 2, 2, 32, 2, 0, 0, 0, -1),
    "f32 41, 256x64, BK 32": R(0, 41, 4, 1, 2, 2, 32, 2, 0, 0, 0, -1),
    "f32 88, 256x256, BK 32": R(0, 88, 2, 4, 4, 2, 32, 1, 0, 0, 0, -1),
    # bf16, one tile per block (gemm_lp.hip); "epi x": that flag set compiled in
    "bf16 1, 128x128": R(1, 1, 2, 2, 2, 2, 0, 2, 0, 1, 0, -1),
    "bf16 2, 256x64": R(1, 2, 4, 1, 2, 2, 0, 2, 0, 1, 0, -1),
    "bf16 3, 256x256": R(1, 3, 2, 4, 4, 2, 0, 1, 1, 1, 0, -1),
    "bf16 3, 256x256, IL": R(1, 3, 2, 4, 4, 2, 0, 1, 1, 1, 1, -1),
    "bf16 4, 256x320, 32x32x16": R(1, 4, 4, 2, 2, 5, 0, 1, 1, 0, 0, -1),
    "bf16 4, 256x320, 32x32x16, IL": R(1, 4, 4, 2, 2, 5, 0, 1, 1, 0, 1, -1),
    "bf16 4, 256x320, 16x16x32": R(1, 4, 4, 2, 2, 5, 0, 1, 1, 2, 0, -1),
    "bf16 4, 256x320, 16x16x32, IL": R(1, 4, 4, 2, 2, 5, 0, 1, 1, 2, 1, -1),
    # fp8, one tile per block
    "fp8 1, 128x128": R(1, 1, 2, 2, 2, 2, 0, 2, 0, 0, 0, -1),
    "fp8 2, 256x64": R(1, 2, 4, 1, 2, 2, 0, 2, 0, 0, 0, -1),
    "fp8 3, 256x256": R(1, 3, 2, 4, 4, 2, 0, 1, 1, 0, 0, -1),
    "fp8 3, 256x256, IL": R(1, 3, 2, 4, 4, 2, 0, 1, 1, 0, 1, -1),
    # the other bf16 / fp8 kernels
    "8-phase": R(4, 5, 0, 0, 0, 0, 0, 0, 0, 0, 0, -1),
    "sweep16, 128-B rows": R(5, 4, 0, 0, 0, 0, 0, 0, 0, 0, 0, -1),
    "sweep16, 64-B rows": R(6, 4, 0, 0, 0, 0, 0, 0, 0, 0, 0, -1),
}
for _n, _f in (("qkv", B | BF), ("res", B | RES), ("gelu", B | GELU | BF), ("produce", B | RES | ST), ("fold", B | BF | LN),
               ("fold_gelu", B | GELU | BF | LN)):
    for _t in ("bf16 1, 128x128", "bf16 2, 256x64", "bf16 3, 256x256"):
        ROUTES[f"{_t}, epi {_n}"] = ROUTES[_t]._replace(epi=_f)
    ROUTES[f"k-stream, epi {_n}"] = R(2, 3, 0, 0, 0, 0, 0, 0, 0, 0, 0, _f)
    ROUTES[f"k-stream, 3 A stages, epi {_n}"] = R(3, 3, 0, 0, 0, 0, 0, 0, 0, 0, 0, _f)
# the ViT linears' epilogues, as keyword arguments of ops.gemm_route
EPI = {
    "none": {}, "bias": dict(bias=True), "qkv": dict(bias=True, out_bf16=True), "res": dict(bias=True, residual=True),
    "gelu": dict(bias=True, activation=2, out_bf16=True),
    "produce": dict(bias=True, residual=True, stats_out=True), "fold": dict(bias=True, out_bf16=True, stats_in=True),
    "fold_gelu": dict(bias=True, activation=2, out_bf16=True, stats_in=True),
}


def route(m, n, k, dtype="f32", emode="store", **kw):
    return ops.gemm_route(m, n, k, dtype, emode, **kw)


def check(cases):
    for name, got in cases:
        assert got == ROUTES[name], (name, got)


# ---- the project's own GEMMs -------------------------------------------------------------------

@pytest.mark.parametrize("batch", [1, 64, 256])
def test_vit_b16_block_linears(batch):
    """ViT-B/16 (197 tokens, d = 768, MLP 3072): QKV, out-proj, fc1 and c_proj,
    plain and as the LayerNorm fold's producer (out-proj, c_proj) and consumers
    (QKV, fc1).  K <= 1024 streams with three A stages where the flag set has
    that instance, with two for the fold's consumers; c_proj (K = 3072) runs
    the one-tile kernel, also the last block's (no producer after it)."""
    m = 197 * batch
    bf = lambda n, k, e: route(m, n, k, "bf16", **EPI[e])  # noqa: E731
    check([
        ("k-stream, 3 A stages, epi qkv", bf(2304, 768, "qkv")), ("k-stream, epi fold", bf(2304, 768, "fold")),
        ("k-stream, 3 A stages, epi res", bf(768, 768, "res")), ("k-stream, 3 A stages, epi produce", bf(768, 768, "produce")),
        ("k-stream, 3 A stages, epi gelu", bf(3072, 768, "gelu")), ("k-stream, epi fold_gelu", bf(3072, 768, "fold_gelu")),
        ("bf16 3, 256x256, epi produce", bf(768, 3072, "produce")),
        # the last block's c_proj; one image's 197 rows: the cost model keeps 128x128
        ("bf16 1, 128x128, epi res" if batch == 1 else "bf16 3, 256x256, epi res", bf(768, 3072, "res")),
    ])


def seed_rows(n, k=100):
    """rr_internal.hpp seed_sample_rows"""
    return min(n, max(min(n // 48, 32768), 4096, k))


@pytest.mark.parametrize("nq", [320, 1280])
def test_ranker_gemms(nq):
    """The rankers' seed (E_SCORES_T over the seed sample) and filter GEMMs
    over a 1.6 M-row gallery: C3's exact fp32 sweep (d = 2048) and its
    prefilter's bf16 pass (every row), C4's bf16 ranker (d = 512), C5's fp8
    ranker (d = 2048, row scales)."""
    n = 1_600_000
    s = seed_rows(n)
    assert s == 32768
    big = nq == 1280
    check([
        ("f32 22, 128x128, BK 16", route(s, nq, 2048, emode="scores_t")),
        ("f32 22, 128x128, BK 16" if big else "f32 41, 256x64, BK 16", route(n - s, nq, 2048, emode="filter")),
        # (320 queries on the seed sample: two 256-wide panels of the 8-phase pipeline against one padded 320-wide tile)
        ("bf16 4, 256x320, 32x32x16" if big else "8-phase", route(s, nq, 2048, "bf16", "scores_t")),
        ("sweep16, 128-B rows", route(n, nq, 2048, "bf16", "filter")),
        ("bf16 1, 128x128", route(s, nq, 512, "bf16", "scores_t")),  # (the 32768-row seed sample: 128x128 at both)
        ("bf16 3, 256x256" if big else "bf16 2, 256x64", route(n - s, nq, 512, "bf16", "filter")),
        ("fp8 1, 128x128", route(s, nq, 2048, "fp8", "scores_t", row_scales=True)),
        ("fp8 3, 256x256, IL" if big else "fp8 2, 256x64", route(n - s, nq, 2048, "fp8", "filter", row_scales=True)),
    ])


def f32_conv_gemms(arch, hw):
    """(m per image, cout, k, amode, residual) of the convs networks.ResNet
    issues with conv_math="f32": the stem (generic gather), 1x1 stride-1 convs
    as dense A, everything else as implicit im2col."""
    out = [((hw // 2) ** 2, 64, 147, "conv_generic", False)]
    h = hw // 4
    inpl = 64
    for stage, (planes, blocks) in enumerate(zip((64, 128, 256, 512), W.RESNET_LAYERS[arch])):
        for b in range(blocks):
            stride = 2 if stage > 0 and b == 0 else 1
            ho = h // stride
            out.append((h * h, planes, inpl, "dense", False))                     # conv1 1x1
            out.append((ho * ho, planes, 9 * planes, "conv", False))              # conv2 3x3 (stride on it)
            if b == 0:
                out.append((ho * ho, 4 * planes, inpl, "dense" if stride == 1 else "conv", False))  # downsample
            out.append((ho * ho, 4 * planes, planes, "dense", True))              # conv3 1x1 + identity
            inpl, h = 4 * planes, ho
    return out


F32_CONV_TABLE = {
    # batch: {route name: how many of the trunk's conv GEMMs, R50 / R101}
    1: {"resnet50": {"f32 22, 128x128, BK 32": 53}, "resnet101": {"f32 22, 128x128, BK 32": 104}},
    64: {"resnet50": {"f32 22, 128x128, BK 32": 46, "f32 41, 256x64, BK 32": 7},
         "resnet101": {"f32 22, 128x128, BK 32": 97, "f32 41, 256x64, BK 32": 7}},
}


@pytest.mark.parametrize("arch", ["resnet50", "resnet101"])
@pytest.mark.parametrize("batch", [1, 64])
def test_f32_conv_gemms(arch, batch):
    """The fp32 R50 / R101 trunks at 224 x 224: every conv GEMM runs a BK 32
    tile, 256x64 for the seven GEMMs with 64 output channels at batch 64; 88
    (long K, no residual, a grid that fills the CUs) serves none of them up to
    batch 64."""
    got = {}
    for m, n, k, amode, res in f32_conv_gemms(arch, 224):
        r = route(m * batch, n, k, amode=amode, bias=True, residual=res, activation=1, ldb=(k + 3) // 4 * 4)
        name = next(nm for nm, rt in ROUTES.items() if rt == r)
        got[name] = got.get(name, 0) + 1
        if name.startswith("f32 88"):
            assert amode == "conv" and not res and k >= 1024 and n % 256 == 0
    assert got == F32_CONV_TABLE[batch][arch]


# ---- forced values ------------------------------------------------------------------------------

FORCED_SHAPES = {
    "vit fc1": dict(m=197 * 64, n=3072, k=768, dtype="bf16", bias=True, activation=2, out_bf16=True),
    "bf16 filter, long K": dict(m=1_600_000, n=1280, k=2048, dtype="bf16", emode="filter"),
    "bf16 filter, short K": dict(m=1_567_232, n=1280, k=512, dtype="bf16", emode="filter"),
    "fp8 filter": dict(m=1_567_232, n=1280, k=2048, dtype="fp8", emode="filter", row_scales=True),
    "f32 stored C": dict(m=64 * 196, n=1024, k=2304, dtype="f32", amode="conv", bias=True, activation=1),
}
LP_PRODUCT = list(itertools.product(range(7), (-1, 0, 1, 2), (-1, 0, 1), (-1, 0, 1)))  # lp_cfg, sweep_form, sweep_mf16, sweep_il
F32_PRODUCT = list(itertools.product((0, 22, 41, 88), (0, 16, 32)))                      # gemm_cfg, gemm_bk
# per shape and product, in product order: [[route name, run length], ...]
FORCED = json.load(open(os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden", "gemm_route_forced.json")))


def unroll(runs):
    return [name for name, n in runs for _ in range(n)]


@pytest.mark.parametrize("shape", sorted(FORCED_SHAPES))
def test_forced_values(shape):
    """Every value of the six tuning keys, as the product of the four
    low-precision keys and the product of the two fp32 keys, on five shapes."""
    geo = FORCED_SHAPES[shape]
    want = unroll(FORCED[shape]["lp"])
    assert len(want) == len(LP_PRODUCT) == 252
    for (lp, sf, sm, si), name in zip(LP_PRODUCT, want):
        assert ops.gemm_route(**geo, lp_cfg=lp, sweep_form=sf, sweep_mf16=sm, sweep_il=si) == ROUTES[name], (lp, sf, sm, si, name)
    want = unroll(FORCED[shape]["f32"])
    assert len(want) == len(F32_PRODUCT) == 12
    for (cfg, bk), name in zip(F32_PRODUCT, want):
        assert ops.gemm_route(**geo, gemm_cfg=cfg, gemm_bk=bk) == ROUTES[name], (cfg, bk, name)


# ---- every boundary in the rules ----------------------------------------------------------------

def lin(m, n, k, e="qkv", **kw):
    return route(m, n, k, "bf16", **EPI[e], **kw)


def flt(nq, k, dtype="bf16", m=1_600_000, **kw):
    return route(m, nq, k, dtype, "filter", row_scales=dtype == "fp8", **kw)


BOUNDARIES = [
    # the k-streams: K <= 1024 by default, N % 256, K % 64, the flag sets, split-K / sym
    ("K = 1024 streams", "k-stream, 3 A stages, epi qkv", lambda: lin(12608, 768, 1024)),
    ("K = 1088 does not", "bf16 3, 256x256, epi qkv", lambda: lin(12608, 768, 1088)),
    ("K = 1088 under lp_cfg 6", "k-stream, 3 A stages, epi qkv", lambda: lin(12608, 768, 1088, lp_cfg=6)),
    ("fold at K = 1088 under lp_cfg 6", "bf16 3, 256x256, epi fold", lambda: lin(12608, 768, 1088, "fold", lp_cfg=6)),
    ("fold at K = 1024", "k-stream, epi fold", lambda: lin(12608, 768, 1024, "fold")),
    ("N % 256 != 0", "bf16 3, 256x256, epi qkv", lambda: lin(12608, 768 + 64, 768)),
    ("K % 64 != 0: no stream, no LDS-DMA tile", "bf16 1, 128x128, epi qkv", lambda: lin(12608, 768, 768 + 32)),
    ("k_split: no stream", "bf16 3, 256x256, epi qkv", lambda: lin(12608, 768, 768, k_split=256)),
    ("sym: no stream", "bf16 1, 128x128, epi qkv", lambda: lin(768, 768, 768, sym=True)),
    ("lp_cfg 3: the one-tile kernel", "bf16 3, 256x256, epi gelu", lambda: lin(12608, 3072, 768, "gelu", lp_cfg=3)),
    ("lp_cfg 4 on a stored C is 3", "bf16 3, 256x256, epi gelu", lambda: lin(12608, 3072, 768, "gelu", lp_cfg=4)),
    ("lp_cfg 5 on a stored C is 3", "bf16 3, 256x256, epi gelu", lambda: lin(12608, 3072, 768, "gelu", lp_cfg=5)),
    # every epilogue flag set: compiled in on every tile but the fold's (256-column tile only), else read at run time
    ("flags none", "bf16 3, 256x256", lambda: lin(12608, 768, 768, "none")),
    ("flags bias (fp32 out): no compiled-in set", "bf16 3, 256x256", lambda: lin(12608, 768, 768, "bias")),
    ("flags qkv, 128x128", "bf16 1, 128x128, epi qkv", lambda: lin(12608, 768, 768, "qkv", lp_cfg=1)),
    ("flags res, 256x64", "bf16 2, 256x64, epi res", lambda: lin(12608, 768, 768, "res", lp_cfg=2)),
    ("flags gelu, 128x128", "bf16 1, 128x128, epi gelu", lambda: lin(12608, 768, 768, "gelu", lp_cfg=1)),
    ("flags produce, lp_cfg 1: the fold takes 256x256", "bf16 3, 256x256, epi produce",
     lambda: lin(12608, 768, 768, "produce", lp_cfg=1)),
    ("flags fold, lp_cfg 2: the fold takes 256x256", "bf16 3, 256x256, epi fold", lambda: lin(12608, 768, 768, "fold", lp_cfg=2)),
    ("flags fold_gelu, lp_cfg 3", "bf16 3, 256x256, epi fold_gelu", lambda: lin(12608, 768, 768, "fold_gelu", lp_cfg=3)),
    ("a fold flag set nothing serves (ReLU)", "none",
     lambda: route(12608, 768, 768, "bf16", bias=True, activation=1, out_bf16=True, stats_in=True)),
    ("the fold on a partial k-tile: no instance", "none", lambda: lin(12608, 768, 768 + 32, "fold")),
    # the sweeps: K = 1023 / 1024 cannot be told apart (K % 8), so 1016 / 1024
    ("bf16 filter, K = 1024: sweep16", "sweep16, 128-B rows", lambda: flt(1280, 1024)),
    ("bf16 filter, K = 1016: not sweep16, not the 256x320 tile", "bf16 1, 128x128", lambda: flt(1280, 1016)),
    ("bf16 filter, K = 960: the 256x256 tile", "bf16 3, 256x256", lambda: flt(1280, 960)),
    ("bf16 filter, K = 1024, sweep_form 0: the 256x320 tile", "bf16 4, 256x320, 32x32x16, IL", lambda: flt(1280, 1024, sweep_form=0)),
    ("bf16 filter, K = 1088 (K % 128 != 0), sweep_form 0", "bf16 4, 256x320, 32x32x16, IL", lambda: flt(1280, 1088, sweep_form=0)),
    ("bf16 filter, 768 queries, K % 128 == 0: the 8-phase pick", "8-phase", lambda: flt(768, 2048, sweep_form=0)),
    ("bf16 filter, 768 queries, K % 128 != 0", "bf16 4, 256x320, 32x32x16, IL", lambda: flt(768, 2048 + 64, sweep_form=0)),
    ("bf16 filter, K % 64 != 0, sweep_form 1: 64-B rows", "sweep16, 64-B rows", lambda: flt(1280, 2048 + 32, sweep_form=1)),
    ("bf16 filter, K % 32 != 0, sweep_form 1: not sweep16", "bf16 1, 128x128", lambda: flt(1280, 2048 + 8, sweep_form=1)),
    ("bf16 filter, K % 256 != 0 is nothing to bf16", "sweep16, 128-B rows", lambda: flt(1280, 2048 + 128)),
    ("bf16 filter, aligned16 = 0: no sweep16", "bf16 4, 256x320, 32x32x16, IL", lambda: flt(1280, 2048, aligned16=False)),
    ("bf16 filter, aligned16 = 0, lp_cfg 5: no 8-phase", "bf16 3, 256x256", lambda: flt(1280, 2048, aligned16=False, lp_cfg=5)),
    ("bf16 filter with row scales: no sweep16, no 256x320", "bf16 3, 256x256",
     lambda: route(1_600_000, 1280, 2048, "bf16", "filter", row_scales=True)),
    ("bf16 filter, lda past sweep16's 2^31-byte tile", "bf16 4, 256x320, 32x32x16, IL", lambda: flt(1280, 2048, lda=1 << 22)),
    ("fp8 filter without row scales: the 256x320 pick runs 256x256", "fp8 3, 256x256",
     lambda: route(1_600_000, 1280, 2048, "fp8", "filter")),
    ("fp8 filter, K % 128 != 0", "fp8 1, 128x128", lambda: flt(1280, 2048 + 64, "fp8")),
    ("fp8 filter, lp_cfg 5, K % 256 == 0", "8-phase", lambda: flt(1280, 2048, "fp8", lp_cfg=5)),
    ("fp8 filter, lp_cfg 5, K % 256 != 0", "fp8 3, 256x256, IL", lambda: flt(1280, 2048 + 128, "fp8", lp_cfg=5)),
    ("fp8 filter, sweep_il 0", "fp8 3, 256x256", lambda: flt(1280, 2048, "fp8", sweep_il=0)),
    ("bf16 seed, lp_cfg 5", "8-phase", lambda: route(32768, 1280, 2048, "bf16", "scores_t", lp_cfg=5)),
    ("bf16 seed: no sweep16, no IL", "bf16 4, 256x320, 32x32x16", lambda: route(32768, 1280, 2048, "bf16", "scores_t", sweep_form=1, sweep_il=1)),
    # fp32: t88 = 239 / 240 tiles, 88 under BK 16 and with a residual
    ("t88 = 240", "f32 88, 256x256, BK 32", lambda: route(256 * 60, 1024, 2304, amode="conv")),
    ("t88 = 239", "f32 22, 128x128, BK 32", lambda: route(256 * 239, 256, 2304, amode="conv")),
    ("t88 = 240, one column", "f32 88, 256x256, BK 32", lambda: route(256 * 240, 256, 2304, amode="conv")),
    ("88 needs K >= 1024", "f32 22, 128x128, BK 32", lambda: route(256 * 60, 1024, 1020, amode="dense")),
    ("88 not with a residual", "f32 22, 128x128, BK 32", lambda: route(256 * 60, 1024, 2304, amode="conv", residual=True)),
    ("88 forced with a residual", "f32 88, 256x256, BK 32", lambda: route(256 * 60, 1024, 2304, residual=True, gemm_cfg=88)),
    ("88 forced under gemm_bk 16", "f32 22, 128x128, BK 16", lambda: route(256 * 60, 1024, 2304, gemm_cfg=88, gemm_bk=16)),
    ("88 picked, not under gemm_bk 16", "f32 22, 128x128, BK 16", lambda: route(256 * 60, 1024, 2304, gemm_bk=16)),
    ("88 forced on the generic gather", "f32 22, 128x128, BK 32", lambda: route(256 * 60, 1024, 2304, amode="conv_generic", gemm_cfg=88)),
    ("88 forced on a ranker GEMM", "f32 22, 128x128, BK 16", lambda: route(32768, 1280, 2048, emode="scores_t", gemm_cfg=88)),
    ("88 not with split-K", "f32 22, 128x128, BK 32", lambda: route(256 * 60, 1024, 2304, k_split=1152)),
]


@pytest.mark.parametrize("what,name,call", BOUNDARIES, ids=[b[0] for b in BOUNDARIES])
def test_boundaries(what, name, call):
    assert call() == ROUTES[name]


PARTIAL_K = [(dt, em, k) for dt, ks in (("bf16", (8, 72, 2048 + 8, 2048 + 32)), ("fp8", (16, 2048 + 64))) for em in ("filter", "scores_t")
             for k in ks]


@pytest.mark.parametrize("dtype,emode,k", PARTIAL_K)
def test_partial_k_tile_after_the_8_phase_fallback(dtype, emode, k):
    """The one deliberate change of route.  A forced lp_cfg 5 on a sweep the
    8-phase pipeline does not take falls to config 3, the 256x256 LDS-DMA tile,
    whose staging reads whole 128-byte rows (gemm_lp_kernel glds_tile: no zero
    fill past K).  The dispatch before gemm_route applied its whole-k-tile rule
    only before that fallback and so launched the LDS-DMA tile at bf16 K % 64
    != 0 and fp8 K % 128 != 0; the route applies it after the fallback too:
    config 1, as a forced 3 gives."""
    got = ops.gemm_route(1_600_000, 1280, k, dtype, emode, row_scales=dtype == "fp8", lp_cfg=5, sweep_form=0)
    assert got == ROUTES[f"{dtype} 1, 128x128"]
    assert got == ops.gemm_route(1_600_000, 1280, k, dtype, emode, row_scales=dtype == "fp8", lp_cfg=3, sweep_form=0)
    assert got.gl == 0


def test_no_lds_dma_tile_on_a_partial_k_tile():
    """Whatever the tuning: GL = 1 only with whole k-tiles."""
    for dtype, epr in (("bf16", 64), ("fp8", 128)):
        for k in (epr // 2, epr + 16, 1024 + 16, 2048 + epr // 2):
            for em in ("filter", "scores_t"):
                for lp, sf, sm, si in LP_PRODUCT:
                    r = ops.gemm_route(50432, 1280, k, dtype, em, lp_cfg=lp, sweep_form=sf, sweep_mf16=sm, sweep_il=si)
                    assert r.gl == 0 and r.family in (1, 6), (dtype, k, em, lp, sf, sm, si, r)


# ---- rejections ---------------------------------------------------------------------------------

@pytest.mark.parametrize("bad", [
    dict(dtype="fp8"),                                     # fp8 has no stored-C GEMM
    dict(dtype="bf16", amode="conv"), dict(dtype="fp8", emode="filter", amode="conv_c4"),  # low precision: dense A only
    dict(dtype="bf16", k=2048 + 4), dict(dtype="bf16", lda=2048 + 4), dict(dtype="bf16", ldb=2048 + 4),  # 16 bytes
    dict(dtype="fp8", emode="filter", k=2048 + 8), dict(dtype="fp8", emode="filter", lda=2048 + 8),
    dict(dtype="fp8", emode="filter", ldb=2048 + 8),
    dict(dtype="bf16", emode="scores_t", ldc=12610),       # ldc % 4
    dict(k=2050), dict(lda=2050), dict(ldb=2050), dict(emode="scores_t", ldc=12610),
    dict(amode="conv", k_split=64), dict(emode="filter", k_split=64), dict(emode="scores_t", sym=True),
    dict(amode="conv_generic", sym=True), dict(k_split=48),
    dict(amode="conv", emode="filter"), dict(amode="conv_c4", emode="scores_t"),  # no such mode combination
    dict(m=-1), dict(n=-1), dict(k=0), dict(activation=3),
    dict(gemm_cfg=23), dict(gemm_bk=8), dict(lp_cfg=7), dict(lp_cfg=-1), dict(sweep_form=3), dict(sweep_form=-2),
    dict(sweep_mf16=2), dict(sweep_il=-2),
], ids=str)
def test_rejected(bad):
    ok = dict(m=12608, n=768, k=2048)
    assert ops.gemm_route(**ok).family == 0
    with pytest.raises(ValueError):
        ops.gemm_route(**{**ok, **bad})


def test_entry_null_pointers_and_empty_shapes():
    L = _lib.lib()
    assert L.rr_gemm_route(None, None, None) == _lib.RR_EINVAL
    # nothing to launch (M == 0 or N == 0): the route of the shape
    assert ops.gemm_route(0, 768, 2048) == ROUTES["f32 22, 128x128, BK 32"]
    assert ops.gemm_route(12608, 0, 768, "bf16", "filter") == ROUTES["bf16 1, 128x128"]


def test_tuning_table_is_one():
    """_lib.TUNE_*, ops._TUNE_KEYS and ops._TUNE_DEFAULT are views of _lib.TUNING."""
    assert set(ops._TUNE_KEYS) == set(ops._TUNE_DEFAULT) == set(_lib.TUNING)
    for name, (key, default) in _lib.TUNING.items():
        assert getattr(_lib, "TUNE_" + name.upper()) == key == ops._TUNE_KEYS[name] and ops._TUNE_DEFAULT[name] == default
    assert len({k for k, _ in _lib.TUNING.values()}) == len(_lib.TUNING) == 13


# ---- what the GPU tests say they reach ----------------------------------------------------------

def test_claims_of_the_gpu_tests():
    n = 20000  # test_gpu_rank_limits._nan_case's gallery; the 40-row one runs the same kernels on one tile
    s = seed_rows(n)
    pre = lambda nq, d, em, **t: route(n if em == "filter" else s, nq, d, "bf16", em, **t)  # noqa: E731
    check([
        # test_gpu_rank_limits.py::test_nan_rank_last_prefilter_every_sweep
        ("bf16 1, 128x128", pre(6, 128, "filter", sweep_form=0)), ("bf16 1, 128x128", pre(256, 256, "filter", sweep_form=0)),
        ("sweep16, 128-B rows", pre(6, 128, "filter", sweep_form=1)), ("sweep16, 128-B rows", pre(256, 256, "filter", sweep_form=1)),
        ("sweep16, 64-B rows", pre(6, 128, "filter", sweep_form=2)), ("sweep16, 64-B rows", pre(256, 256, "filter", sweep_form=2)),
        ("bf16 3, 256x256", pre(256, 256, "filter", sweep_form=0, lp_cfg=3)), ("bf16 3, 256x256", pre(256, 256, "scores_t", lp_cfg=3)),
        ("bf16 4, 256x320, 32x32x16, IL", pre(256, 256, "filter", sweep_form=0, lp_cfg=4)),
        ("8-phase", pre(256, 256, "filter", sweep_form=0, lp_cfg=5)), ("8-phase", pre(256, 256, "scores_t", lp_cfg=5)),
        ("bf16 2, 256x64", pre(33, 192, "filter", sweep_form=0, lp_cfg=2)), ("bf16 2, 256x64", pre(33, 192, "scores_t", lp_cfg=2)),
        ("bf16 4, 256x320, 32x32x16", pre(33, 192, "filter", sweep_form=0, lp_cfg=4, sweep_il=0)),
        ("bf16 4, 256x320, 16x16x32", pre(33, 192, "filter", sweep_form=0, lp_cfg=4, sweep_mf16=1, sweep_il=0)),
        ("bf16 4, 256x320, 16x16x32, IL", pre(33, 192, "filter", sweep_form=0, lp_cfg=4, sweep_mf16=1)),
        ("bf16 4, 256x320, 32x32x16", pre(33, 192, "scores_t", lp_cfg=4)),
    ])
    # ::test_nan_rank_last_exact_every_f32_tile, and "the default pick only reaches 22 / 16 at these sizes"
    for em, m in (("scores_t", s), ("filter", n - s)):
        for cfg, bk in ((22, 16), (22, 32), (41, 16), (41, 32)):
            r = route(m, 33, 192, emode=em, gemm_cfg=cfg, gemm_bk=bk)
            assert (r.family, r.cfg, r.bk) == (0, cfg, bk)
        assert route(m, 33, 192, emode=em) == ROUTES["f32 22, 128x128, BK 16"]
    # ::test_nan_rank_last_lowp_every_sweep (rr_cosine_topk_lp: the filter runs over the rows past the seed)
    lp = lambda dt, nq, d, em, **t: route(n - s if em == "filter" else s, nq, d, dt, em, row_scales=dt == "fp8", **t)  # noqa: E731
    check([
        ("bf16 1, 128x128", lp("bf16", 6, 128, "filter", sweep_form=0)), ("bf16 1, 128x128", lp("bf16", 256, 256, "filter", sweep_form=0)),
        ("sweep16, 128-B rows", lp("bf16", 6, 128, "filter", sweep_form=1)), ("sweep16, 64-B rows", lp("bf16", 256, 256, "filter", sweep_form=2)),
        ("8-phase", lp("bf16", 256, 256, "filter", sweep_form=0, lp_cfg=5)),
        ("fp8 1, 128x128", lp("fp8", 6, 128, "filter")), ("fp8 1, 128x128", lp("fp8", 256, 256, "filter")),
        ("fp8 3, 256x256, IL", lp("fp8", 256, 256, "filter", lp_cfg=3)), ("8-phase", lp("fp8", 256, 256, "filter", lp_cfg=5)),
        ("8-phase", lp("fp8", 256, 256, "scores_t", lp_cfg=5)), ("fp8 2, 256x64", lp("fp8", 33, 384, "filter", lp_cfg=2)),
    ])
    # test_gpu_lowp.py::test_lowp_topk_many_queries_vs_dequantised: 1100 queries, 200 k rows, d = 512
    s2 = seed_rows(200_000)
    check([
        ("bf16 3, 256x256", route(200_000 - s2, 1100, 512, "bf16", "filter")),
        ("fp8 3, 256x256, IL", route(200_000 - s2, 1100, 512, "fp8", "filter", row_scales=True)),
        ("8-phase", route(200_000 - s2, 1100, 512, "bf16", "filter", lp_cfg=5)),
        ("8-phase", route(200_000 - s2, 1100, 512, "fp8", "filter", row_scales=True, lp_cfg=5)),
    ])
    # test_gpu_linear_edges.py::test_bf16_linear_ragged_shapes_every_config: lp_cfg 3 falls to 128x128 on a
    # partial 64-deep k-tile; K = 320 at N = 258 / 260 runs the 256x256 tile
    for m, nn, k in ((1, 1, 200), (130, 3, 72), (257, 66, 264), (130, 129, 8), (257, 1001, 200), (257, 68, 72), (1, 132, 8)):
        r = lin(m, nn, k, "qkv", lp_cfg=3)
        assert (r.family, r.cfg, r.gl) == (1, 1, 0), (m, nn, k, r)
    for m, nn, k in ((1, 258, 320), (130, 260, 320)):
        assert lin(m, nn, k, "qkv", lp_cfg=3) == ROUTES["bf16 3, 256x256, epi qkv"]
        assert lin(m, nn, k, "none", lp_cfg=3) == ROUTES["bf16 3, 256x256"]
        for cfg, tile in ((1, "bf16 1, 128x128"), (2, "bf16 2, 256x64")):
            assert lin(m, nn, k, "res", lp_cfg=cfg) == ROUTES[tile + ", epi res"]
    # ::test_bf16_linear_persistent_tile_boundary: the default streams its flag sets (with three A stages:
    # K = 320), lp_cfg 3 is the one-tile kernel; the other flag sets run the one-tile kernel either way
    for m, nn, k in ((1, 256, 320), (257, 256, 320), (1, 512, 320), (257, 512, 320)):
        for e in ("qkv", "res", "gelu"):
            assert lin(m, nn, k, e) == ROUTES[f"k-stream, 3 A stages, epi {e}"]
            assert lin(m, nn, k, e, lp_cfg=3) == ROUTES[f"bf16 3, 256x256, epi {e}"]
        assert lin(m, nn, k, "bias").family == 1 and lin(m, nn, k, "bias", lp_cfg=3) == ROUTES["bf16 3, 256x256"]
    # test_gpu_vit.py::test_linear_bf16_persistent_tile_bit_identical: default / lp_cfg 3 / lp_cfg 6
    for kind, e, nn, k in (("bf16_out", "qkv", 2304, 768), ("gelu", "gelu", 2304, 768), ("res", "res", 768, 768),
                           ("produce", "produce", 768, 768), ("produce_k3072", "produce", 768, 3072),
                           ("fold", "fold", 2304, 768), ("fold_gelu", "fold_gelu", 2304, 768)):
        m = 8037 if nn == 2304 else 30001
        fold = e.startswith("fold")
        stream = f"k-stream, epi {e}" if fold else f"k-stream, 3 A stages, epi {e}"
        assert lin(m, nn, k, e, lp_cfg=3) == ROUTES[f"bf16 3, 256x256, epi {e}"]
        assert lin(m, nn, k, e) == ROUTES[stream if k <= 1024 else f"bf16 3, 256x256, epi {e}"]
        assert lin(m, nn, k, e, lp_cfg=6) == ROUTES[stream]  # (c_proj's K = 3072: lp_cfg 6 streams it)
    # ::test_linear_bf16_ln_produce...: the reference under lp_cfg 3 is the one-tile kernel with bias + residual
    assert lin(394, 768, 768, "res", lp_cfg=3) == ROUTES["bf16 3, 256x256, epi res"]
