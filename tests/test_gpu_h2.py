"""The f16x2 split core (csrc/h2_*.hip; rr_conv2d_h2): the power-of-two
scaled 2-way fp16 split, and fp32-grade accuracy of the convolutions it runs,
measured against float64 next to the exact-fp32 MFMA core and the split-bf16
core on the same inputs (the bar the retired split-bf16 core's tests set:
error relative to sum |a||b| per output, max and mean, at most the exact-fp32
core's), plus the max-|y| records the convs hand to each other.

The reference computes these convolutions in fp32 on the CPU
(networks/backbone.py:60-109, :305-346)."""
import numpy as np
import pytest
import torch
import torch.nn.functional as F

from oracle import embed_ref
from research_image_retrieval_amd import ops
from research_image_retrieval_amd import weights as W
from research_image_retrieval_amd.networks import GeM

pytestmark = pytest.mark.gpu

DESC_TOL = 1e-6  # as tests/test_gpu_embed.py


def _planes_to_f64(p):
    return p.view(torch.float16).double()


def _rel_err(got, ref64, scale64):
    e = (got.double() - ref64).abs() / scale64.clamp_min(1e-300)
    return e.max().item(), e.mean().item()


def test_split2_scaled_pieces(cuda):
    """Each row's scale is a power of two putting its max |w| in [2^14, 2^15);
    w 2^e = p0 + p1 + r with |r| <= 2^-22 |w 2^e| (ulp-level for tiny values);
    padding columns are zero."""
    rs = np.random.RandomState(0)
    rows, k = 37, 300
    w = (rs.standard_normal((rows, k)) * np.exp2(rs.randint(-30, 30, (rows, 1)))).astype(np.float32)
    w[3] = 0.0
    w[5, :7] = [1e-30, -2e-31, 3.4e37, 0.0, -0.0, 1e-3, 7.0]
    planes, isc = ops.split2_f16(torch.from_numpy(w).to(cuda), kpad=320)
    planes, isc = planes.cpu(), isc.cpu().double()
    assert planes.shape == (2, rows, 320) and bool((planes[:, :, k:] == 0).all())
    e = -torch.log2(isc)
    assert torch.equal(e, e.round()), "scales must be powers of two"
    amax = torch.from_numpy(np.abs(w)).double().max(1).values
    live = amax > 0
    sc_max = amax[live] / isc[live]
    assert bool((sc_max >= 2.0 ** 14).all()) and bool((sc_max < 2.0 ** 15).all())
    assert float(isc[3]) == 1.0  # a zero row keeps scale 1
    p = _planes_to_f64(planes[:, :, :k])
    ws = torch.from_numpy(w).double() / isc[:, None]
    r = (p[0] + p[1] - ws).abs()
    # fp16 subnormal quantum 2^-24 bounds the remainder of tiny scaled values
    assert bool((r <= torch.maximum(ws.abs() * 2.0 ** -22, torch.full_like(r, 2.0 ** -25))).all())


def test_amax_record(cuda):
    g = torch.Generator().manual_seed(1)
    x = torch.randn(1000003, generator=g)
    x[12345] = -77.5
    x[999] = float("inf")  # non-finite values are left out
    x[1001] = float("nan")
    rec = ops.amax_records(1, cuda)[0]
    ops.amax_f32(x.to(cuda), rec)
    assert ops.amax_value(rec) == 77.5
    # unaligned start
    rec2 = ops.amax_records(1, cuda)[0]
    ops.amax_f32(x.to(cuda)[1:], rec2)
    assert ops.amax_value(rec2) == 77.5


CONV_SHAPES = [  # b, h, w, cin, cout, k, stride, pad, residual
    (2, 14, 14, 64, 128, 3, 1, 1, False),
    (3, 15, 13, 32, 96, 3, 2, 1, False),
    (2, 28, 28, 64, 256, 1, 2, 0, False),
    (2, 9, 11, 256, 64, 1, 1, 0, True),
    (4, 7, 7, 512, 2048, 1, 1, 0, True),
    (2, 14, 14, 256, 256, 3, 1, 1, True),
    (3, 21, 19, 128, 512, 1, 1, 0, True),
    (4, 28, 28, 64, 64, 1, 1, 0, False),    # dense N = 64, K = 64 (config 15's 256x64 form)
    (3, 28, 30, 256, 64, 1, 1, 0, False),   # dense N = 64, K = 256
    (2, 28, 28, 512, 128, 1, 1, 0, False),  # dense N = 128 (its 256x128 form)
]


def _conv_case(cuda, b, h, w, cin, cout, k, s, p, res, xscale=1.0, seed=0):
    g = torch.Generator().manual_seed(b * h + cin + cout + seed)
    x = torch.relu(torch.randn(b, h, w, cin, generator=g)) * xscale
    wt = torch.randn(cout, k, k, cin, generator=g) * (2.0 / (k * k * cin)) ** 0.5
    bias = torch.randn(cout, generator=g) * 0.1 * xscale
    oh, ow = (h + 2 * p - k) // s + 1, (w + 2 * p - k) // s + 1
    r = torch.randn(b, oh, ow, cout, generator=g) * xscale if res else None
    xn, wn = x.permute(0, 3, 1, 2).double(), wt.permute(0, 3, 1, 2).double()
    conv = F.conv2d(xn, wn, None, s, p).permute(0, 2, 3, 1)
    scale = F.conv2d(xn.abs(), wn.abs(), None, s, p).permute(0, 2, 3, 1)
    ref = torch.relu(conv + bias.double() + (r.double() if res else 0.0))
    return x, wt, bias, r, ref, scale


def _run_h2(cuda, x, wt, bias, r, s, p, y_rec=True):
    xd = x.to(cuda)
    rec = ops.amax_records(2, cuda)
    ops.amax_f32(xd, rec[0])
    y = ops.conv2d_h2(xd, rec[0], ops.H2Conv(wt.to(cuda)), bias.to(cuda), s, p, None if r is None else r.to(cuda),
                      True, rec[1] if y_rec else None)
    return y, rec


@pytest.mark.parametrize("b,h,w,cin,cout,k,s,p,res", CONV_SHAPES)
def test_conv2d_h2_vs_float64(cuda, b, h, w, cin, cout, k, s, p, res):
    x, wt, bias, r, ref, scale = _conv_case(cuda, b, h, w, cin, cout, k, s, p, res)
    y_h2, rec = _run_h2(cuda, x, wt, bias, r, s, p)
    xd, wd = x.to(cuda), wt.to(cuda)
    rd = r.to(cuda) if res else None
    y_f32 = ops.conv2d(xd, wd, bias.to(cuda), s, p, rd, True).cpu()
    y_h2 = y_h2.cpu()
    live = ref > 0
    eh2 = _rel_err(y_h2[live], ref[live], scale[live])
    ef32 = _rel_err(y_f32[live], ref[live], scale[live])
    print(f"conv {b}x{h}x{w}x{cin}->{cout} k{k}s{s}: h2 max {eh2[0]:.3g} mean {eh2[1]:.3g} | "
          f"f32 max {ef32[0]:.3g} mean {ef32[1]:.3g}")
    # mean error at most 1.05x the exact-fp32 core's (+1e-9); max within 1.25x of it: the
    # one-accumulator tiles the library picks for K >= 256, N % 256 == 0
    # (configs 10-12) round the a0b1 + a1b0 terms against the running sum, three
    # roundings per product instead of one, measured up to 1.2x the exact core's
    # max error at a lower mean (profiles/r03j_acc1_ab.txt)
    assert eh2[0] <= 1.25 * max(ef32[0], 1e-7) and eh2[1] <= ef32[1] * 1.05 + 1e-9
    # the output's max-|y| record holds exactly max |y|
    assert ops.amax_value(rec[1]) == float(y_h2.abs().max())


@pytest.mark.parametrize("xscale", [2.0 ** -60, 2.0 ** 50, 3.0e-7])
def test_conv2d_h2_scale_invariant(cuda, xscale):
    """The split scales follow the data: activations and residuals at 2^-60 or
    2^50 (far outside fp16's range) keep the same relative accuracy, and a
    power-of-two input scale scales the output exactly."""
    shape = (2, 14, 14, 256, 256, 3, 1, 1, True)
    x, wt, bias, r, ref, scale = _conv_case(cuda, *shape, xscale=xscale, seed=11)
    y, _ = _run_h2(cuda, x, wt, bias, r, 1, 1, y_rec=False)
    live = ref > 0
    e = _rel_err(y.cpu()[live], ref[live], scale[live])
    print(f"xscale {xscale:g}: h2 max {e[0]:.3g} mean {e[1]:.3g}")
    assert e[0] < 4e-7
    if xscale in (2.0 ** -60, 2.0 ** 50):
        x1, _, b1, r1, _, _ = _conv_case(cuda, *shape, xscale=1.0, seed=11)
        y1, _ = _run_h2(cuda, x1, wt, b1, r1, 1, 1, y_rec=False)
        assert torch.equal(y.cpu(), y1.cpu() * xscale)


@pytest.mark.parametrize("b,h,w", [(2, 224, 224), (3, 37, 53)])
def test_stem_h2_vs_float64(cuda, b, h, w):
    """The NHWC4 stem (7x7/2, pad 3, K padded to 224) on the f16x2 core."""
    g = torch.Generator().manual_seed(b * h + w)
    x = torch.randn(b, h, w, 3, generator=g) * 1.5
    x4 = F.pad(x, (0, 1)).contiguous()
    wt = torch.randn(64, 7, 7, 3, generator=g) * (2.0 / 147) ** 0.5
    w4 = F.pad(wt, (0, 1)).contiguous()
    bias = torch.randn(64, generator=g) * 0.1
    xn, wn = x.permute(0, 3, 1, 2).double(), wt.permute(0, 3, 1, 2).double()
    ref = torch.relu(F.conv2d(xn, wn, None, 2, 3).permute(0, 2, 3, 1) + bias.double())
    scale = F.conv2d(xn.abs(), wn.abs(), None, 2, 3).permute(0, 2, 3, 1)
    y_h2, _ = _run_h2(cuda, x4, w4, bias, None, 2, 3)
    y_h2 = y_h2.cpu()
    y_f32 = ops.conv2d(x4.to(cuda), w4.to(cuda), bias.to(cuda), 2, 3, None, True).cpu()
    assert y_h2.shape == ref.shape
    live = ref > 0
    eh2 = _rel_err(y_h2[live], ref[live], scale[live])
    ef32 = _rel_err(y_f32[live], ref[live], scale[live])
    print(f"stem {b}x{h}x{w}: h2 max {eh2[0]:.3g} mean {eh2[1]:.3g} | f32 max {ef32[0]:.3g} mean {ef32[1]:.3g}")
    # mean error at most 1.05x the exact-fp32 core's (+1e-9); max within 1.25x of it: the
    # one-accumulator tiles the library picks for K >= 256, N % 256 == 0
    # (configs 10-12) round the a0b1 + a1b0 terms against the running sum, three
    # roundings per product instead of one, measured up to 1.2x the exact core's
    # max error at a lower mean (profiles/r03j_acc1_ab.txt)
    assert eh2[0] <= 1.25 * max(ef32[0], 1e-7) and eh2[1] <= ef32[1] * 1.05 + 1e-9


TILE_SHAPES = [  # shapes that reach each f16x2 config's edges: ragged M, N = 64 / 96 / 128 / 256k
    (2, 9, 11, 256, 64, 1, 1, 0, True),
    (3, 15, 13, 32, 96, 3, 2, 1, False),
    (2, 14, 14, 64, 128, 3, 1, 1, False),
    (3, 21, 19, 128, 512, 1, 1, 0, True),
    (2, 14, 14, 256, 256, 3, 1, 1, True),
]


@pytest.mark.parametrize("cfg", [3, 4, 7, 8, 9, 10, 11, 12, 13, 14])
@pytest.mark.parametrize("b,h,w,cin,cout,k,s,p,res", TILE_SHAPES)
def test_conv2d_h2_tile_configs(cuda, cfg, b, h, w, cin, cout, k, s, p, res):
    """Every f16x2 tile config forced on every shape: fp32-grade vs float64
    (configs that do not serve a shape fall back to the pick)."""
    x, wt, bias, r, ref, scale = _conv_case(cuda, b, h, w, cin, cout, k, s, p, res, seed=cfg)
    with ops.tuning(0, s3_cfg=cfg):
        y, rec = _run_h2(cuda, x, wt, bias, r, s, p)
    y = y.cpu()
    live = ref > 0
    e = _rel_err(y[live], ref[live], scale[live])
    assert e[0] < 4e-7, (cfg, e)
    assert ops.amax_value(rec[1]) == float(y.abs().max())


HALO_SHAPES = [  # stride-1 3x3, Cin % 32 == 0, N % 256 == 0, W <= 15: config 13 serves these
    (2, 14, 14, 256, 256, 3, 1, 1, False),
    (3, 7, 7, 512, 512, 3, 1, 1, True),
    (2, 15, 15, 256, 256, 3, 1, 1, True),   # the widest map the 288-row halo holds
    (1, 13, 11, 64, 512, 3, 1, 1, False),   # odd sizes, two Cin slices
    (5, 14, 14, 32, 256, 3, 1, 1, False),   # one Cin slice, ragged M (980 rows)
    (2, 28, 28, 128, 128, 3, 1, 1, False),  # the 256x128 instance (halo 320 rows)
    (1, 27, 31, 64, 128, 3, 1, 1, True),    # its widest map
    (1, 56, 56, 64, 64, 3, 1, 1, False),    # the 256x64 instance (halo 384 rows)
    (1, 9, 63, 32, 64, 3, 1, 1, True),      # its widest map
]


@pytest.mark.parametrize("cfg", [13, 14])
@pytest.mark.parametrize("b,h,w,cin,cout,k,s,p,res", HALO_SHAPES)
def test_conv2d_h2_halo(cuda, cfg, b, h, w, cin, cout, k, s, p, res):
    """Config 13 (halo-staged A: each input pixel fetched once per Cin slice,
    taps read from the LDS halo, zero row for padding taps and rows past M):
    the same accuracy bar as every f16x2 conv against float64 and the
    exact-fp32 core, and the max-|y| record exact."""
    x, wt, bias, r, ref, scale = _conv_case(cuda, b, h, w, cin, cout, k, s, p, res, seed=13)
    # config 14: the same tile on v_mfma_f32_16x16x32_f16 (four 16x16 sub-tiles per 32x32 tile)
    with ops.tuning(0, s3_cfg=cfg):
        y, rec = _run_h2(cuda, x, wt, bias, r, s, p)
    y = y.cpu()
    rd = r.to(cuda) if res else None
    y_f32 = ops.conv2d(x.to(cuda), wt.to(cuda), bias.to(cuda), s, p, rd, True).cpu()
    live = ref > 0
    e = _rel_err(y[live], ref[live], scale[live])
    ef32 = _rel_err(y_f32[live], ref[live], scale[live])
    print(f"halo cfg {cfg} {b}x{h}x{w}x{cin}->{cout}: max {e[0]:.3g} mean {e[1]:.3g} | f32 max {ef32[0]:.3g} "
          f"mean {ef32[1]:.3g}")
    assert e[0] <= 1.25 * max(ef32[0], 1e-7) and e[1] <= ef32[1] * 1.05 + 1e-9
    assert ops.amax_value(rec[1]) == float(y.abs().max())
    assert bool(torch.isfinite(y).all())


def test_h2_persistent_tile_bit_identical(cuda):
    """Config 8 (persistent k-stream), config 9 (three LDS stages) and config
    4 keep the same per-accumulator k order and epilogue arithmetic:
    identical bits (1x1 with residual; 3x3 for config 9)."""
    x, wt, bias, r, _, _ = _conv_case(cuda, 3, 29, 31, 256, 1024, 1, 1, 0, True, seed=5)
    outs = {}
    for cfg in (4, 8, 9):
        with ops.tuning(0, s3_cfg=cfg):
            outs[cfg] = _run_h2(cuda, x, wt, bias, r, 1, 0)[0].cpu()
    assert torch.equal(outs[4], outs[8]) and torch.equal(outs[4], outs[9])
    x, wt, bias, r, _, _ = _conv_case(cuda, 2, 15, 13, 256, 256, 3, 1, 1, False, seed=6)
    y9 = {}
    for cfg in (4, 9):
        with ops.tuning(0, s3_cfg=cfg):
            y9[cfg] = _run_h2(cuda, x, wt, bias, None, 1, 1)[0].cpu()
    assert torch.equal(y9[4], y9[9])


@pytest.mark.parametrize("b,h,w,cin,cout,res,relu", [
    (10, 56, 56, 256, 1024, True, True),   # the residual expansion shape: 490 tiles, ~2 per block, ragged M
    (4, 67, 67, 256, 1024, True, False),   # residual without ReLU, ragged
    (5, 80, 80, 1024, 512, False, True),   # K = 1024 reduction, 250 x 2 tiles
    (2, 9, 11, 288, 256, True, True),      # K = 288: nine k-tiles, one tile (an odd stream length)
    (1, 3, 5, 512, 256, False, False),     # one partial tile, no epilogue options
])
def test_h2_persistent_256_tile_bit_identical(cuda, b, h, w, cin, cout, res, relu):
    """Config 15 (config 12 as a persistent k-stream, four-slab epilogue with
    the residual two bands ahead) keeps config 12's per-accumulator k order and
    epilogue arithmetic: identical bits and the same max-|y| record, with
    several tiles per block (the stream across tile boundaries) and ragged M."""
    x, wt, bias, r, _, _ = _conv_case(cuda, b, h, w, cin, cout, 1, 1, 0, res, seed=17)
    xd, rd = x.to(cuda), (r.to(cuda) if res else None)
    cw = ops.H2Conv(wt.to(cuda))
    outs, amax = {}, {}
    for cfg in (12, 15):  # 15 with a residual: sc1 output stores, nt residual loads
        rec = ops.amax_records(2, cuda)
        ops.amax_f32(xd, rec[0])
        with ops.tuning(0, s3_cfg=cfg):
            y = ops.conv2d_h2(xd, rec[0], cw, bias.to(cuda), 1, 0, rd, relu, rec[1])
        outs[cfg], amax[cfg] = y.cpu(), ops.amax_value(rec[1])
    assert torch.equal(outs[12], outs[15])
    assert amax[12] == amax[15] == float(outs[15].abs().max())


@pytest.mark.parametrize("b,h,w,cin,res,relu,nout", [
    (6, 28, 28, 512, False, True, 128),   # the R101 512->128 reduction shape: 19 tiles, ragged M
    (5, 80, 80, 256, True, True, 128),    # 125 tiles, several per block, residual (sc1 / nt)
    (2, 9, 11, 288, True, False, 128),    # K = 288: nine k-tiles, one partial tile
    (1, 3, 5, 1024, False, False, 128),   # one partial tile, no epilogue options
    (6, 56, 56, 64, False, True, 64),     # the R101 64->64 stage-1 shape: K = 64, 74 tiles, ragged
    (4, 56, 56, 256, False, True, 64),    # 256->64
    (9, 64, 64, 96, True, True, 64),      # K = 96: three k-tiles, residual, 144 tiles
    (1, 3, 5, 64, True, False, 64),       # one partial tile
])
def test_h2_persistent_narrow_tile_bit_identical(cuda, b, h, w, cin, res, relu, nout):
    """The 256x128 form of config 15 (the pick for dense N = 128, K >= 256)
    computes each output column with config 12's products in config 12's
    order: a 128-channel layer equals the first 128 channels of the same layer
    at 256 channels on config 12 (per-channel weight scales: the sliced planes
    are the same), bit for bit.  The 256x64 form (dense N = 64, K >= 64) keeps
    config 7's two accumulator sets and k order: the same layer on config 7,
    bit for bit.  Both max-|y| records exact."""
    x, wt, bias, r, _, _ = _conv_case(cuda, b, h, w, cin, 256, 1, 1, 0, res, seed=19)
    xd = x.to(cuda)
    rec = ops.amax_records(3, cuda)
    ops.amax_f32(xd, rec[0])
    rn = r[..., :nout].contiguous().to(cuda) if res else None
    wn, bn = ops.H2Conv(wt[:nout].contiguous().to(cuda)), bias[:nout].contiguous().to(cuda)
    if nout == 64:
        with ops.tuning(0, s3_cfg=7):
            ref = ops.conv2d_h2(xd, rec[0], wn, bn, 1, 0, rn, relu, rec[1]).cpu()
    else:
        with ops.tuning(0, s3_cfg=12):
            ref = ops.conv2d_h2(xd, rec[0], ops.H2Conv(wt.to(cuda)), bias.to(cuda), 1, 0,
                                r.to(cuda) if res else None, relu, rec[1]).cpu()[..., :nout]
    yn = ops.conv2d_h2(xd, rec[0], wn, bn, 1, 0, rn, relu, rec[2]).cpu()
    assert torch.equal(yn, ref)
    assert ops.amax_value(rec[2]) == float(yn.abs().max())


@pytest.mark.parametrize("b,h,w,cin,cout,k,s,p,res,cfg", [
    (3, 29, 31, 256, 1024, 1, 1, 0, True, 12),   # 1x1 + residual (dense A), ragged last tile
    (2, 14, 14, 1024, 256, 1, 1, 0, False, 12),  # 1x1, K = 1024
    (2, 15, 13, 256, 512, 3, 2, 1, False, 12),   # strided 3x3 (implicit-GEMM conv A)
    (2, 14, 15, 256, 256, 3, 1, 1, False, 14),   # halo 3x3, 16x16x32 form
])
def test_h2_issue_spread_bit_identical(cuda, b, h, w, cin, cout, k, s, p, res, cfg):
    """conv_il: the 256x256 conv tile and the 16x16x32 halo tile with their
    next k-tiles' loads issued among the MFMAs compute the same products in
    the same order as with one burst at the top of the k-tile: identical
    bits."""
    x, wt, bias, r, _, _ = _conv_case(cuda, b, h, w, cin, cout, k, s, p, res, seed=11)
    outs = {}
    for il in (0, 1):
        with ops.tuning(0, s3_cfg=cfg, conv_il=il):
            outs[il] = _run_h2(cuda, x, wt, bias, r, s, p)[0].cpu()
    assert torch.equal(outs[0], outs[1])


def test_conv2d_h2_nonfinite_inputs(cuda):
    """An inf / NaN activation turns the outputs that read it into NaN / inf
    as fp32 does, and leaves every other output fp32-accurate (non-finite
    values stay out of the max-|x| record)."""
    x, wt, bias, r, ref, scale = _conv_case(cuda, 2, 14, 14, 64, 128, 3, 1, 1, False, seed=3)
    x[0, 5, 5, 7] = float("inf")
    x[1, 9, 2, 3] = float("nan")
    y, _ = _run_h2(cuda, x, wt, bias, None, 1, 1)
    y = y.cpu()
    touched = torch.zeros(2, 14, 14, dtype=torch.bool)
    touched[0, 4:7, 4:7] = True
    touched[1, 8:11, 1:4] = True
    assert bool((~torch.isfinite(y[touched]) | (y[touched] == 0)).any())
    ok = ~touched[..., None].expand_as(y) & (ref > 0)
    e = _rel_err(y[ok], ref[ok], scale[ok])
    assert e[0] < 4e-7


def test_resnet_h2_descriptors_vs_float64(cuda):
    """The whole R50-GeM extractor: f16x2 trunk vs exact-fp32 trunk, both
    against the oracle evaluated in float64."""
    rs = np.random.RandomState(3)
    img = torch.from_numpy(rs.randint(0, 256, size=(3, 64, 72, 3), dtype=np.uint8))
    x = embed_ref.normalize_u8(img)
    got = {}
    for math in ("h2", "f32"):
        net = GeM(2048, backbone="resnet50", seed=4, device=cuda, conv_math=math)
        got[math] = net.forward_test(x.to(cuda)).cpu().double()
    sd = {k: v.double() for k, v in W.synthetic_resnet_state_dict("resnet50", 4).items()}
    ww, wb = W.synthetic_linear(2048, 2048, 5)
    ref = embed_ref.gem_net_forward_test(x.double(), sd, W.RESNET_LAYERS["resnet50"], ww.double(), wb.double())
    e_h2 = (got["h2"] - ref).abs().max().item()
    e_f32 = (got["f32"] - ref).abs().max().item()
    print(f"R50-GeM descriptors vs float64: h2 {e_h2:.3g}  f32 {e_f32:.3g}")
    assert e_h2 < DESC_TOL and e_h2 <= 2.0 * e_f32


@pytest.mark.parametrize("b,hx,cin,planes,stride", [(3, 56, 64, 64, 1), (2, 56, 256, 128, 2), (2, 27, 512, 256, 2),
                                                    (5, 7, 1024, 512, 2)])
def test_bottleneck_out_h2_vs_float64(cuda, b, hx, cin, planes, stride):
    """A stage-entry block's conv3 + strided downsample projection as one
    f16x2 GEMM (rr_bottleneck_out_h2) vs float64 of the reference's sum
    ReLU(bn3(conv3(y)) + bn_d(conv_d(x))) (networks/backbone.py:327-346),
    next to the two-launch exact-fp32 path; odd map sizes included."""
    g = torch.Generator().manual_seed(b * hx + cin)
    oh = (hx - 1) // stride + 1
    cout = 4 * planes
    y = torch.relu(torch.randn(b, oh, oh, planes, generator=g))
    x = torch.relu(torch.randn(b, hx, hx, cin, generator=g))
    w3 = torch.randn(cout, 1, 1, planes, generator=g) / planes ** 0.5
    wd = torch.randn(cout, 1, 1, cin, generator=g) / cin ** 0.5
    b3, bd = torch.randn(cout, generator=g) * 0.1, torch.randn(cout, generator=g) * 0.1
    xs = x[:, ::stride, ::stride].double()
    ref = y.double() @ w3.reshape(cout, planes).double().t() + b3.double() + xs @ wd.reshape(cout, cin).double().t() \
        + bd.double()
    ref = torch.relu(ref)
    scale = y.double() @ w3.reshape(cout, planes).double().abs().t() + xs @ wd.reshape(cout, cin).double().abs().t()
    rec = ops.amax_records(3, cuda)
    yd, xd = y.to(cuda), x.to(cuda)
    ops.amax_f32(yd, rec[0])
    ops.amax_f32(xd, rec[1])
    wb = ops.H2Bottleneck(w3.to(cuda), b3.to(cuda), wd.to(cuda), bd.to(cuda))
    out = ops.bottleneck_out_h2(yd, rec[0], xd, rec[1], wb, stride, rec[2]).cpu()
    idn = ops.conv2d(xd, wd.to(cuda), bd.to(cuda), stride, 0, None, False)
    out_f32 = ops.conv2d(yd, w3.to(cuda), b3.to(cuda), 1, 0, idn, True).cpu()
    live = ref > 0
    e = _rel_err(out[live], ref[live], scale[live])
    ef32 = _rel_err(out_f32[live], ref[live], scale[live])
    print(f"bottleneck {b}x{hx}x{cin}/{stride} planes {planes}: h2 max {e[0]:.3g} mean {e[1]:.3g} | "
          f"f32 max {ef32[0]:.3g} mean {ef32[1]:.3g}")
    assert e[0] <= max(ef32[0], 1e-7) * 1.5 and e[1] <= ef32[1] * 1.05 + 1e-9
    assert ops.amax_value(rec[2]) == float(out.abs().max())


def test_resnet_h2_fused_downsample_matches_unfused(cuda):
    """The trunk with the stage-entry conv3 + projection fused equals the
    unfused f16x2 trunk to fp32 accuracy (only the sum's rounding order
    differs) and both stay within the trunk tolerance of each other."""
    from research_image_retrieval_amd.networks import ResNet
    rs = np.random.RandomState(9)
    x = torch.from_numpy(rs.standard_normal((2, 96, 80, 3)).astype(np.float32)).to(cuda)
    net = ResNet("resnet50", seed=3, device=cuda)
    a = net.forward(x)
    net.fuse_downsample = False
    b = net.forward(x)
    d = (a - b).abs().max().item()
    print("fused vs unfused trunk max|diff|", d, "max|y|", a.abs().max().item())
    assert d < 2e-6


@pytest.mark.parametrize("b,h,w", [(2, 224, 224), (3, 37, 53), (1, 9, 7), (2, 64, 72), (96, 64, 72)])
def test_stem_pool_h2_bit_identical(cuda, b, h, w):
    """The stem with its max-pool fused (rr_stem_pool_h2) writes the same bits
    as the f16x2 stem conv + ReLU followed by the max-pool, on map sizes whose
    pooled grid leaves ragged 8 x 7 tiles; its max-|x| record equals the conv
    output's (networks/backbone.py:103-109).  96 x 64 x 72: 576 tiles, two or
    three per persistent block (tile i's pool runs inside tile i + 1's k-loop)."""
    g = torch.Generator().manual_seed(b * h + w)
    x4 = F.pad(torch.randn(b, h, w, 3, generator=g) * 1.5, (0, 1)).contiguous().to(cuda)
    wt = F.pad(torch.randn(64, 7, 7, 3, generator=g) * (2.0 / 147) ** 0.5, (0, 1)).contiguous().to(cuda)
    bias = (torch.randn(64, generator=g) * 0.1).to(cuda)
    wc = ops.H2Conv(wt)
    rec = ops.amax_records(3, cuda)
    ops.amax_f32(x4, rec[0])
    y = ops.conv2d_h2(x4, rec[0], wc, bias, 2, 3, None, True, rec[1])
    ref = ops.maxpool2d(y, 3, 2, 1)
    # default: the persistent halo stem (resident weights, one patch fetch per
    # tile); s3_cfg 7: the implicit-GEMM config-7 stem — the same products
    # and per-accumulator order, so both match the unfused bits
    for cfg in (0, 7):
        rec[2].zero_()
        with ops.tuning(cuda.index, s3_cfg=cfg):
            got = ops.stem_pool_h2(x4, rec[0], wc, bias, 2, 3, rec[2])
        assert got.shape == ref.shape
        assert torch.equal(got.view(torch.int32), ref.view(torch.int32)), cfg
        assert ops.amax_value(rec[2]) == ops.amax_value(rec[1])


def test_resnet_h2_fused_stem_pool_bit_identical(cuda):
    """The trunk with the fused stem + max-pool equals the unfused trunk bit
    for bit (same pooled values, same max-|x| record)."""
    from research_image_retrieval_amd.networks import ResNet
    rs = np.random.RandomState(11)
    x = torch.from_numpy(rs.standard_normal((2, 70, 90, 3)).astype(np.float32)).to(cuda)
    net = ResNet("resnet50", seed=3, device=cuda)
    a = net.forward(x)
    net.fuse_stem_pool = False
    b = net.forward(x)
    assert torch.equal(a.view(torch.int32), b.view(torch.int32))


@pytest.mark.parametrize("ratio", [1e3, 1e5])
def test_conv2d_h2_heavy_tailed_channels(cuda, ratio):
    """A few input channels 1e3-1e5x larger than the rest (BN-folded real
    weights give such channel imbalance): one split scale per tensor puts the
    small channels ~2^10-2^17 below the max, still inside the 2^18 the two
    fp16 pieces keep at full precision.  The same bar against float64 and
    the exact-fp32 core as every f16x2 conv."""
    for shape in ((2, 14, 14, 256, 256, 3, 1, 1, True), (2, 14, 14, 256, 1024, 1, 1, 0, True)):
        b, h, w, cin, cout, k, s, p, res = shape
        x, wt, bias, r, _, _ = _conv_case(cuda, *shape, seed=21)
        x[..., [3, 77, 200]] *= ratio
        xn, wn = x.permute(0, 3, 1, 2).double(), wt.permute(0, 3, 1, 2).double()
        conv = F.conv2d(xn, wn, None, s, p).permute(0, 2, 3, 1)
        scale = F.conv2d(xn.abs(), wn.abs(), None, s, p).permute(0, 2, 3, 1)
        ref = torch.relu(conv + bias.double() + r.double())
        y, rec = _run_h2(cuda, x, wt, bias, r, s, p)
        y_f32 = ops.conv2d(x.to(cuda), wt.to(cuda), bias.to(cuda), s, p, r.to(cuda), True).cpu()
        live = ref > 0
        e = _rel_err(y.cpu()[live], ref[live], scale[live])
        ef32 = _rel_err(y_f32[live], ref[live], scale[live])
        print(f"heavy-tailed x{ratio:g} {shape}: h2 max {e[0]:.3g} mean {e[1]:.3g} | "
              f"f32 max {ef32[0]:.3g} mean {ef32[1]:.3g}")
        assert e[0] <= 1.25 * max(ef32[0], 1e-7) and e[1] <= ef32[1] * 1.05 + 1e-9
        assert ops.amax_value(rec[1]) == float(y.abs().max())


def test_resnet_h2_heavy_tailed_activations_vs_float64(cuda):
    """The R50-GeM extractor with heavy-tailed intermediate activations: a
    few channels of layer1.0's and layer3.2's first ReLU outputs scaled by
    1e4 (their BN affine x1e4, the next conv's input columns x1e-4: the same
    function, every such channel 1e4x the rest).  f16x2 vs float64 within 2x
    the exact-fp32 trunk's error, and <= 1e-6 (the descriptor bar)."""
    rs = np.random.RandomState(5)
    img = torch.from_numpy(rs.randint(0, 256, size=(2, 64, 72, 3), dtype=np.uint8))
    x = embed_ref.normalize_u8(img)
    sd = W.synthetic_resnet_state_dict("resnet50", 6)
    for blk, chans in (("layer1.0", [1, 9, 30]), ("layer3.2", [5, 100, 200])):
        for key in ("weight", "bias"):
            sd[f"{blk}.bn1.{key}"][chans] *= 1e4
        sd[f"{blk}.conv2.weight"][:, chans] *= 1e-4
    got = {}
    for math in ("h2", "f32"):
        net = GeM(2048, backbone="resnet50", state_dict=sd, seed=6, device=cuda, conv_math=math)
        got[math] = net.forward_test(x.to(cuda)).cpu().double()
    ww, wb = W.synthetic_linear(2048, 2048, 7)
    ref = embed_ref.gem_net_forward_test(x.double(), {k: v.double() for k, v in sd.items()},
                                         W.RESNET_LAYERS["resnet50"], ww.double(), wb.double())
    e_h2 = (got["h2"] - ref).abs().max().item()
    e_f32 = (got["f32"] - ref).abs().max().item()
    print(f"heavy-tailed R50-GeM descriptors vs float64: h2 {e_h2:.3g}  f32 {e_f32:.3g}")
    assert e_h2 < DESC_TOL and e_h2 <= 2.0 * e_f32


@pytest.mark.parametrize("ratio_log2", [10, 20])
def test_h2_batch_coupling_bounded(cuda, ratio_log2):
    """One split scale per activation tensor couples the images of a batch:
    an image next to one whose activations are 2^r larger has its values
    split 2^r below the tensor max.  Its descriptor embedded alone and inside
    such a batch (networks.GeM R50, the f16x2 trunk) differ by <= 1e-6, and
    both stay <= 1e-6 from float64."""
    rs = np.random.RandomState(8)
    img = torch.from_numpy(rs.randint(0, 256, size=(2, 64, 72, 3), dtype=np.uint8))
    x = embed_ref.normalize_u8(img)
    big = x[1:2] * 2.0 ** ratio_log2
    net = GeM(2048, backbone="resnet50", seed=9, device=cuda)
    alone = net.forward_test(x[:1].to(cuda)).cpu().double()
    batch = net.forward_test(torch.cat([x[:1], big]).to(cuda)).cpu().double()
    sd = {k: v.double() for k, v in W.synthetic_resnet_state_dict("resnet50", 9).items()}
    ww, wb = W.synthetic_linear(2048, 2048, 10)
    ref = embed_ref.gem_net_forward_test(x[:1].double(), sd, W.RESNET_LAYERS["resnet50"], ww.double(), wb.double())
    d = (alone[0] - batch[0]).abs().max().item()
    ea, eb = (alone - ref).abs().max().item(), (batch[:1] - ref).abs().max().item()
    print(f"batch coupling 2^{ratio_log2}: alone vs in batch {d:.3g}; vs float64 alone {ea:.3g} in batch {eb:.3g}")
    assert d <= DESC_TOL and ea <= DESC_TOL and eb <= DESC_TOL


@pytest.mark.parametrize("b,h,w,cin,res", [
    (24, 56, 56, 64, False),   # the R101 64@56 shape, 294 tiles (several per block)
    (40, 31, 63, 32, True),    # the widest map, one slice per tile: every next slice is the next tile's
    (30, 28, 28, 128, False),  # four slices per tile
    (1, 56, 56, 64, False),    # fewer tiles than blocks
])
def test_h2_halo_persistent_bit_identical(cuda, b, h, w, cin, res):
    """The N = 64 halo tile as a persistent stream (the default: the next
    tile's first halo slice and B stage load under the current tile's last
    slice; C staged through the released halo buffer) computes the same
    products in the same order as the one-tile kernel (s3_cfg 13): identical
    bits and max-|y| record."""
    x, wt, bias, r, _, _ = _conv_case(cuda, b, h, w, cin, 64, 3, 1, 1, res, seed=29)
    outs, amax = {}, {}
    # 13: the one-tile form; halo_mf 3: the persistent stream (round 5's
    # default; the default is now the 512-row tile where it fits)
    for cfg, mf in ((13, -1), (0, 3), (0, -1)):
        with ops.tuning(0, s3_cfg=cfg, halo_mf=mf):
            y, rec = _run_h2(cuda, x, wt, bias, r, 1, 1)
        outs[(cfg, mf)], amax[(cfg, mf)] = y.cpu(), ops.amax_value(rec[1])
    ref = outs[(13, -1)]
    for k in outs:
        assert torch.equal(outs[k], ref), k
        assert amax[k] == float(ref.abs().max()), k


@pytest.mark.parametrize("b,h,w,cin,res", [
    (24, 56, 56, 64, False),   # the R101 64@56 shape, 147 tiles of 512 rows
    (7, 33, 63, 32, True),     # the widest map the 640-row halo holds, one slice per tile
    (5, 20, 28, 128, False),   # four slices per tile
    (1, 56, 56, 64, False),    # a ragged last tile
])
def test_h2_halo_512_bit_identical(cuda, b, h, w, cin, res):
    """The 512-row single-buffer N = 64 halo tile (the default where its halo
    holds the map; halo_mf 2 forces it: 8 waves of 64 x 64, one halo buffer
    refilled behind a barrier per slice) computes the same products in the
    same order as round 5's persistent 256-row stream (halo_mf 3): identical
    bits and max-|y| record."""
    x, wt, bias, r, _, _ = _conv_case(cuda, b, h, w, cin, 64, 3, 1, 1, res, seed=31)
    outs, amax = {}, {}
    for mf in (3, 2):
        with ops.tuning(0, halo_mf=mf):
            y, rec = _run_h2(cuda, x, wt, bias, r, 1, 1)
        outs[mf], amax[mf] = y.cpu(), ops.amax_value(rec[1])
    assert torch.equal(outs[3], outs[2])
    assert amax[3] == amax[2] == float(outs[2].abs().max())


@pytest.mark.parametrize("b,h,w,cin,res", [(6, 28, 28, 128, False), (3, 17, 31, 64, True)])
def test_h2_halo_n128_single_buffer_bit_identical(cuda, b, h, w, cin, res):
    """N = 128: the single-buffer halo tile with three taps per barrier (the
    default) against the two-buffer one-tap tile (halo_mf 4): same products in
    the same order, identical bits."""
    x, wt, bias, r, _, _ = _conv_case(cuda, b, h, w, cin, 128, 3, 1, 1, res, seed=37)
    outs = {}
    for mf in (-1, 4):
        with ops.tuning(0, halo_mf=mf):
            y, _ = _run_h2(cuda, x, wt, bias, r, 1, 1)
        outs[mf] = y.cpu()
    assert torch.equal(outs[-1], outs[4])



@pytest.mark.parametrize("b,h,w,cin,cout", [
    (2, 14, 14, 64, 256),    # one 16 x 16 block per image, two Cin slices
    (3, 15, 13, 32, 256),    # ragged blocks, one slice
    (2, 28, 28, 128, 128),   # 2 x 2 blocks per image
    (1, 27, 31, 64, 128),    # the widest map the 320-row raster halo holds
    (2, 56, 56, 64, 64),     # 16 x 32 blocks (the 512-row N = 64 tile), 4 x 2 per image
    (3, 17, 40, 32, 64),     # ragged 16 x 32 blocks
])
def test_h2_halo_2d_bit_identical(cuda, b, h, w, cin, cout):
    """The 2-D block halo tiles (halo_2d 1 forces them where the raster halo
    also serves) compute every output from the same products in the same
    order as the raster halo tiles (halo_2d 0): identical bits and max-|y|
    record, the ragged blocks' off-map rows neither stored nor counted."""
    x, wt, bias, r, _, _ = _conv_case(cuda, b, h, w, cin, cout, 3, 1, 1, False, seed=41)
    outs, amax = {}, {}
    for t2 in (0, 1):
        with ops.tuning(0, halo_2d=t2):
            y, rec = _run_h2(cuda, x, wt, bias, r, 1, 1)
        outs[t2], amax[t2] = y.cpu(), ops.amax_value(rec[1])
    assert torch.equal(outs[0], outs[1])
    assert amax[0] == amax[1] == float(outs[1].abs().max())


@pytest.mark.parametrize("b,h,w,cin,cout,res", [
    (1, 20, 40, 64, 256, False),    # N % 256, W = 40: the raster tile would need 338 halo rows (288)
    (2, 33, 50, 128, 128, False),   # N = 128, W = 50 (358 > 320)
    (1, 18, 70, 64, 64, False),     # N = 64, W = 70 (654 > 640)
    (1, 9, 130, 32, 64, False),     # N = 64, one ragged block row, five block columns
    (1, 20, 40, 64, 256, True),     # a residual epilogue: not a 2-D tile's, falls back
])
def test_conv2d_h2_halo_2d_wide(cuda, b, h, w, cin, cout, res):
    """Maps too wide for a raster halo: the 2-D block tiles (forced) at the
    f16x2 bar against float64 and the exact-fp32 core, with the max-|y| record
    exact; the default is bit-identical to them, except for N = 128 on fewer
    blocks than CUs (and residual epilogues), where it keeps the implicit GEMM."""
    x, wt, bias, r, ref, scale = _conv_case(cuda, b, h, w, cin, cout, 3, 1, 1, res, seed=43)
    with ops.tuning(0, halo_2d=1):
        y, rec = _run_h2(cuda, x, wt, bias, r, 1, 1)
    y = y.cpu()
    y_def, _ = _run_h2(cuda, x, wt, bias, r, 1, 1)
    with ops.tuning(0, halo_2d=0):
        y_off, _ = _run_h2(cuda, x, wt, bias, r, 1, 1)
    small128 = cout == 128 and b * ((h + 15) // 16) * ((w + 15) // 16) < 256
    assert torch.equal(y_def.cpu(), (y_off if small128 or res else y).cpu())
    rd = r.to(cuda) if res else None
    y_f32 = ops.conv2d(x.to(cuda), wt.to(cuda), bias.to(cuda), 1, 1, rd, True).cpu()
    live = ref > 0
    e = _rel_err(y[live], ref[live], scale[live])
    ef32 = _rel_err(y_f32[live], ref[live], scale[live])
    print(f"halo 2d {b}x{h}x{w}x{cin}->{cout}: max {e[0]:.3g} mean {e[1]:.3g} | f32 max {ef32[0]:.3g} "
          f"mean {ef32[1]:.3g}")
    assert e[0] <= 1.25 * max(ef32[0], 1e-7) and e[1] <= ef32[1] * 1.05 + 1e-9
    assert ops.amax_value(rec[1]) == float(y.abs().max())
    assert bool(torch.isfinite(y).all())


def test_conv2d_h2_dense_past_4gb_row_chunks(cuda):
    """A dense 1x1 conv whose input passes 4 GB (config 15's 32-bit byte
    offsets; C2's layer-1 batches) runs as row chunks of config-15 launches:
    every output row equals, bit for bit, the same rows from a launch on its
    image alone with the same input split scale, across the chunk boundary
    (image 7 straddles it), and the max-|y| record is the whole output's."""
    b, h, w, cin = 8, 725, 725, 256   # 4.3 GB of fp32 input
    g = torch.Generator(device=cuda).manual_seed(5)
    x = torch.relu(torch.randn(b, h, w, cin, device=cuda, generator=g))
    rin = ops.amax_records(1, cuda)[0]
    ops.amax_f32(x, rin)
    for cout in (64, 256):
        wc = ops.H2Conv(torch.randn(cout, 1, 1, cin, device=cuda, generator=g) * (2.0 / cin) ** 0.5)
        bias = torch.randn(cout, device=cuda, generator=g) * 0.1
        rout = ops.amax_records(1, cuda)[0]
        y = ops.conv2d_h2(x, rin, wc, bias, 1, 0, None, True, rout)
        for i in (0, 7):
            ri = ops.amax_records(1, cuda)[0]
            yi = ops.conv2d_h2(x[i:i + 1], rin, wc, bias, 1, 0, None, True, ri)
            assert torch.equal(y[i:i + 1], yi), (cout, i)
        assert ops.amax_value(rout) == float(y.abs().max())
        del y
    torch.cuda.empty_cache()
