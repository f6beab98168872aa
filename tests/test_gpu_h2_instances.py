"""Every compiled f16x2 conv kernel (rr_conv2d_h2: csrc/h2_tile.hip,
h2_stream.hip, h2_stream256.hip, h2_halo.hip) against float64, one witness
each from tests/h2_witness.py (tests/test_h2_coverage.py proves on the CPU
that the witnesses reach the kernels they name and cover all of them), then
the k-loops' depth edges, the implicit-GEMM loader's geometry edges and the
optional operands.

Unlike tests/test_gpu_h2.py, whose bars these are, every output is compared,
not only those the reference's ReLU leaves positive: error |y - ref| /
sum |x||w| over all outputs, a ReLU output is >= 0 and exactly 0 where the
float64 pre-activation is clearly negative, and the output's storage is
filled with NaN before the call so that a row the kernel leaves unwritten
shows.

Bars, tests/test_gpu_h2.py's: a route the library picks (no knob set) must
match the exact-fp32 MFMA core (ops.conv2d) on the same inputs, max <= 1.25
max(f32 max, 1e-7) and mean <= 1.05 f32 mean + 1e-9; a forced route must keep
max < 4e-7.  Measured on all outputs, both bars of a pick hold as they are on
two accumulator sets at K > 64; where they did not, they moved with the exact
core's error on the same inputs as the yardstick (MI355X, pairs h2 | f32):

* Max on the one-accumulator kernels (the route's acc == 1: tiles 10, 11, 12,
  stream 15's 256x256 and 256x128 forms, the halo tiles): sqrt(3) x max(f32
  max, 1e-7).  They round a0b1 + a1b0 against the running sum, three roundings
  per k-step where two accumulator sets have one: up to three times the
  variance.  Measured: tile 11 on the NHWC4 stem (K = 224) 3.00e-7 | 1.85e-7,
  1.62x; stream 15, 256x256 at K = 288 3.30e-7 | 2.52e-7, 1.31x; the others
  within 1.25x.
* Mean, where an output sums 64 products or fewer (K <= 64, or the border
  outputs of a padded conv with few live taps): 1.05 x the mean over the
  outputs of sqrt(1 + c / n_i), n_i output i's live products, c = 16 on two
  accumulator sets and 24 on one.  The split keeps 22 of each fp32 operand's
  24 significand bits and drops a1 b1 (<= 2^-22 |a b|), an error per product
  where the exact core's products are exact; it adds as a random walk, so its
  variance against the exact core's rounding of the sum falls as 1 / n.
  Measured, with the factor this allows: K = 32 on two sets (stream 8)
  3.00e-8 | 2.45e-8, 1.22x of 1.29; on one (tile 11) 2.63e-8 | 2.08e-8, 1.26x
  of 1.39; K = 64 on two (stream 8) 2.12e-8 | 2.07e-8, 1.02x of 1.17; on one
  (tile 11, the pick for N = 128) 2.31e-8 | 2.02e-8, 1.15x of 1.23; 3x3 pad 2
  on a 6x5 map (tile 12, corner outputs of one live tap) 2.31e-8 | 2.01e-8,
  1.15x of 1.16.
"""
import functools

import pytest
import torch
import torch.nn.functional as F

import h2_witness as HW
import test_h2_route as TR
from research_image_retrieval_amd import ops

pytestmark = pytest.mark.gpu

NAMES = {route: name for name, route in TR.ROUTES.items()}


_geo = HW.geo


def _key(geo):
    return tuple(geo[k] for k in ("b", "h", "w", "cin", "cout", "kh", "kw", "stride", "pad"))


@functools.lru_cache(maxsize=4)
def _case(key, residual, seed=0):
    """Inputs by test_gpu_h2._conv_case's recipe (ReLU'd activations, He
    weights, a bias and a residual of the activations' size) and the float64
    pre-activation conv + bias (+ residual) with its scale sum |x||w|.  Shared
    between the tests of one geometry: nothing here is written to."""
    b, h, w, cin, cout, kh, kw, s, p = key
    g = torch.Generator().manual_seed(b * h + cin + cout + seed)
    x = torch.relu(torch.randn(b, h, w, cin, generator=g))
    wt = torch.randn(cout, kh, kw, cin, generator=g) * (2.0 / (kh * kw * cin)) ** 0.5
    bias = torch.randn(cout, generator=g) * 0.1
    oh, ow = (h + 2 * p - kh) // s + 1, (w + 2 * p - kw) // s + 1
    r = torch.randn(b, oh, ow, cout, generator=g) if residual else None
    if (kh, kw, s, p) == (1, 1, 1, 0):  # the same sums as a GEMM (large M: F.conv2d in float64 is slow)
        x2, w2 = x.double().reshape(-1, cin), wt.double().reshape(cout, cin)
        conv, scale = (x2 @ w2.t()).reshape(b, oh, ow, cout), (x2.abs() @ w2.abs().t()).reshape(b, oh, ow, cout)
    else:
        xn, wn = x.permute(0, 3, 1, 2).double(), wt.permute(0, 3, 1, 2).double()
        conv = F.conv2d(xn, wn, None, s, p).permute(0, 2, 3, 1)
        scale = F.conv2d(xn.abs(), wn.abs(), None, s, p).permute(0, 2, 3, 1)
    pre = conv + bias.double() + (r.double() if residual else 0.0)
    return x, wt, bias, r, pre, scale


class _Dev:
    """One case's operands on the device, uploaded once for its runs."""

    def __init__(self, cuda, case, geo):
        x, wt, bias, r, _, _ = case
        self.cuda, self.s, self.p = cuda, geo["stride"], geo["pad"]
        self.x, self.w, self.bias = x.to(cuda), wt.to(cuda), bias.to(cuda)
        self.r = None if r is None else r.to(cuda)
        self.wc = ops.H2Conv(self.w)
        self.x_amax = ops.amax_of(self.x)
        b, h, w, _ = x.shape
        cout, kh, kw, _ = wt.shape
        self.oshape = (b, (h + 2 * self.p - kh) // self.s + 1, (w + 2 * self.p - kw) // self.s + 1, cout)

    def h2(self, relu, knobs, bias=True, y_rec=True):
        rec = ops.amax_records(1, self.cuda)[0] if y_rec else None
        # NaN in the block the allocator hands conv2d_h2 next for its output:
        # freeing the block restores the allocator's state, so the next request
        # of the same size gets it again, and an unwritten row then reads NaN
        poison = torch.full(self.oshape, float("nan"), dtype=torch.float32, device=self.cuda)
        poisoned = poison.data_ptr()
        del poison
        with ops.tuning(0, **knobs):
            y = ops.conv2d_h2(self.x, self.x_amax, self.wc, self.bias if bias else None, self.s, self.p, self.r, relu, rec)
        assert y.data_ptr() == poisoned, "the output did not land in the NaN-filled block: the stale-row check is void"
        return y.cpu(), (ops.amax_value(rec) if y_rec else None)

    def f32(self, relu):
        return ops.conv2d(self.x, self.w, self.bias, self.s, self.p, self.r, relu).cpu()


def _err(y, ref, scale):
    e = (y.double() - ref).abs() / scale.clamp_min(1e-300)
    return e.max().item(), e.mean().item()


def _live_products(geo):
    """The products each output pixel sums, [OH, OW]: Cin x the filter taps inside the map."""
    def taps(size, k):
        out = (size + 2 * geo["pad"] - k) // geo["stride"] + 1
        return torch.tensor([sum(0 <= o * geo["stride"] - geo["pad"] + t < size for t in range(k)) for o in range(out)])
    return geo["cin"] * taps(geo["h"], geo["kh"])[:, None] * taps(geo["w"], geo["kw"])[None, :]


def _pick_bars(geo, acc):
    """The factors of the exact-fp32 core's max and mean a picked route must keep (the module docstring)."""
    n = _live_products(geo).double().flatten()
    n = n[n > 0]  # (an output that reads only padding is bias + residual, exact)
    mean_bar = 1.05 if n.min() > 64 else 1.05 * (1.0 + (16.0 if acc == 2 else 24.0) / n).sqrt().mean().item()
    return (1.25 if acc == 2 else 3.0 ** 0.5), mean_bar


def _check(what, y, amax, y_f32, case, geo, relu, knobs):
    _, _, _, r, pre, scale = case
    ref = torch.relu(pre) if relu else pre
    assert y.shape == ref.shape, what
    assert bool(torch.isfinite(y).all()), f"{what}: a row left unwritten (NaN-filled storage) or a non-finite output"
    if relu:
        assert bool((y >= 0).all()), f"{what}: negative output under ReLU"
        assert bool((y[pre < -4e-7 * scale] == 0).all()), f"{what}: ReLU must zero a clearly negative pre-activation"
    e, ef = _err(y, ref, scale), _err(y_f32, ref, scale)
    print(f"{what} relu {int(relu)}: h2 max {e[0]:.3g} mean {e[1]:.3g} | f32 max {ef[0]:.3g} mean {ef[1]:.3g}")
    if not knobs:  # the library's pick
        acc = ops.h2_route(**geo, residual=r is not None, relu=relu).acc
        max_bar, mean_bar = _pick_bars(geo, acc)
        assert e[0] <= max_bar * max(ef[0], 1e-7) and e[1] <= ef[1] * mean_bar + 1e-9, (what, relu, acc, max_bar, mean_bar, e, ef)
    else:
        assert e[0] < 4e-7, (what, relu, e, ef)
    if amax is not None:
        assert amax == float(y.abs().max()), what


def _route_name(geo, residual, relu, knobs):
    r = ops.h2_route(**geo, residual=residual, relu=relu, **knobs)
    return NAMES.get(r._replace(chunk_rows=0), str(r))


# ---- every instantiation ------------------------------------------------------
@pytest.mark.parametrize("w", HW.WITNESSES, ids=HW.witness_id)
def test_instance_vs_float64(cuda, w):
    case = _case(_key(w.geometry), w.residual)
    dev = _Dev(cuda, case, w.geometry)
    y, amax = dev.h2(w.relu, w.knobs)
    _check(HW.witness_id(w), y, amax, dev.f32(w.relu), case, w.geometry, w.relu, w.knobs)


# ---- k-loop depth ---------------------------------------------------------------
def _depth_cases():
    T = HW
    cases = []
    for cin in (32, 96, 160, 192, 224):   # 1, 3, 5, 6, 7 k-tiles (BK 16: twice as many)
        for name, knobs in ((T.T4, dict(s3_cfg=4)), (T.T9, dict(s3_cfg=9)), (T.T10, dict(s3_cfg=10)),
                            (T.T12, dict(s3_cfg=12)), (T.T12IL, dict(s3_cfg=12, conv_il=1))):
            cases.append((name, cin, 256, False, knobs))
        cases.append((T.S8, cin, 256, True, {}))
        cases.append((T.T3, cin, 128, False, dict(s3_cfg=3)))
        cases.append((T.T11, cin, 128, False, {}))
        cases.append((T.T7, cin, 64, False, dict(s3_cfg=7)))
        if cin >= 64:
            cases.append((T.S15N64, cin, 64, True, {}))
    for cin in (256, 288):                # 8 and 9 k-tiles: an even and an odd stream length
        cases.append((T.S15, cin, 256, True, {}))
        cases.append((T.S15N128, cin, 128, True, {}))
    return cases


@pytest.mark.parametrize("name,cin,cout,residual,knobs", _depth_cases(), ids=[f"{c[0]} | K {c[1]}" for c in _depth_cases()])
def test_k_depth(cuda, name, cin, cout, residual, knobs):
    """One k-tile (the clamped look-ahead loads, nk > 1 ? 1 : 0), odd and even
    counts, every tail length of config 9's unroll by six: dense 1x1 on 330
    rows (a ragged second tile), both ReLU settings."""
    geo = HW.dense(cin, cout)
    case = _case(_key(geo), residual, seed=4)
    dev = _Dev(cuda, case, geo)
    for relu in (False, True):
        assert _route_name(geo, residual, relu, knobs) == name
        y, amax = dev.h2(relu, knobs)
        _check(f"{name} K {cin}", y, amax, dev.f32(relu), case, geo, relu, knobs)


# more tiles than a 256-CU device has blocks, at the shortest K the stream
# takes: a tile boundary on every k-tile (or every second)
STREAM_CASES = [  # route, geometry, residual, knobs, the one-tile twin's route and knobs
    (HW.S8, _geo(40, 40, 25, 32, 256, 1, 1, 1, 0), True, {}, HW.T4, dict(s3_cfg=4)),          # M = 40000: 313 tiles
    (HW.S15, _geo(70, 40, 25, 256, 256, 1, 1, 1, 0), True, {}, HW.T12, dict(s3_cfg=12)),      # M = 70000: 274 tiles
    (HW.S15N64, _geo(70, 40, 25, 64, 64, 1, 1, 1, 0), True, {}, HW.T7, dict(s3_cfg=7)),       # 274 tiles, two k-tiles
    (HW.H384P, _geo(40, 31, 63, 32, 64, 3, 3, 1, 1), True, dict(halo_mf=3), HW.H384, dict(s3_cfg=13)),  # 306 tiles, one slice
]


@pytest.mark.parametrize("name,geo,residual,knobs,twin,twin_knobs", STREAM_CASES, ids=[c[0] for c in STREAM_CASES])
def test_stream_past_one_tile_per_block(cuda, name, geo, residual, knobs, twin, twin_knobs):
    """The persistent k-streams with several tiles per block: float64 on all
    outputs, and the bits and max-|y| record of the one-tile kernel that keeps
    the same per-accumulator order."""
    case = _case(_key(geo), residual, seed=7)
    dev = _Dev(cuda, case, geo)
    for relu in (False, True):
        assert _route_name(geo, residual, relu, knobs) == name and _route_name(geo, residual, relu, twin_knobs) == twin
        y, amax = dev.h2(relu, knobs)
        _check(name, y, amax, dev.f32(relu), case, geo, relu, knobs)
        y1, amax1 = dev.h2(relu, twin_knobs)
        assert torch.equal(y.view(torch.int32), y1.view(torch.int32)) and amax == amax1, (name, relu)


# ---- conv-A geometry ------------------------------------------------------------
GEOMETRIES = [
    ("3x3 pad 0", _geo(2, 9, 8, 64, 256, 3, 3, 1, 0)),            # output smaller than the input
    ("3x3 pad 2", _geo(2, 6, 5, 32, 256, 3, 3, 1, 2)),            # output larger: rr_conv2d_h2 takes any pad >= 0
    ("1x3 pad 1", _geo(2, 7, 9, 64, 256, 1, 3, 1, 1)),            # padded rows read no input at all
    ("3x1 pad 0", _geo(2, 7, 9, 32, 256, 3, 1, 1, 0)),
    ("5x5 pad 2", _geo(2, 9, 7, 32, 256, 5, 5, 1, 2)),
    ("3x3 stride 2, 8x7", _geo(2, 8, 7, 64, 256, 3, 3, 2, 1)),
    ("3x3 stride 2, 1 pixel high", _geo(3, 1, 9, 64, 256, 3, 3, 2, 1)),
    ("1x1 stride 2, 9x7", _geo(2, 9, 7, 64, 256, 1, 1, 2, 0)),
    ("3x3 pad 1 on 2x2", _geo(3, 2, 2, 64, 256, 3, 3, 1, 1)),     # a map smaller than the filter's reach
    ("3x3 pad 1, 25 rows", _geo(1, 5, 5, 32, 256, 3, 3, 1, 1)),   # b = 1, M < 32
]
HALO_GEOMETRIES = ("3x3 pad 1 on 2x2", "3x3 pad 1, 25 rows")     # 3x3 / stride 1 / pad 1: the pick is a halo tile


@pytest.mark.parametrize("knobs", [{}, dict(s3_cfg=7), dict(s3_cfg=12)], ids=["pick", "forced 7", "forced 12"])
@pytest.mark.parametrize("what,geo", GEOMETRIES, ids=[g[0] for g in GEOMETRIES])
def test_conv_geometry_edges(cuda, what, geo, knobs):
    """The implicit-GEMM A loader's tap walk and bounds on filters and maps the
    trunk never has: the pick, config 7 (BK 16: two k-tiles per 32 channels)
    and config 12.  Only a 3x3 / stride 1 / pad 1 conv may go to a halo tile."""
    residual = False  # (error is taken relative to sum |x||w|, which a row of few live taps keeps small)
    case = _case(_key(geo), residual, seed=9)
    dev = _Dev(cuda, case, geo)
    for relu in (False, True):
        name = _route_name(geo, residual, relu, knobs)
        if knobs:
            assert name == (HW.T7 if knobs["s3_cfg"] == 7 else HW.T12)
        else:
            assert ("halo" in name) == (what in HALO_GEOMETRIES), name
        y, amax = dev.h2(relu, knobs)
        _check(f"{what} on {name}", y, amax, dev.f32(relu), case, geo, relu, knobs)


# ---- optional operands ------------------------------------------------------------
def _one_per_family():
    seen = {}
    for w in HW.WITNESSES:
        if w.relu:
            seen[TR.ROUTES[w.route].family] = w  # the last of each family: with a residual where it has one
    return [seen[f] for f in sorted(seen)]


@pytest.mark.parametrize("w", _one_per_family(), ids=HW.witness_id)
def test_optional_operands(cuda, w):
    """bias = NULL is a zero bias and y_amax = NULL changes no output, bit for bit."""
    x, wt, bias, r, pre, scale = _case(_key(w.geometry), w.residual)
    dev = _Dev(cuda, (x, wt, torch.zeros_like(bias), r, pre, scale), w.geometry)
    y0, amax0 = dev.h2(w.relu, w.knobs)
    y1, amax1 = dev.h2(w.relu, w.knobs, bias=False)
    y2, _ = dev.h2(w.relu, w.knobs, y_rec=False)
    assert bool(torch.isfinite(y0).all())
    assert torch.equal(y0.view(torch.int32), y1.view(torch.int32)) and amax0 == amax1
    assert torch.equal(y0.view(torch.int32), y2.view(torch.int32))
