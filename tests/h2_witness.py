"""One witness per compiled f16x2 conv kernel: a small conv and the tuning
knobs under which rr_conv2d_h2 launches exactly that instantiation.

h2_route.hpp names the kernel instances (test_h2_route.ROUTES holds them); the
launchers compile each for its A modes (dense: 1x1 / stride 1 / pad 0; conv:
the implicit GEMM; c4: the NHWC4 stem) and for the residual / ReLU epilogues of
h2_ep_dispatch.  tests/test_h2_coverage.py proves on the CPU, through
ops.h2_route, that every entry here reaches the instance it names and that the
entries cover the compiled space exactly; tests/test_gpu_h2_instances.py runs
each against float64.  No tests in this file.

Shapes: b, h, w = 3, 11, 10 is M = 330, two 256-row tiles with the second
ragged (three 128-row tiles, one ragged 512-row tile); the strided convs
have M = 396 and the stem M = 240; Cin 64 is two k-tiles.
Every witness stays under 1000 output rows.
"""
import collections

# geometry: ops.h2_route's shape arguments (without residual / relu); knobs: ops.tuning's
Witness = collections.namedtuple("Witness", "route amode residual relu geometry knobs")

AMODES = ("dense", "conv", "c4")


def amode_of(geometry):
    """The A mode rr_conv2d_h2 takes for a geometry (conv2d_h2_geometry, rr_api.hip)."""
    g = geometry
    if g["cin"] == 4:
        return "c4"
    return "dense" if (g["kh"], g["kw"], g["stride"], g["pad"]) == (1, 1, 1, 0) else "conv"


def geo(b, h, w, cin, cout, kh, kw, stride, pad):
    """ops.h2_route's shape arguments of one conv."""
    return dict(b=b, h=h, w=w, cin=cin, cout=cout, kh=kh, kw=kw, stride=stride, pad=pad)


def _geo(b, h, w, cin, cout, k, stride, pad):  # a square filter
    return geo(b, h, w, cin, cout, k, k, stride, pad)


def dense(cin, cout):          # 1x1, M = 330
    return _geo(3, 11, 10, cin, cout, 1, 1, 0)


def conv3(cout):               # 3x3 stride 1 pad 1, W = 10: every raster halo holds it; M = 330, K = 576
    return _geo(3, 11, 10, 64, cout, 3, 1, 1)


def wide40(cout):              # W = 40: past the 288- and 320-row raster halos; M = 720, K = 288
    return _geo(1, 18, 40, 32, cout, 3, 1, 1)


WIDE70 = _geo(1, 9, 70, 32, 64, 3, 1, 1)   # W = 70: past the 384- and 640-row raster halos; M = 630


def conv3s2(cout):             # 3x3 stride 2 (implicit-GEMM conv A) on an odd map, M = 3 x 12 x 11 = 396
    return _geo(3, 23, 21, 64, cout, 3, 2, 1)


def proj_s2(cout):             # 1x1 stride 2 (conv A) on an odd map, M = 396
    return _geo(3, 23, 21, 64, cout, 1, 2, 0)


def stem(cout):                # NHWC4 7x7 stride 2 pad 3, K = 196 padded to 224, M = 240
    return _geo(2, 23, 19, 4, cout, 7, 2, 3)


T3, T4, T7 = "tile 3, 256x128", "tile 4, 128x256, 16x16x32", "tile 7, 256x64, BK 16"
T9, T10 = "tile 9, 128x256, 16x16x32, 3 stages", "tile 10, 128x256, 16x16x32, 1 acc"
T11, T12, T12IL = "tile 11, 128x128, 16x16x32, 1 acc", "tile 12, 256x256, 1 acc", "tile 12, 256x256, 1 acc, IL"
S8, S15, S15N128, S15N64 = ("stream 8, 128x256, 16x16x32", "stream 15, 256x256", "stream 15, 256x128",
                            "stream 15, 256x64, 2 acc")
H288, H288MF, H288IL = ("halo 288 rows, 256x256, 32x32x16, 1 tap", "halo 288 rows, 256x256, 16x16x32, 1 tap",
                        "halo 288 rows, 256x256, 16x16x32, 1 tap, IL")
H320, H320MF, H320SB = ("halo 320 rows, 256x128, 32x32x16, 1 tap", "halo 320 rows, 256x128, 16x16x32, 1 tap",
                        "halo 320 rows, 256x128, 16x16x32, 3 taps, one buffer")
H384, H384MF, H384P = ("halo 384 rows, 256x64, 32x32x16, 3 taps", "halo 384 rows, 256x64, 16x16x32, 3 taps",
                       "halo 384 rows, 256x64, 32x32x16, 3 taps, persistent")
H640 = "halo 640 rows, 512x64, 32x32x16, 3 taps"
B256, B128, B512 = ("2-D halo 16x16, 256x256, 16x16x32, 1 tap", "2-D halo 16x16, 256x128, 16x16x32, 3 taps, one buffer",
                    "2-D halo 16x32, 512x64, 32x32x16, 3 taps")

BOTH, NO_RES, RES = (False, True), (False,), (True,)

# route, the residual epilogues this line witnesses, geometry, knobs ({}: the library's pick).
# One line (or two, where a residual moves the pick) per (route, A mode).
TABLE = [
    # ---- one tile per block: dense, conv and NHWC4 A
    (T3, BOTH, dense(64, 96), {}),
    (T3, NO_RES, conv3s2(64), {}),
    (T3, RES, WIDE70, {}),                       # a residual keeps the 2-D tile away
    (T3, BOTH, stem(64), {}),
    (T4, BOTH, dense(64, 256), dict(s3_cfg=4)),
    (T4, BOTH, proj_s2(256), {}),
    (T4, BOTH, stem(256), {}),
    (T7, BOTH, dense(64, 64), dict(s3_cfg=7)),
    (T7, BOTH, conv3(64), dict(s3_cfg=7)),
    (T7, BOTH, stem(64), dict(s3_cfg=7)),
    (T9, BOTH, dense(64, 256), dict(s3_cfg=9)),
    (T9, BOTH, conv3(256), dict(s3_cfg=9)),
    (T9, BOTH, stem(256), dict(s3_cfg=9)),
    (T10, BOTH, dense(64, 256), dict(s3_cfg=10)),
    (T10, BOTH, conv3(256), dict(s3_cfg=10)),
    (T10, BOTH, stem(256), dict(s3_cfg=10)),
    (T11, BOTH, dense(64, 128), {}),
    (T11, BOTH, wide40(128), {}),                # 6 blocks: too few for the 2-D tile's pick
    (T11, BOTH, stem(128), {}),
    (T12, BOTH, dense(64, 256), dict(s3_cfg=12)),
    (T12, NO_RES, conv3s2(256), {}),
    (T12, RES, wide40(256), {}),
    (T12, BOTH, stem(256), dict(s3_cfg=12)),
    (T12IL, BOTH, dense(64, 256), dict(s3_cfg=12, conv_il=1)),
    (T12IL, NO_RES, conv3s2(256), dict(conv_il=1)),
    (T12IL, RES, wide40(256), dict(conv_il=1)),
    # ---- persistent k-streams: dense A
    (S8, BOTH, dense(64, 256), {}),
    (S15, BOTH, dense(288, 256), {}),
    (S15N128, BOTH, dense(288, 128), {}),
    (S15N64, BOTH, dense(64, 64), {}),
    # ---- raster halo tiles: 3x3 stride 1 pad 1
    (H288, BOTH, conv3(256), dict(halo_mf=0)),
    (H288MF, BOTH, conv3(256), {}),
    (H288IL, BOTH, conv3(256), dict(conv_il=1)),
    (H320, BOTH, conv3(128), dict(halo_mf=0)),
    (H320MF, BOTH, conv3(128), dict(halo_mf=4)),
    (H320SB, BOTH, conv3(128), {}),
    (H384, BOTH, conv3(64), dict(s3_cfg=13)),
    (H384MF, BOTH, conv3(64), dict(halo_mf=1)),
    (H384P, BOTH, conv3(64), dict(halo_mf=3)),
    (H640, BOTH, conv3(64), {}),
    # ---- 2-D block halo tiles: no residual epilogue
    (B256, NO_RES, wide40(256), {}),
    (B128, NO_RES, conv3(128), dict(halo_2d=1)),
    (B512, NO_RES, WIDE70, {}),
    # ---- N = 512: the instances that walk several column tiles per launch, two of their widest
    (T3, RES, dense(64, 512), dict(s3_cfg=3)),
    (T4, RES, dense(64, 512), dict(s3_cfg=4)),
    (T7, RES, dense(64, 512), dict(s3_cfg=7)),
    (T9, RES, dense(64, 512), dict(s3_cfg=9)),
    (T10, RES, dense(64, 512), dict(s3_cfg=10)),
    (T11, RES, dense(64, 512), dict(s3_cfg=11)),
    (T12, RES, dense(64, 512), dict(s3_cfg=12)),
    (T12IL, RES, dense(64, 512), dict(s3_cfg=12, conv_il=1)),
    (S8, RES, dense(64, 512), {}),
    (S15, RES, dense(288, 512), {}),
    (H288, NO_RES, conv3(512), dict(halo_mf=0)),
    (H288MF, NO_RES, conv3(512), {}),
    (H288IL, NO_RES, conv3(512), dict(conv_il=1)),
    (B256, NO_RES, wide40(512), {}),
]

WITNESSES = [Witness(route, amode_of(geo), residual, relu, geo, knobs)
             for route, residuals, geo, knobs in TABLE for residual in residuals for relu in (False, True)]


def witness_id(w):
    g = w.geometry
    ep = ("res" if w.residual else "nores") + ("+relu" if w.relu else "")
    return f"{w.route} | {w.amode} {g['cin']}->{g['cout']} | {ep}"
