"""Which f16x2 kernel instance serves which conv GEMM: the table of record.

h2_route (csrc/h2_route.hpp) is the one place that decides it, and
rr_h2_route reports its result without a GPU.  Config 15 is bit-identical to
config 12 and the halo forms to each other, so no parity test notices a layer
that moves from one to another; this table does.  Filled from h2_route once it
matched the earlier five-file dispatch on every compared shape; a change here
is a deliberate re-routing and wants a measurement.

Out of scope: the stem (rr_stem_pool_h2) and the stage-entry blocks' fused
conv3 + downsample (rr_bottleneck_out_h2) do not pass launch_gemm_s3.
"""
import pytest

from research_image_retrieval_amd import ops
from research_image_retrieval_amd import weights as W

R = ops.H2Route
# family, cfg, wm, wn, fm, fn, bk, hr, tpk, mf16, nstg, acc, il, pers, t2, chunk_rows
ROUTES = {
    # one tile per block (h2_tile.hip)
    "tile 3, 256x128": R(0, 3, 4, 2, 2, 2, 32, 0, 0, 0, 2, 2, 0, 0, 0, 0),
    "tile 4, 128x256, 16x16x32": R(0, 4, 2, 4, 2, 2, 32, 0, 0, 1, 2, 2, 0, 0, 0, 0),
    "tile 7, 256x64, BK 16": R(0, 7, 8, 1, 1, 2, 16, 0, 0, 0, 2, 2, 0, 0, 0, 0),
    "tile 9, 128x256, 16x16x32, 3 stages": R(0, 9, 2, 4, 2, 2, 32, 0, 0, 1, 3, 2, 0, 0, 0, 0),
    "tile 10, 128x256, 16x16x32, 1 acc": R(0, 10, 2, 4, 2, 2, 32, 0, 0, 1, 2, 1, 0, 0, 0, 0),
    "tile 11, 128x128, 16x16x32, 1 acc": R(0, 11, 2, 2, 2, 2, 32, 0, 0, 1, 2, 1, 0, 0, 0, 0),
    "tile 12, 256x256, 1 acc": R(0, 12, 2, 4, 4, 2, 32, 0, 0, 0, 2, 1, 0, 0, 0, 0),
    "tile 12, 256x256, 1 acc, IL": R(0, 12, 2, 4, 4, 2, 32, 0, 0, 0, 2, 1, 1, 0, 0, 0),
    # persistent k-streams
    "stream 8, 128x256, 16x16x32": R(1, 8, 2, 4, 2, 2, 32, 0, 0, 1, 2, 2, 0, 1, 0, 0),
    "stream 15, 256x256": R(2, 15, 2, 4, 4, 2, 32, 0, 0, 0, 2, 1, 0, 1, 0, 0),
    "stream 15, 256x128": R(2, 15, 2, 4, 4, 1, 32, 0, 0, 0, 2, 1, 0, 1, 0, 0),
    "stream 15, 256x64, 2 acc": R(2, 15, 4, 2, 2, 1, 32, 0, 0, 0, 2, 2, 0, 1, 0, 0),
    # raster halo tiles (h2_halo.hip)
    "halo 288 rows, 256x256, 32x32x16, 1 tap": R(3, 13, 2, 4, 4, 2, 32, 288, 1, 0, 0, 1, 0, 0, 0, 0),
    "halo 288 rows, 256x256, 16x16x32, 1 tap": R(3, 14, 2, 4, 4, 2, 32, 288, 1, 1, 0, 1, 0, 0, 0, 0),
    "halo 288 rows, 256x256, 16x16x32, 1 tap, IL": R(3, 14, 2, 4, 4, 2, 32, 288, 1, 1, 0, 1, 1, 0, 0, 0),
    "halo 320 rows, 256x128, 32x32x16, 1 tap": R(3, 13, 4, 2, 2, 2, 32, 320, 1, 0, 0, 1, 0, 0, 0, 0),
    "halo 320 rows, 256x128, 16x16x32, 1 tap": R(3, 14, 4, 2, 2, 2, 32, 320, 1, 1, 0, 1, 0, 0, 0, 0),
    "halo 320 rows, 256x128, 16x16x32, 3 taps, one buffer": R(3, 14, 4, 2, 2, 2, 32, 320, 3, 1, 0, 1, 0, 2, 0, 0),
    "halo 384 rows, 256x64, 32x32x16, 3 taps": R(3, 13, 4, 2, 2, 1, 32, 384, 3, 0, 0, 1, 0, 0, 0, 0),
    "halo 384 rows, 256x64, 16x16x32, 3 taps": R(3, 14, 4, 2, 2, 1, 32, 384, 3, 1, 0, 1, 0, 0, 0, 0),
    "halo 384 rows, 256x64, 32x32x16, 3 taps, persistent": R(3, 13, 4, 2, 2, 1, 32, 384, 3, 0, 0, 1, 0, 1, 0, 0),
    "halo 640 rows, 512x64, 32x32x16, 3 taps": R(3, 13, 8, 1, 2, 2, 32, 640, 3, 0, 0, 1, 0, 0, 0, 0),
    # 2-D block halo tiles
    "2-D halo 16x16, 256x256, 16x16x32, 1 tap": R(4, 14, 2, 4, 4, 2, 32, 324, 1, 1, 0, 1, 0, 0, 16, 0),
    "2-D halo 16x16, 256x128, 16x16x32, 3 taps, one buffer": R(4, 14, 4, 2, 2, 2, 32, 324, 3, 1, 0, 1, 0, 2, 16, 0),
    "2-D halo 16x32, 512x64, 32x32x16, 3 taps": R(4, 13, 8, 1, 2, 2, 32, 640, 3, 0, 0, 1, 0, 0, 32, 0),
}


def expect(name, chunk_rows=0):
    return ROUTES[name]._replace(chunk_rows=chunk_rows)


# ---- the trunk layers -------------------------------------------------------
def trunk_gemms(arch, h, w):
    """(label, conv geometry) of every conv GEMM of the trunk that passes
    launch_gemm_s3, by resnet_conv_flops' layer walk (its FLOPs pin the
    geometry used here).  Label: layerL.0.* the stage-entry block, layerL.*.*
    the others."""
    def out(x, k, s, p):
        return (x + 2 * p - k) // s + 1

    flops = W.resnet_conv_flops(arch, h, w)
    specs = {name: (cout, cin, k) for name, _, cout, cin, k in W.resnet_conv_specs(arch)}
    H, Wd = out(out(h, 7, 2, 3), 3, 2, 1), out(out(w, 7, 2, 3), 3, 2, 1)
    gemms = []
    for li, nb in enumerate(W.RESNET_LAYERS[arch]):
        for bi in range(nb):
            s1, s2 = W.block_strides(2 if (bi == 0 and li > 0) else 1, "3x3")
            H1, W1 = out(H, 1, s1, 0), out(Wd, 1, s1, 0)
            Ho, Wo = out(H1, 3, s2, 1), out(W1, 3, s2, 1)
            for conv, hin, win, stride, oh, ow in (("conv1", H, Wd, s1, H1, W1), ("conv2", H1, W1, s2, Ho, Wo),
                                                   ("conv3", Ho, Wo, 1, Ho, Wo)):
                name = f"layer{li + 1}.{bi}.{conv}"
                cout, cin, k = specs[name]
                assert flops[name] == 2 * oh * ow * cout * cin * k * k
                if conv == "conv3" and bi == 0:
                    continue  # fused with the downsample projection (rr_bottleneck_out_h2)
                geo = dict(h=hin, w=win, cin=cin, cout=cout, kh=k, kw=k, stride=stride, pad=k // 2,
                           residual=conv == "conv3", relu=True)
                gemms.append((f"layer{li + 1}.{'0' if bi == 0 else '*'}.{conv}", geo))
            H, Wd = Ho, Wo
    return gemms


# (h, w, batch) -> label -> (route, rows per launch)
TRUNK = {
    (96, 128, 4): {
        "layer1.0.conv1": ("stream 15, 256x64, 2 acc", 0),
        "layer1.0.conv2": ("halo 640 rows, 512x64, 32x32x16, 3 taps", 0),
        "layer1.*.conv1": ("stream 15, 256x64, 2 acc", 0),
        "layer1.*.conv2": ("halo 640 rows, 512x64, 32x32x16, 3 taps", 0),
        "layer1.*.conv3": ("stream 8, 128x256, 16x16x32", 0),
        "layer2.0.conv1": ("stream 15, 256x128", 0),
        "layer2.0.conv2": ("tile 11, 128x128, 16x16x32, 1 acc", 0),
        "layer2.*.conv1": ("stream 15, 256x128", 0),
        "layer2.*.conv2": ("halo 320 rows, 256x128, 16x16x32, 3 taps, one buffer", 0),
        "layer2.*.conv3": ("stream 8, 128x256, 16x16x32", 0),
        "layer3.0.conv1": ("stream 15, 256x256", 0),
        "layer3.0.conv2": ("tile 12, 256x256, 1 acc", 0),
        "layer3.*.conv1": ("stream 15, 256x256", 0),
        "layer3.*.conv2": ("halo 288 rows, 256x256, 16x16x32, 1 tap", 0),
        "layer3.*.conv3": ("stream 15, 256x256", 0),
        "layer4.0.conv1": ("stream 15, 256x256", 0),
        "layer4.0.conv2": ("tile 12, 256x256, 1 acc", 0),
        "layer4.*.conv1": ("stream 15, 256x256", 0),
        "layer4.*.conv2": ("halo 288 rows, 256x256, 16x16x32, 1 tap", 0),
        "layer4.*.conv3": ("stream 15, 256x256", 0),
    },
    (224, 224, 64): {
        "layer1.0.conv1": ("stream 15, 256x64, 2 acc", 0),
        "layer1.0.conv2": ("halo 640 rows, 512x64, 32x32x16, 3 taps", 0),
        "layer1.*.conv1": ("stream 15, 256x64, 2 acc", 0),
        "layer1.*.conv2": ("halo 640 rows, 512x64, 32x32x16, 3 taps", 0),
        "layer1.*.conv3": ("stream 8, 128x256, 16x16x32", 0),
        "layer2.0.conv1": ("stream 15, 256x128", 0),
        "layer2.0.conv2": ("tile 11, 128x128, 16x16x32, 1 acc", 0),
        "layer2.*.conv1": ("stream 15, 256x128", 0),
        "layer2.*.conv2": ("halo 320 rows, 256x128, 16x16x32, 3 taps, one buffer", 0),
        "layer2.*.conv3": ("stream 8, 128x256, 16x16x32", 0),
        "layer3.0.conv1": ("stream 15, 256x256", 0),
        "layer3.0.conv2": ("tile 12, 256x256, 1 acc", 0),
        "layer3.*.conv1": ("stream 15, 256x256", 0),
        "layer3.*.conv2": ("halo 288 rows, 256x256, 16x16x32, 1 tap", 0),
        "layer3.*.conv3": ("stream 15, 256x256", 0),
        "layer4.0.conv1": ("stream 15, 256x256", 0),
        "layer4.0.conv2": ("tile 12, 256x256, 1 acc", 0),
        "layer4.*.conv1": ("stream 15, 256x256", 0),
        "layer4.*.conv2": ("halo 288 rows, 256x256, 16x16x32, 1 tap", 0),
        "layer4.*.conv3": ("stream 15, 256x256", 0),
    },
    (1024, 768, 128): {
        "layer1.0.conv1": ("stream 15, 256x64, 2 acc", 0),
        "layer1.0.conv2": ("2-D halo 16x32, 512x64, 32x32x16, 3 taps", 0),
        "layer1.*.conv1": ("stream 15, 256x64, 2 acc", 4194048),
        "layer1.*.conv2": ("2-D halo 16x32, 512x64, 32x32x16, 3 taps", 0),
        "layer1.*.conv3": ("stream 8, 128x256, 16x16x32", 0),
        "layer2.0.conv1": ("stream 15, 256x128", 4194048),
        "layer2.0.conv2": ("tile 11, 128x128, 16x16x32, 1 acc", 0),
        "layer2.*.conv1": ("stream 15, 256x128", 0),
        "layer2.*.conv2": ("2-D halo 16x16, 256x128, 16x16x32, 3 taps, one buffer", 0),
        "layer2.*.conv3": ("stream 8, 128x256, 16x16x32", 0),
        "layer3.0.conv1": ("stream 15, 256x256", 0),
        "layer3.0.conv2": ("tile 12, 256x256, 1 acc", 0),
        "layer3.*.conv1": ("stream 15, 256x256", 0),
        "layer3.*.conv2": ("2-D halo 16x16, 256x256, 16x16x32, 1 tap", 0),
        "layer3.*.conv3": ("stream 15, 256x256", 0),
        "layer4.0.conv1": ("stream 15, 256x256", 0),
        "layer4.0.conv2": ("tile 12, 256x256, 1 acc", 0),
        "layer4.*.conv1": ("stream 15, 256x256", 0),
        "layer4.*.conv2": ("2-D halo 16x16, 256x256, 16x16x32, 1 tap", 0),
        "layer4.*.conv3": ("stream 15, 256x256", 0),
    },
}


@pytest.mark.parametrize("arch", ["resnet50", "resnet101"])
@pytest.mark.parametrize("size", sorted(TRUNK))
def test_trunk_layers(arch, size):
    h, w, batch = size
    table = TRUNK[size]
    seen = {}
    for label, geo in trunk_gemms(arch, h, w):
        assert seen.setdefault(label, geo) == geo, label  # one geometry per table line
        name, chunk_rows = table[label]
        assert ops.h2_route(b=batch, **geo) == expect(name, chunk_rows), (label, geo)
    assert set(seen) == set(table)


# ---- forced knobs -----------------------------------------------------------
FORCED_SHAPES = {
    "3x3 64@56": dict(b=64, h=56, w=56, cin=64, cout=64, kh=3, kw=3, stride=1, pad=1, relu=True),
    "3x3 128@28": dict(b=64, h=28, w=28, cin=128, cout=128, kh=3, kw=3, stride=1, pad=1, relu=True),
    "3x3 256@14": dict(b=64, h=14, w=14, cin=256, cout=256, kh=3, kw=3, stride=1, pad=1, relu=True),
    "dense 256->1024 + residual": dict(b=64, h=14, w=14, cin=256, cout=1024, residual=True, relu=True),
    "dense 64->256 + residual": dict(b=64, h=56, w=56, cin=64, cout=256, residual=True, relu=True),
}
KNOBS = ("halo_mf", "halo_2d", "conv_il")
KNOB_VALUES = {"halo_mf": (-1, 0, 1, 2, 3, 4), "halo_2d": (-1, 0, 1), "conv_il": (0, 1)}
# shape -> s3_cfg -> route under every value of the three knobs, or (the knobs
# it depends on, {their values: route})
FORCED = {
    "3x3 64@56": {
        0: (('halo_mf', 'halo_2d'), {
            (-1, -1): "halo 640 rows, 512x64, 32x32x16, 3 taps",
            (-1, 0): "halo 640 rows, 512x64, 32x32x16, 3 taps",
            (-1, 1): "2-D halo 16x32, 512x64, 32x32x16, 3 taps",
            (0, -1): "halo 640 rows, 512x64, 32x32x16, 3 taps",
            (0, 0): "halo 640 rows, 512x64, 32x32x16, 3 taps",
            (0, 1): "2-D halo 16x32, 512x64, 32x32x16, 3 taps",
            (1, -1): "halo 384 rows, 256x64, 16x16x32, 3 taps",
            (1, 0): "halo 384 rows, 256x64, 16x16x32, 3 taps",
            (1, 1): "2-D halo 16x32, 512x64, 32x32x16, 3 taps",
            (2, -1): "halo 640 rows, 512x64, 32x32x16, 3 taps",
            (2, 0): "halo 640 rows, 512x64, 32x32x16, 3 taps",
            (2, 1): "2-D halo 16x32, 512x64, 32x32x16, 3 taps",
            (3, -1): "halo 384 rows, 256x64, 32x32x16, 3 taps, persistent",
            (3, 0): "halo 384 rows, 256x64, 32x32x16, 3 taps, persistent",
            (3, 1): "2-D halo 16x32, 512x64, 32x32x16, 3 taps",
            (4, -1): "halo 384 rows, 256x64, 16x16x32, 3 taps",
            (4, 0): "halo 384 rows, 256x64, 16x16x32, 3 taps",
            (4, 1): "2-D halo 16x32, 512x64, 32x32x16, 3 taps",
        }),
        1: "tile 7, 256x64, BK 16",
        2: "tile 7, 256x64, BK 16",
        3: "tile 3, 256x128",
        4: "tile 4, 128x256, 16x16x32",
        5: "tile 7, 256x64, BK 16",
        6: "tile 7, 256x64, BK 16",
        7: "tile 7, 256x64, BK 16",
        8: "tile 7, 256x64, BK 16",
        9: "tile 7, 256x64, BK 16",
        10: "tile 7, 256x64, BK 16",
        11: "tile 7, 256x64, BK 16",
        12: "tile 7, 256x64, BK 16",
        13: "halo 384 rows, 256x64, 32x32x16, 3 taps",
        14: "halo 384 rows, 256x64, 16x16x32, 3 taps",
        15: (('halo_mf', 'halo_2d'), {
            (-1, -1): "halo 384 rows, 256x64, 32x32x16, 3 taps",
            (-1, 0): "halo 384 rows, 256x64, 32x32x16, 3 taps",
            (-1, 1): "2-D halo 16x32, 512x64, 32x32x16, 3 taps",
            (0, -1): "halo 384 rows, 256x64, 32x32x16, 3 taps",
            (0, 0): "halo 384 rows, 256x64, 32x32x16, 3 taps",
            (0, 1): "2-D halo 16x32, 512x64, 32x32x16, 3 taps",
            (1, -1): "halo 384 rows, 256x64, 16x16x32, 3 taps",
            (1, 0): "halo 384 rows, 256x64, 16x16x32, 3 taps",
            (1, 1): "2-D halo 16x32, 512x64, 32x32x16, 3 taps",
            (2, -1): "halo 640 rows, 512x64, 32x32x16, 3 taps",
            (2, 0): "halo 640 rows, 512x64, 32x32x16, 3 taps",
            (2, 1): "2-D halo 16x32, 512x64, 32x32x16, 3 taps",
            (3, -1): "halo 384 rows, 256x64, 32x32x16, 3 taps, persistent",
            (3, 0): "halo 384 rows, 256x64, 32x32x16, 3 taps, persistent",
            (3, 1): "2-D halo 16x32, 512x64, 32x32x16, 3 taps",
            (4, -1): "halo 384 rows, 256x64, 16x16x32, 3 taps",
            (4, 0): "halo 384 rows, 256x64, 16x16x32, 3 taps",
            (4, 1): "2-D halo 16x32, 512x64, 32x32x16, 3 taps",
        }),
    },
    "3x3 128@28": {
        0: (('halo_mf', 'halo_2d'), {
            (-1, -1): "halo 320 rows, 256x128, 16x16x32, 3 taps, one buffer",
            (-1, 0): "halo 320 rows, 256x128, 16x16x32, 3 taps, one buffer",
            (-1, 1): "2-D halo 16x16, 256x128, 16x16x32, 3 taps, one buffer",
            (0, -1): "halo 320 rows, 256x128, 32x32x16, 1 tap",
            (0, 0): "halo 320 rows, 256x128, 32x32x16, 1 tap",
            (0, 1): "2-D halo 16x16, 256x128, 16x16x32, 3 taps, one buffer",
            (1, -1): "halo 320 rows, 256x128, 16x16x32, 3 taps, one buffer",
            (1, 0): "halo 320 rows, 256x128, 16x16x32, 3 taps, one buffer",
            (1, 1): "2-D halo 16x16, 256x128, 16x16x32, 3 taps, one buffer",
            (2, -1): "halo 320 rows, 256x128, 32x32x16, 1 tap",
            (2, 0): "halo 320 rows, 256x128, 32x32x16, 1 tap",
            (2, 1): "2-D halo 16x16, 256x128, 16x16x32, 3 taps, one buffer",
            (3, -1): "halo 320 rows, 256x128, 32x32x16, 1 tap",
            (3, 0): "halo 320 rows, 256x128, 32x32x16, 1 tap",
            (3, 1): "2-D halo 16x16, 256x128, 16x16x32, 3 taps, one buffer",
            (4, -1): "halo 320 rows, 256x128, 16x16x32, 1 tap",
            (4, 0): "halo 320 rows, 256x128, 16x16x32, 1 tap",
            (4, 1): "2-D halo 16x16, 256x128, 16x16x32, 3 taps, one buffer",
        }),
        1: "tile 3, 256x128",
        2: "tile 3, 256x128",
        3: "tile 3, 256x128",
        4: "tile 4, 128x256, 16x16x32",
        5: "tile 3, 256x128",
        6: "tile 3, 256x128",
        7: "tile 7, 256x64, BK 16",
        8: "tile 11, 128x128, 16x16x32, 1 acc",
        9: "tile 11, 128x128, 16x16x32, 1 acc",
        10: "tile 11, 128x128, 16x16x32, 1 acc",
        11: "tile 11, 128x128, 16x16x32, 1 acc",
        12: "tile 11, 128x128, 16x16x32, 1 acc",
        13: "halo 320 rows, 256x128, 32x32x16, 1 tap",
        14: "halo 320 rows, 256x128, 16x16x32, 3 taps, one buffer",
        15: (('halo_mf', 'halo_2d'), {
            (-1, -1): "halo 320 rows, 256x128, 16x16x32, 3 taps, one buffer",
            (-1, 0): "halo 320 rows, 256x128, 16x16x32, 3 taps, one buffer",
            (-1, 1): "2-D halo 16x16, 256x128, 16x16x32, 3 taps, one buffer",
            (0, -1): "halo 320 rows, 256x128, 32x32x16, 1 tap",
            (0, 0): "halo 320 rows, 256x128, 32x32x16, 1 tap",
            (0, 1): "2-D halo 16x16, 256x128, 16x16x32, 3 taps, one buffer",
            (1, -1): "halo 320 rows, 256x128, 16x16x32, 3 taps, one buffer",
            (1, 0): "halo 320 rows, 256x128, 16x16x32, 3 taps, one buffer",
            (1, 1): "2-D halo 16x16, 256x128, 16x16x32, 3 taps, one buffer",
            (2, -1): "halo 320 rows, 256x128, 32x32x16, 1 tap",
            (2, 0): "halo 320 rows, 256x128, 32x32x16, 1 tap",
            (2, 1): "2-D halo 16x16, 256x128, 16x16x32, 3 taps, one buffer",
            (3, -1): "halo 320 rows, 256x128, 32x32x16, 1 tap",
            (3, 0): "halo 320 rows, 256x128, 32x32x16, 1 tap",
            (3, 1): "2-D halo 16x16, 256x128, 16x16x32, 3 taps, one buffer",
            (4, -1): "halo 320 rows, 256x128, 16x16x32, 1 tap",
            (4, 0): "halo 320 rows, 256x128, 16x16x32, 1 tap",
            (4, 1): "2-D halo 16x16, 256x128, 16x16x32, 3 taps, one buffer",
        }),
    },
    "3x3 256@14": {
        0: (('halo_mf', 'halo_2d', 'conv_il'), {
            (-1, -1, 0): "halo 288 rows, 256x256, 16x16x32, 1 tap",
            (-1, -1, 1): "halo 288 rows, 256x256, 16x16x32, 1 tap, IL",
            (-1, 0, 0): "halo 288 rows, 256x256, 16x16x32, 1 tap",
            (-1, 0, 1): "halo 288 rows, 256x256, 16x16x32, 1 tap, IL",
            (-1, 1, 0): "2-D halo 16x16, 256x256, 16x16x32, 1 tap",
            (-1, 1, 1): "2-D halo 16x16, 256x256, 16x16x32, 1 tap",
            (0, -1, 0): "halo 288 rows, 256x256, 32x32x16, 1 tap",
            (0, -1, 1): "halo 288 rows, 256x256, 32x32x16, 1 tap",
            (0, 0, 0): "halo 288 rows, 256x256, 32x32x16, 1 tap",
            (0, 0, 1): "halo 288 rows, 256x256, 32x32x16, 1 tap",
            (0, 1, 0): "2-D halo 16x16, 256x256, 16x16x32, 1 tap",
            (0, 1, 1): "2-D halo 16x16, 256x256, 16x16x32, 1 tap",
            (1, -1, 0): "halo 288 rows, 256x256, 16x16x32, 1 tap",
            (1, -1, 1): "halo 288 rows, 256x256, 16x16x32, 1 tap, IL",
            (1, 0, 0): "halo 288 rows, 256x256, 16x16x32, 1 tap",
            (1, 0, 1): "halo 288 rows, 256x256, 16x16x32, 1 tap, IL",
            (1, 1, 0): "2-D halo 16x16, 256x256, 16x16x32, 1 tap",
            (1, 1, 1): "2-D halo 16x16, 256x256, 16x16x32, 1 tap",
            (2, -1, 0): "halo 288 rows, 256x256, 32x32x16, 1 tap",
            (2, -1, 1): "halo 288 rows, 256x256, 32x32x16, 1 tap",
            (2, 0, 0): "halo 288 rows, 256x256, 32x32x16, 1 tap",
            (2, 0, 1): "halo 288 rows, 256x256, 32x32x16, 1 tap",
            (2, 1, 0): "2-D halo 16x16, 256x256, 16x16x32, 1 tap",
            (2, 1, 1): "2-D halo 16x16, 256x256, 16x16x32, 1 tap",
            (3, -1, 0): "halo 288 rows, 256x256, 32x32x16, 1 tap",
            (3, -1, 1): "halo 288 rows, 256x256, 32x32x16, 1 tap",
            (3, 0, 0): "halo 288 rows, 256x256, 32x32x16, 1 tap",
            (3, 0, 1): "halo 288 rows, 256x256, 32x32x16, 1 tap",
            (3, 1, 0): "2-D halo 16x16, 256x256, 16x16x32, 1 tap",
            (3, 1, 1): "2-D halo 16x16, 256x256, 16x16x32, 1 tap",
            (4, -1, 0): "halo 288 rows, 256x256, 16x16x32, 1 tap",
            (4, -1, 1): "halo 288 rows, 256x256, 16x16x32, 1 tap, IL",
            (4, 0, 0): "halo 288 rows, 256x256, 16x16x32, 1 tap",
            (4, 0, 1): "halo 288 rows, 256x256, 16x16x32, 1 tap, IL",
            (4, 1, 0): "2-D halo 16x16, 256x256, 16x16x32, 1 tap",
            (4, 1, 1): "2-D halo 16x16, 256x256, 16x16x32, 1 tap",
        }),
        1: "tile 4, 128x256, 16x16x32",
        2: "tile 4, 128x256, 16x16x32",
        3: "tile 3, 256x128",
        4: "tile 4, 128x256, 16x16x32",
        5: "tile 4, 128x256, 16x16x32",
        6: "tile 4, 128x256, 16x16x32",
        7: "tile 7, 256x64, BK 16",
        8: "tile 4, 128x256, 16x16x32",
        9: "tile 9, 128x256, 16x16x32, 3 stages",
        10: "tile 10, 128x256, 16x16x32, 1 acc",
        11: "tile 11, 128x128, 16x16x32, 1 acc",
        12: (('conv_il',), {
            (0,): "tile 12, 256x256, 1 acc",
            (1,): "tile 12, 256x256, 1 acc, IL",
        }),
        13: "halo 288 rows, 256x256, 32x32x16, 1 tap",
        14: (('conv_il',), {
            (0,): "halo 288 rows, 256x256, 16x16x32, 1 tap",
            (1,): "halo 288 rows, 256x256, 16x16x32, 1 tap, IL",
        }),
        15: (('halo_mf', 'halo_2d', 'conv_il'), {
            (-1, -1, 0): "halo 288 rows, 256x256, 16x16x32, 1 tap",
            (-1, -1, 1): "halo 288 rows, 256x256, 16x16x32, 1 tap, IL",
            (-1, 0, 0): "halo 288 rows, 256x256, 16x16x32, 1 tap",
            (-1, 0, 1): "halo 288 rows, 256x256, 16x16x32, 1 tap, IL",
            (-1, 1, 0): "2-D halo 16x16, 256x256, 16x16x32, 1 tap",
            (-1, 1, 1): "2-D halo 16x16, 256x256, 16x16x32, 1 tap",
            (0, -1, 0): "halo 288 rows, 256x256, 32x32x16, 1 tap",
            (0, -1, 1): "halo 288 rows, 256x256, 32x32x16, 1 tap",
            (0, 0, 0): "halo 288 rows, 256x256, 32x32x16, 1 tap",
            (0, 0, 1): "halo 288 rows, 256x256, 32x32x16, 1 tap",
            (0, 1, 0): "2-D halo 16x16, 256x256, 16x16x32, 1 tap",
            (0, 1, 1): "2-D halo 16x16, 256x256, 16x16x32, 1 tap",
            (1, -1, 0): "halo 288 rows, 256x256, 16x16x32, 1 tap",
            (1, -1, 1): "halo 288 rows, 256x256, 16x16x32, 1 tap, IL",
            (1, 0, 0): "halo 288 rows, 256x256, 16x16x32, 1 tap",
            (1, 0, 1): "halo 288 rows, 256x256, 16x16x32, 1 tap, IL",
            (1, 1, 0): "2-D halo 16x16, 256x256, 16x16x32, 1 tap",
            (1, 1, 1): "2-D halo 16x16, 256x256, 16x16x32, 1 tap",
            (2, -1, 0): "halo 288 rows, 256x256, 32x32x16, 1 tap",
            (2, -1, 1): "halo 288 rows, 256x256, 32x32x16, 1 tap",
            (2, 0, 0): "halo 288 rows, 256x256, 32x32x16, 1 tap",
            (2, 0, 1): "halo 288 rows, 256x256, 32x32x16, 1 tap",
            (2, 1, 0): "2-D halo 16x16, 256x256, 16x16x32, 1 tap",
            (2, 1, 1): "2-D halo 16x16, 256x256, 16x16x32, 1 tap",
            (3, -1, 0): "halo 288 rows, 256x256, 32x32x16, 1 tap",
            (3, -1, 1): "halo 288 rows, 256x256, 32x32x16, 1 tap",
            (3, 0, 0): "halo 288 rows, 256x256, 32x32x16, 1 tap",
            (3, 0, 1): "halo 288 rows, 256x256, 32x32x16, 1 tap",
            (3, 1, 0): "2-D halo 16x16, 256x256, 16x16x32, 1 tap",
            (3, 1, 1): "2-D halo 16x16, 256x256, 16x16x32, 1 tap",
            (4, -1, 0): "halo 288 rows, 256x256, 16x16x32, 1 tap",
            (4, -1, 1): "halo 288 rows, 256x256, 16x16x32, 1 tap, IL",
            (4, 0, 0): "halo 288 rows, 256x256, 16x16x32, 1 tap",
            (4, 0, 1): "halo 288 rows, 256x256, 16x16x32, 1 tap, IL",
            (4, 1, 0): "2-D halo 16x16, 256x256, 16x16x32, 1 tap",
            (4, 1, 1): "2-D halo 16x16, 256x256, 16x16x32, 1 tap",
        }),
    },
    "dense 256->1024 + residual": {
        0: "stream 15, 256x256",
        1: "tile 4, 128x256, 16x16x32",
        2: "tile 4, 128x256, 16x16x32",
        3: "tile 3, 256x128",
        4: "tile 4, 128x256, 16x16x32",
        5: "tile 4, 128x256, 16x16x32",
        6: "tile 4, 128x256, 16x16x32",
        7: "tile 7, 256x64, BK 16",
        8: "stream 8, 128x256, 16x16x32",
        9: "tile 9, 128x256, 16x16x32, 3 stages",
        10: "tile 10, 128x256, 16x16x32, 1 acc",
        11: "tile 11, 128x128, 16x16x32, 1 acc",
        12: (('conv_il',), {
            (0,): "tile 12, 256x256, 1 acc",
            (1,): "tile 12, 256x256, 1 acc, IL",
        }),
        13: (('conv_il',), {
            (0,): "tile 12, 256x256, 1 acc",
            (1,): "tile 12, 256x256, 1 acc, IL",
        }),
        14: (('conv_il',), {
            (0,): "tile 12, 256x256, 1 acc",
            (1,): "tile 12, 256x256, 1 acc, IL",
        }),
        15: "stream 15, 256x256",
    },
    "dense 64->256 + residual": {
        0: "stream 8, 128x256, 16x16x32",
        1: "tile 4, 128x256, 16x16x32",
        2: "tile 4, 128x256, 16x16x32",
        3: "tile 3, 256x128",
        4: "tile 4, 128x256, 16x16x32",
        5: "tile 4, 128x256, 16x16x32",
        6: "tile 4, 128x256, 16x16x32",
        7: "tile 7, 256x64, BK 16",
        8: "stream 8, 128x256, 16x16x32",
        9: "tile 9, 128x256, 16x16x32, 3 stages",
        10: "tile 10, 128x256, 16x16x32, 1 acc",
        11: "tile 11, 128x128, 16x16x32, 1 acc",
        12: (('conv_il',), {
            (0,): "tile 12, 256x256, 1 acc",
            (1,): "tile 12, 256x256, 1 acc, IL",
        }),
        13: "stream 8, 128x256, 16x16x32",
        14: "stream 8, 128x256, 16x16x32",
        15: "stream 8, 128x256, 16x16x32",
    },
}


def forced_cases():
    for shape in FORCED_SHAPES:
        for cfg in range(16):
            yield shape, cfg


@pytest.mark.parametrize("shape,cfg", list(forced_cases()))
def test_forced_knobs(shape, cfg):
    geo = FORCED_SHAPES[shape]
    want = FORCED[shape][cfg]
    for mf in KNOB_VALUES["halo_mf"]:
        for h2d in KNOB_VALUES["halo_2d"]:
            for il in KNOB_VALUES["conv_il"]:
                knobs = dict(halo_mf=mf, halo_2d=h2d, conv_il=il)
                name = want if isinstance(want, str) else want[1][tuple(knobs[k] for k in want[0])]
                # the dense shapes carry a residual: s3_cfg_res overrides s3_cfg for them
                got = ops.h2_route(s3_cfg=cfg, **knobs, **geo)
                assert got == expect(name), (shape, cfg, knobs)
                if geo.get("residual"):
                    assert ops.h2_route(s3_cfg=3, s3_cfg_res=cfg, **knobs, **geo) == (got if cfg else expect("tile 3, 256x128"))
                else:
                    assert ops.h2_route(s3_cfg=cfg, s3_cfg_res=3, **knobs, **geo) == got


# ---- boundaries -------------------------------------------------------------
def conv3(b, hw, c, **kw):
    return dict(b=b, h=hw, w=hw, cin=c, cout=c, kh=3, kw=3, stride=1, pad=1, relu=True, **kw)


BOUNDARIES = [
    ("N 256, W 15: 288 rows hold it", conv3(64, 15, 256),
     "halo 288 rows, 256x256, 16x16x32, 1 tap", 0),
    ("N 256, W 16: past 288 rows", conv3(64, 16, 256),
     "2-D halo 16x16, 256x256, 16x16x32, 1 tap", 0),
    ("N 256, W 16, halo_2d 0", conv3(64, 16, 256, halo_2d=0),
     "tile 12, 256x256, 1 acc", 0),
    ("N 128, W 31: 320 rows hold it", conv3(64, 31, 128),
     "halo 320 rows, 256x128, 16x16x32, 3 taps, one buffer", 0),
    ("N 128, W 32: past 320 rows", conv3(64, 32, 128),
     "2-D halo 16x16, 256x128, 16x16x32, 3 taps, one buffer", 0),
    ("N 128, W 32, halo_2d 0", conv3(64, 32, 128, halo_2d=0),
     "tile 11, 128x128, 16x16x32, 1 acc", 0),
    ("N 64, W 63: 384 rows hold it", conv3(64, 63, 64, s3_cfg=13),
     "halo 384 rows, 256x64, 32x32x16, 3 taps", 0),
    ("N 64, W 64: past 384 rows", conv3(64, 64, 64, s3_cfg=13),
     "tile 7, 256x64, BK 16", 0),
    ("N 64, W 63: 640 rows hold it", conv3(64, 63, 64),
     "halo 640 rows, 512x64, 32x32x16, 3 taps", 0),
    ("N 64, W 64: past 640 rows", conv3(64, 64, 64),
     "2-D halo 16x32, 512x64, 32x32x16, 3 taps", 0),
    ("N 64, W 63, halo_mf 2", conv3(64, 63, 64, halo_mf=2, halo_2d=0),
     "halo 640 rows, 512x64, 32x32x16, 3 taps", 0),
    ("N 64, W 64, halo_mf 2, halo_2d 0", conv3(64, 64, 64, halo_mf=2, halo_2d=0),
     "tile 7, 256x64, BK 16", 0),
    ("dense K 224, N 256", dict(b=64, h=14, w=14, cin=224, cout=256),
     "stream 8, 128x256, 16x16x32", 0),
    ("dense K 256, N 256", dict(b=64, h=14, w=14, cin=256, cout=256),
     "stream 15, 256x256", 0),
    ("1x1 stride 2 K 224, N 256", dict(b=64, h=14, w=14, cin=224, cout=256, stride=2),
     "tile 4, 128x256, 16x16x32", 0),
    ("1x1 stride 2 K 256, N 256", dict(b=64, h=14, w=14, cin=256, cout=256, stride=2),
     "tile 12, 256x256, 1 acc", 0),
    ("dense K 256, N 64", dict(b=64, h=14, w=14, cin=256, cout=64),
     "stream 15, 256x64, 2 acc", 0),
    ("dense K 256, N 128", dict(b=64, h=14, w=14, cin=256, cout=128),
     "stream 15, 256x128", 0),
    ("dense K 256, N 192", dict(b=64, h=14, w=14, cin=256, cout=192),
     "tile 3, 256x128", 0),
    ("dense K 32, N 64", dict(b=64, h=14, w=14, cin=32, cout=64),
     "tile 3, 256x128", 0),
    ("dense K 224, N 128", dict(b=64, h=14, w=14, cin=224, cout=128),
     "tile 11, 128x128, 16x16x32, 1 acc", 0),
    ("3x3 stride 2, N 64", dict(b=64, h=56, w=56, cin=64, cout=64, kh=3, kw=3, stride=2, pad=1),
     "tile 3, 256x128", 0),
    ("3x3 stride 2, N 128", dict(b=64, h=56, w=56, cin=128, cout=128, kh=3, kw=3, stride=2, pad=1),
     "tile 11, 128x128, 16x16x32, 1 acc", 0),
    ("3x3 stride 2, N 192", dict(b=64, h=56, w=56, cin=64, cout=192, kh=3, kw=3, stride=2, pad=1),
     "tile 3, 256x128", 0),
    ("3x3 stride 2, N 256", dict(b=64, h=28, w=28, cin=256, cout=256, kh=3, kw=3, stride=2, pad=1),
     "tile 12, 256x256, 1 acc", 0),
    ("M 2^22 - 1 rows of 1 KB: below 4 GB", dict(b=(1 << 22) - 1, h=1, w=1, cin=256, cout=64),
     "stream 15, 256x64, 2 acc", 0),
    ("M 2^22 rows of 1 KB: 4 GB", dict(b=1 << 22, h=1, w=1, cin=256, cout=64),
     "stream 15, 256x64, 2 acc", 4194048),
    ("C of 4 GB (ldc 1024)", dict(b=1 << 20, h=1, w=1, cin=256, cout=1024),
     "stream 15, 256x256", 1048320),
    ("4 GB, forced 12: one launch of the tile", dict(b=1 << 22, h=1, w=1, cin=256, cout=256, s3_cfg=12),
     "tile 12, 256x256, 1 acc", 0),
    ("N 128 2-D, 255 blocks", dict(b=85, h=16, w=48, cin=128, cout=128, kh=3, kw=3, stride=1, pad=1),
     "tile 11, 128x128, 16x16x32, 1 acc", 0),
    ("N 128 2-D, 256 blocks", dict(b=128, h=16, w=32, cin=128, cout=128, kh=3, kw=3, stride=1, pad=1),
     "2-D halo 16x16, 256x128, 16x16x32, 3 taps, one buffer", 0),
    ("N 128 2-D, 255 blocks, halo_2d 1", dict(b=85, h=16, w=48, cin=128, cout=128, kh=3, kw=3, stride=1, pad=1, halo_2d=1),
     "2-D halo 16x16, 256x128, 16x16x32, 3 taps, one buffer", 0),
    ("N 128, W 28, halo_2d 1", conv3(1, 28, 128, halo_2d=1),
     "2-D halo 16x16, 256x128, 16x16x32, 3 taps, one buffer", 0),
    ("2-D halo tiles have no residual epilogue", conv3(64, 16, 256, residual=True),
     "tile 12, 256x256, 1 acc", 0),
]


@pytest.mark.parametrize("what,geo,name,chunk_rows", BOUNDARIES, ids=[b[0] for b in BOUNDARIES])
def test_boundaries(what, geo, name, chunk_rows):
    assert ops.h2_route(**geo) == expect(name, chunk_rows)


# ---- rejection --------------------------------------------------------------
OK_SHAPE = dict(b=2, h=14, w=14, cin=64, cout=64, kh=3, kw=3, stride=1, pad=1)


@pytest.mark.parametrize("bad", [
    dict(cin=48), dict(cin=3), dict(cout=6), dict(cout=0), dict(b=-1), dict(h=0), dict(kh=0), dict(stride=0),
    dict(pad=-1), dict(h=1, pad=0),            # empty output
    dict(b=1 << 20, h=64, w=64),               # 2^32 output pixels
    dict(s3_cfg=16), dict(s3_cfg=-1), dict(s3_cfg_res=16), dict(halo_mf=5), dict(halo_mf=-2), dict(halo_2d=2),
    dict(conv_il=2),
], ids=str)
def test_rejected(bad):
    ops.h2_route(**OK_SHAPE)
    with pytest.raises(ValueError):
        ops.h2_route(**{**OK_SHAPE, **bad})


def test_relu_out_of_range_is_rejected_by_the_entry():
    import ctypes
    from research_image_retrieval_amd import _lib
    shape = (ctypes.c_int * 11)(2, 14, 14, 64, 64, 3, 3, 1, 1, 0, 2)
    tune = (ctypes.c_int * 5)(0, 0, -1, -1, -1)
    out = (ctypes.c_int * 18)()
    args = [ctypes.cast(a, ctypes.c_void_p) for a in (shape, tune, out)]
    assert _lib.lib().rr_h2_route(*args) == _lib.RR_EINVAL
    shape[10] = 1
    assert _lib.lib().rr_h2_route(*args) == 0
    assert _lib.lib().rr_h2_route(None, args[1], args[2]) == _lib.RR_EINVAL
