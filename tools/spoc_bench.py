"""SpoC on the device: every launch of the head at (b, H x W) = (64, 7 x 7) and
(1, 7 x 7) with its bytes or FLOPs, its rate and the share of the measured copy
rate or of the exact-fp32 MFMA peak it reaches; rr_spoc_refine and
rr_linear_groupmax against the compositions of EXISTING entries that compute
the same thing in the same process (rr_linear_ex over all rows, then the torch
elementwise op or amax); and SpoCWrapper.forward_test beside
GeMWrapper.forward_test at 64 x 224x224 R50 with the head's share.

Device events around --iters calls; legs are alternated in one process after a
warm-up, and the median (min - max) over --rounds is reported (DESIGN.md §
Numbers (SpoC head)).  HBM: 8.0 TB/s spec, 6.29 TB/s measured for a float4
copy; the exact-fp32 MFMA peak is 157 TFLOP/s.

    python tools/spoc_bench.py [--rounds 7] [--iters 20] [--conv-math h2] [--skip-model]
"""
import argparse
import os
import statistics
import sys

import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
from research_image_retrieval_amd import models, ops  # noqa: E402

HBM_COPY = 6.29e12   # B/s, measured float4 copy
MFMA_F32 = 157e12    # FLOP/s, v_mfma_f32_* with fp32 inputs
C, DC, F, LEVELS = 2048, 512, 2048, [1, 2, 4]


def t_ms(fn, iters):
    s, e = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    s.record()
    for _ in range(iters):
        fn()
    e.record()
    torch.cuda.synchronize()
    return s.elapsed_time(e) / iters


def alternated(legs, rounds, iters, warm=2):
    """legs: name -> callable.  (median, min, max) ms per call of each leg over
    `rounds` rounds that run every leg once, in turn."""
    for fn in legs.values():
        for _ in range(warm):
            fn()
    torch.cuda.synchronize()
    ts = {k: [] for k in legs}
    for _ in range(rounds):
        for k, fn in legs.items():
            ts[k].append(t_ms(fn, iters))
    return {k: (statistics.median(v), min(v), max(v)) for k, v in ts.items()}


def us(t):
    return f"{t[0] * 1e3:.1f} us ({t[1] * 1e3:.1f} - {t[2] * 1e3:.1f})"


def rate(t, nbytes=None, flops=None):
    if flops is not None:
        r = flops / (t[0] * 1e-3)
        return f"{flops / 1e9:.2f} GFLOP -> {r / 1e12:.1f} TFLOP/s = {100 * r / MFMA_F32:.1f} % of the fp32 MFMA peak"
    r = nbytes / (t[0] * 1e-3)
    return f"{nbytes / 1e6:.2f} MB -> {r / 1e9:.0f} GB/s = {100 * r / HBM_COPY:.1f} % of the copy rate"


def head_launches(m, b, hgt, wid, x4, x4a, a):
    """The head's launches one by one on x4, as SpoCModel.head issues them."""
    n = hgt * wid
    r = ops.spp_regions(hgt, wid, LEVELS)
    w = m.w
    c1a = ops.amax_records(1, x4.device)[0] if m.conv_math == "h2" else None
    c1 = m.convs["ce0_w"](x4, x4a, w["ce0_b"], pad=1, relu=True, y_amax=c1a)
    ctx = m.convs["ce1_w"](c1, c1a, w["ce1_b"], pad=1, relu=True)
    u = m.convs["refine_wx"](x4, x4a, None)
    refined = ops.spoc_refine(u, ctx, w["att_w"], m.att_b, w["refine_wc"], w["refine_b"])
    pooled = ops.spp_max(refined, LEVELS)
    agg = ops.linear_groupmax(pooled, w["agg_w"], w["agg_b"], act=1)
    hidden = ops.linear_splitk(agg, w["fp0_w"], w["fp0_b"], act=1)
    feats = ops.linear_splitk(hidden, w["fp3_w"], w["fp3_b"])

    def conv0():
        if c1a is not None:
            c1a.zero_()
        return m.convs["ce0_w"](x4, x4a, w["ce0_b"], pad=1, relu=True, y_amax=c1a)

    legs = {"conv3x3 2048->512": conv0,
            "conv3x3 512->512": lambda: m.convs["ce1_w"](c1, c1a, w["ce1_b"], pad=1, relu=True),
            "conv1x1 Wx": lambda: m.convs["refine_wx"](x4, x4a, None),
            "spoc_refine": lambda: ops.spoc_refine(u, ctx, w["att_w"], m.att_b, w["refine_wc"], w["refine_b"]),
            "spp_max": lambda: ops.spp_max(refined, LEVELS),
            "linear_groupmax": lambda: ops.linear_groupmax(pooled, w["agg_w"], w["agg_b"], act=1),
            "linear_splitk relu": lambda: ops.linear_splitk(agg, w["fp0_w"], w["fp0_b"], act=1),
            "linear_splitk": lambda: ops.linear_splitk(hidden, w["fp3_w"], w["fp3_b"]),
            "l2_normalize": lambda: ops.l2_normalize(feats, 1e-12)}
    t = alternated(legs, a.rounds, a.iters)
    rows = b * n
    cost = {"conv3x3 2048->512": dict(flops=2.0 * rows * 9 * C * DC),
            "conv3x3 512->512": dict(flops=2.0 * rows * 9 * DC * DC),
            "conv1x1 Wx": dict(flops=2.0 * rows * C * C), "spoc_refine": dict(flops=2.0 * rows * DC * C),
            "spp_max": dict(nbytes=4.0 * (rows * C + b * r * C)), "linear_groupmax": dict(flops=2.0 * b * r * C * F),
            "linear_splitk relu": dict(nbytes=4.0 * F * F), "linear_splitk": dict(nbytes=4.0 * F * F),
            "l2_normalize": dict(nbytes=8.0 * b * F)}
    print(f"head launches at (b, H x W) = ({b}, {hgt} x {wid}), {m.conv_math} (the 3x3 and Wx convs run on that core, "
          f"their share is of the fp32 MFMA peak all the same):")
    for k, v in t.items():
        print(f"   {k}: {us(v)}; {rate(v, **cost[k])}", flush=True)
    print(f"   sum of the medians {sum(v[0] for v in t.values()) * 1e3:.1f} us", flush=True)
    return u, ctx, pooled


def compositions(m, b, u, ctx, pooled, a):
    """The fused entries against rr_linear_ex + torch on the same tensors."""
    w = m.w
    rows = u.numel() // C
    u2, ctx2 = u.view(rows, C), ctx.view(rows, DC)
    watt = w["att_w"].view(1, DC)

    def unfused_refine():
        lin = ops.linear_ex(ctx2, w["refine_wc"], w["refine_b"])
        att = torch.sigmoid(ops.linear_ex(ctx2, watt) + m.att_b)
        return torch.addcmul(lin, u2, att)

    def unfused_groupmax():
        y = ops.linear_ex(pooled.view(-1, C), w["agg_w"], w["agg_b"], act=1)
        return y.view(b, -1, F).amax(dim=1)

    fused = ops.spoc_refine(u2, ctx2, w["att_w"], m.att_b, w["refine_wc"], w["refine_b"])
    d1 = (fused - unfused_refine()).abs().max().item()
    d2 = (ops.linear_groupmax(pooled, w["agg_w"], w["agg_b"], act=1) - unfused_groupmax()).abs().max().item()
    t = alternated({"refine": lambda: ops.spoc_refine(u2, ctx2, w["att_w"], m.att_b, w["refine_wc"], w["refine_b"]),
                    "refine unfused": unfused_refine,
                    "groupmax": lambda: ops.linear_groupmax(pooled, w["agg_w"], w["agg_b"], act=1),
                    "groupmax unfused": unfused_groupmax}, a.rounds, a.iters)
    print(f"b = {b}: rr_spoc_refine {us(t['refine'])} | rr_linear_ex x 2 + sigmoid + addcmul {us(t['refine unfused'])} | "
          f"ratio {t['refine unfused'][0] / t['refine'][0]:.2f} (max |difference| {d1:.2e})")
    print(f"b = {b}: rr_linear_groupmax {us(t['groupmax'])} | rr_linear_ex + amax {us(t['groupmax unfused'])} | ratio "
          f"{t['groupmax unfused'][0] / t['groupmax'][0]:.2f} (max |difference| {d2:.2e})", flush=True)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--rounds", type=int, default=7)
    ap.add_argument("--iters", type=int, default=20)
    ap.add_argument("--conv-math", default="h2", choices=("h2", "f32"))
    ap.add_argument("--skip-model", action="store_true")
    a = ap.parse_args()
    dev = torch.device("cuda:0")
    g = torch.Generator(device=dev).manual_seed(0)
    with torch.no_grad():
        net = models.SpoCWrapper(8, backbone="resnet50", seed=3, device=dev, conv_math=a.conv_math)
        m = net.backbone
        for b in (64, 1):
            x4 = torch.relu(torch.randn((b, 7, 7, C), device=dev, generator=g))
            x4a = ops.amax_f32(x4, ops.amax_records(1, dev)[0]) if a.conv_math == "h2" else None
            u, ctx, pooled = head_launches(m, b, 7, 7, x4, x4a, a)
            compositions(m, b, u, ctx, pooled, a)
        if a.skip_model:
            return
        b, h, w = 64, 224, 224
        x = torch.randn((b, 3, h, w), device=dev, generator=g)
        xn = ops.nchw_to_nhwc(x, out_c=4)
        gem = models.GeMWrapper(8, backbone="resnet50", seed=3, device=dev, conv_math=a.conv_math)
        x4, x4a = m.trunk_map(xn)
        t = alternated({"spoc": lambda: net.forward_test(x), "gem": lambda: gem.forward_test(x),
                        "head": lambda: m.head(x4, x4a)}, a.rounds, max(1, a.iters // 4))
        print(f"B={b} {h}x{w} R50 {a.conv_math}: SpoCWrapper.forward_test {t['spoc'][0]:.3f} ms "
              f"({t['spoc'][1]:.3f} - {t['spoc'][2]:.3f}) | GeMWrapper.forward_test {t['gem'][0]:.3f} ms "
              f"({t['gem'][1]:.3f} - {t['gem'][2]:.3f}) | ratio {t['spoc'][0] / t['gem'][0]:.3f} | the head alone "
              f"{t['head'][0]:.3f} ms = {100 * t['head'][0] / t['spoc'][0]:.1f} %", flush=True)


if __name__ == "__main__":
    main()
