"""SoSNet on the device: rr_sos_cov at (b, n, c) = (64, 49, 512), (1, 1024, 512)
and (1280, 49, 512) with its bytes (z read once, out written) and the share of
the HBM rate they reach; rr_linear_splitk against rr_linear in the same process
at (m, k, n) = (1 | 64 | 1280, 8192 | 131328, 2048) with the achieved weight
bandwidth (k n 4 B / time); and SoSNetWrapper.forward_test beside
GeMWrapper.forward_test at 64 x 224x224 R50 with the head's share.

Device events around --iters calls; legs are alternated in one process after a
warm-up, and the medians over --rounds are reported (DESIGN.md § SoSNet head).
HBM: 8.0 TB/s spec, 6.29 TB/s measured for a float4 copy; shares are of the
measured figure.

    python tools/sos_bench.py [--rounds 7] [--iters 5] [--conv-math h2] [--skip-model]
"""
import argparse
import os
import statistics
import sys

import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
from research_image_retrieval_amd import models, ops  # noqa: E402

HBM_COPY = 6.29e12  # B/s, measured float4 copy


def t_ms(fn, iters):
    s, e = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    s.record()
    for _ in range(iters):
        fn()
    e.record()
    torch.cuda.synchronize()
    return s.elapsed_time(e) / iters


def alternated(legs, rounds, iters, warm=2):
    """legs: name -> callable.  Median ms per call of each leg over `rounds`
    rounds that run every leg once, in turn."""
    for fn in legs.values():
        for _ in range(warm):
            fn()
    torch.cuda.synchronize()
    ts = {k: [] for k in legs}
    for _ in range(rounds):
        for k, fn in legs.items():
            ts[k].append(t_ms(fn, iters))
    return {k: statistics.median(v) for k, v in ts.items()}


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--rounds", type=int, default=7)
    ap.add_argument("--iters", type=int, default=5)
    ap.add_argument("--conv-math", default="h2", choices=("h2", "f32"))
    ap.add_argument("--skip-model", action="store_true")
    a = ap.parse_args()
    dev = torch.device("cuda:0")
    g = torch.Generator(device=dev).manual_seed(0)
    with torch.no_grad():
        c, dh = 512, 256
        w3 = torch.randn((dh,), device=dev, generator=g) * 0.2
        for b, n in ((64, 49), (1, 1024), (1280, 49)):
            z = torch.randn((b, n, c), device=dev, generator=g)
            hid = torch.relu(torch.randn((b, n, dh), device=dev, generator=g))
            t = alternated({"cov": lambda: ops.sos_cov(z, hid, w3, 0.1)}, a.rounds, 4 * a.iters)["cov"]
            by = (z.numel() + hid.numel() + b * c * (c + 1) // 2) * 4
            print(f"rr_sos_cov (b, n, c) = ({b}, {n}, {c}), dh {dh}: {t * 1e3:.1f} us; z + hid read once and out "
                  f"written = {by / 1e6:.1f} MB -> {by / t / 1e6:.0f} GB/s = {100 * by / (t * 1e-3) / HBM_COPY:.1f} % "
                  f"of the 6.29 TB/s copy rate", flush=True)
            del z, hid
        for k in (8192, 131328):
            w = torch.randn((2048, k), device=dev, generator=g)
            bias = torch.randn((2048,), device=dev, generator=g)
            for m in (1, 64, 1280):
                x = torch.randn((m, k), device=dev, generator=g)
                t = alternated({"splitk": lambda: ops.linear_splitk(x, w, bias), "linear": lambda: ops.linear(x, w, bias)},
                               a.rounds, a.iters if k > 8192 else 4 * a.iters)
                wb = w.numel() * 4
                print(f"M {m}, K {k}, N 2048: rr_linear_splitk {t['splitk'] * 1e3:.1f} us "
                      f"({wb / t['splitk'] / 1e6:.0f} GB/s of the weight, "
                      f"{100 * wb / (t['splitk'] * 1e-3) / HBM_COPY:.1f} % of the copy rate) | rr_linear "
                      f"{t['linear'] * 1e3:.1f} us ({wb / t['linear'] / 1e6:.0f} GB/s) | ratio "
                      f"{t['linear'] / t['splitk']:.2f}; {2.0 * m * k * 2048 / t['splitk'] / 1e9:.1f} TFLOP/s on the rows, "
                      f"{2.0 * max(m, 128) * k * 2048 / t['splitk'] / 1e9:.1f} on the core's 128-row tiles", flush=True)
                del x
            del w
        if a.skip_model:
            return
        b, h, w = 64, 224, 224
        x = torch.randn((b, 3, h, w), device=dev, generator=g)
        xn = ops.nchw_to_nhwc(x, out_c=4)
        gem = models.GeMWrapper(8, backbone="resnet50", seed=3, device=dev, conv_math=a.conv_math)
        net = models.SoSNetWrapper(8, backbone="resnet50", seed=3, device=dev, conv_math=a.conv_math)
        m = net.backbone
        x4, x4a = m.trunk_map(xn)
        t = alternated({"sos": lambda: net.forward_test(x), "gem": lambda: gem.forward_test(x),
                        "head": lambda: m.head(x4, x4a)}, a.rounds, a.iters)
        print(f"B={b} {h}x{w} R50 {a.conv_math}: SoSNetWrapper.forward_test {t['sos']:.3f} ms | "
              f"GeMWrapper.forward_test {t['gem']:.3f} ms | ratio {t['sos'] / t['gem']:.3f} | the head alone "
              f"(attention MLP, projection, rr_sos_cov, feature_proj) {t['head']:.3f} ms = "
              f"{100 * t['head'] / t['sos']:.1f} %", flush=True)
        z = m.proj(x4, x4a, None).view(b, 49, -1)
        h1 = m.att1(x4, x4a, m.w["att_b1"], relu=True)
        hid = ops.linear_ex(h1.view(b * 49, -1), m.w["att_w2"], m.w["att_b2"], act=1).view(b, 49, -1)
        v, inv = ops.sos_cov(z, hid, m.w["att_w3"], m.att_b3)
        hd = ops.linear_splitk(v, m.w["fp0_w"], m.w["fp0_b"], row_scale=inv, act=1)
        t = alternated({"att conv": lambda: m.att1(x4, x4a, m.w["att_b1"], relu=True),
                        "proj conv": lambda: m.proj(x4, x4a, None),
                        "linear_ex 512->256": lambda: ops.linear_ex(h1.view(b * 49, -1), m.w["att_w2"], m.w["att_b2"],
                                                                    act=1),
                        "sos_cov": lambda: ops.sos_cov(z, hid, m.w["att_w3"], m.att_b3),
                        "linear_splitk": lambda: ops.linear_splitk(v, m.w["fp0_w"], m.w["fp0_b"], row_scale=inv, act=1),
                        "linear 2048": lambda: ops.linear(hd, m.w["fp3_w"], m.w["fp3_b"])}, a.rounds, a.iters)
        print("   the head's launches: " + ", ".join(f"{k} {v * 1e3:.1f} us" for k, v in t.items()), flush=True)


if __name__ == "__main__":
    main()
