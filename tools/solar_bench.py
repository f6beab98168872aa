"""SOLAR on the device: SOLAR.forward_test beside GeM.forward_test (same build,
same trunk weights, same input), the head's launches one by one, and
rr_soa_attention alone, at batch 64 x 224x224 and batch 1 x 768x1024.

Legs are alternated in one process after a warm-up, and the medians over
--rounds are reported (SOLAR head).

    python tools/solar_bench.py [--rounds 7] [--iters 5] [--conv-math h2]
"""
import argparse
import os
import statistics
import sys

import torch

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
from research_image_retrieval_amd import ops  # noqa: E402
from research_image_retrieval_amd.networks import SOLAR, GeM  # noqa: E402


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
    a = ap.parse_args()
    dev = torch.device("cuda:0")
    g = torch.Generator(device=dev).manual_seed(0)
    solar = SOLAR(seed=3, device=dev, conv_math=a.conv_math)
    gem = GeM(seed=3, device=dev, conv_math=a.conv_math)
    blk = solar.pooling
    c = blk.mid_ch
    for b, h, w in ((64, 224, 224), (1, 768, 1024)):
        x = torch.randn((b, 3, h, w), device=dev, generator=g)
        xn = ops.nchw_to_nhwc(x, out_c=4)
        _, x4, _, x4a = solar.backbone.maps(xn)
        fgh_leg = lambda: blk.fgh(x4, x4a, blk.fgh_b)  # noqa: E731
        fgh = fgh_leg()
        att = ops.soa_attention(fgh, c)
        hw = x4.shape[1] * x4.shape[2]
        att_a = ops.amax_of(att) if a.conv_math == "h2" else None
        v_leg = lambda: blk.v(att, att_a, blk.v_b, residual=x4)  # noqa: E731
        net = alternated({"solar": lambda: solar.forward_test(x), "gem": lambda: gem.forward_test(x)}, a.rounds,
                         a.iters)
        head = alternated({"fgh conv": fgh_leg, "soa_attention": lambda: ops.soa_attention(fgh, c), "v conv": v_leg,
                           "whole block": lambda: blk(x4, x4a), "gem_pool alone": lambda: ops.gem_pool(x4, 3.0, 1e-6)},
                          a.rounds, 20 * a.iters)
        flop = 4.0 * b * hw * hw * c
        print(f"B={b} {h}x{w} ({hw} positions) {a.conv_math}: SOLAR.forward_test {net['solar']:.3f} ms | "
              f"GeM.forward_test {net['gem']:.3f} ms | ratio {net['solar'] / net['gem']:.3f}", flush=True)
        print("   head launches (median ms): " + " | ".join(f"{k} {v:.4f}" for k, v in head.items()), flush=True)
        print(f"   rr_soa_attention [{b},{hw},{c}]: {head['soa_attention'] * 1e3:.1f} us, "
              f"{flop / head['soa_attention'] / 1e9:.2f} TFLOP/s of {flop / 1e9:.2f} GFLOP, "
              f"{b * ((hw + 15) // 16)} workgroups", flush=True)
        del x, xn, x4, fgh, att


if __name__ == "__main__":
    main()
