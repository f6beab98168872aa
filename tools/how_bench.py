"""HOW on the device: rr_how_vlad (+ the rr_l2_normalize launch that follows it)
and rr_how_asmk beside eager float32 torch on the same device and rows, at
(b, n) = (64, 49), (1, 1024) and (1280, 49) with d = 128, k = 64; final_proj
(rr_linear at K = 8192 and K = 64) by itself; and HOWVLADWrapper.forward_test /
HOWASMKWrapper.forward_test beside GeMWrapper.forward_test at 64 x 224x224 with
the head's share.

Two eager forms of VLAD are timed: the reference's own (models/how_vlad.py:30-58:
cdist, softmax, then a Python loop over the centroids, three launches each) and
tests/how_ref.py's (the loop written as two products).  ASMK's eager form is
how_ref's (argmin, gather, threshold, scatter_add): the reference's double
Python loop over batch x positions reads a device flag per position and is not
timed.  Both eager forms start from the RAW rows, as the kernels do.

Legs are alternated in one process after a warm-up, and the medians over
--rounds are reported (DESIGN.md § HOW head).

    python tools/how_bench.py [--rounds 7] [--iters 5] [--conv-math h2]
"""
import argparse
import os
import statistics
import sys

import torch
import torch.nn.functional as F

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tests"))
import how_ref  # noqa: E402
from research_image_retrieval_amd import models, ops  # noqa: E402


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


def eager_vlad_loop(x, cent, alpha=100.0):
    """The reference's sequence on raw rows: :162, then :36-56 with its loop."""
    x = F.normalize(x, p=2, dim=2)
    b, n, d = x.shape
    k = cent.shape[0]
    dist = torch.cdist(x, cent.unsqueeze(0).expand(b, -1, -1))
    a = F.softmax(-alpha * dist, dim=2)
    vlad = torch.zeros(b, k, d, device=x.device)
    for c in range(k):
        res = x - cent[c].unsqueeze(0).unsqueeze(0)
        vlad[:, c, :] = (a[:, :, c].unsqueeze(2) * res).sum(dim=1)
    return F.normalize(vlad.view(b, -1), p=2, dim=1)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--rounds", type=int, default=7)
    ap.add_argument("--iters", type=int, default=5)
    ap.add_argument("--conv-math", default="h2", choices=("h2", "f32"))
    a = ap.parse_args()
    dev = torch.device("cuda:0")
    g = torch.Generator(device=dev).manual_seed(0)
    d, k = 128, 64
    cent = F.normalize(torch.randn((k, d), device=dev, generator=g), dim=1)
    wts = 0.5 + torch.rand((k,), device=dev, generator=g)
    with torch.no_grad():
        for b, n in ((64, 49), (1, 1024), (1280, 49)):
            x = torch.randn((b, n, d), device=dev, generator=g)

            def vlad_l2():
                v = ops.how_vlad(x, cent)
                return ops.l2_normalize(v, 1e-12, out=v)

            t = alternated({"rr_how_vlad": lambda: ops.how_vlad(x, cent), "rr_how_vlad + l2": vlad_l2,
                            "eager loop": lambda: eager_vlad_loop(x, cent),
                            "eager two products": lambda: F.normalize(how_ref.vlad(x, cent, dtype=torch.float32)["vlad"],
                                                                      dim=1),
                            "rr_how_asmk": lambda: ops.l2_normalize(ops.how_asmk(x, cent, wts), 1e-12),
                            "eager asmk": lambda: how_ref_asmk_device(x, cent, wts)}, a.rounds, 4 * a.iters)
            print(f"(b, n) = ({b}, {n}), d {d}, k {k}: rr_how_vlad {t['rr_how_vlad'] * 1e3:.1f} us, with the L2 launch "
                  f"{t['rr_how_vlad + l2'] * 1e3:.1f} us | eager float32: the reference's loop "
                  f"{t['eager loop'] * 1e3:.1f} us, two products {t['eager two products'] * 1e3:.1f} us || rr_how_asmk with "
                  f"its L2 launch {t['rr_how_asmk'] * 1e3:.1f} us | eager float32 {t['eager asmk'] * 1e3:.1f} us", flush=True)
            del x
        for name, kk in (("VLAD", k * d), ("ASMK", k)):
            w = torch.randn((2048, kk), device=dev, generator=g)
            bias = torch.randn((2048,), device=dev, generator=g)
            for m in (1, 64, 1280):
                v = torch.randn((m, kk), device=dev, generator=g)
                t = alternated({"lin": lambda: ops.linear(v, w, bias)}, a.rounds, 4 * a.iters)["lin"]
                print(f"final_proj ({name}) rr_linear M {m}, K {kk}, N 2048: {t * 1e3:.1f} us "
                      f"({w.numel() * 4 / t / 1e6:.0f} GB/s of the weight)", flush=True)
        b, h, w = 64, 224, 224
        x = torch.randn((b, 3, h, w), device=dev, generator=g)
        xn = ops.nchw_to_nhwc(x, out_c=4)
        gem = models.GeMWrapper(8, backbone="resnet50", seed=3, device=dev, conv_math=a.conv_math)
        for cls in (models.HOWVLADWrapper, models.HOWASMKWrapper):
            net = cls(8, backbone="resnet50", seed=3, device=dev, conv_math=a.conv_math)
            m = net.backbone
            x4, x4a = m.trunk_map(xn)
            t = alternated({"how": lambda: net.forward_test(x), "gem": lambda: gem.forward_test(x),
                            "head": lambda: m.head(x4, x4a)}, a.rounds, a.iters)
            print(f"B={b} {h}x{w} R50 {a.conv_math}: {cls.__name__}.forward_test {t['how']:.3f} ms | "
                  f"GeMWrapper.forward_test {t['gem']:.3f} ms | ratio {t['how'] / t['gem']:.3f} | the head alone "
                  f"(local_proj, pooling, L2, final_proj) {t['head']:.3f} ms = {100 * t['head'] / t['how']:.1f} %",
                  flush=True)
            del net, m, x4


def how_ref_asmk_device(x, cent, wts):
    """tests/how_ref.asmk's steps with the histogram on x's device."""
    desc = F.normalize(x, p=2, dim=2)
    b, kk = x.shape[0], cent.shape[0]
    dist = torch.cdist(desc, cent.unsqueeze(0).expand(b, -1, -1))
    nearest = torch.argmin(dist, dim=2)
    mind = torch.gather(dist, 2, nearest.unsqueeze(2)).squeeze(2)
    thr = mind.mean(dim=1, keepdim=True) + mind.std(dim=1, keepdim=True)
    count = torch.zeros(b, kk, device=x.device).scatter_add_(1, nearest, (mind < thr).float())
    return F.normalize(wts.unsqueeze(0) * count, p=2, dim=1)


if __name__ == "__main__":
    main()
