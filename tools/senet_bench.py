"""The SE-ResNet trunk on the device: SENet("senet50").maps beside
ResNet("resnet50").maps at 224 x 224 for batch 1 and 64; the launches an SE
block adds, by rr_timing class; rr_se_squeeze and rr_se_apply at every stage's
shape with their bytes and the share of the measured copy rate they reach; and
the byte model's expectation next to the measured overhead (DESIGN.md § Numbers
(SE-ResNet trunk)).

Byte model.  With N = b hw c elements of a block's output, a plain bottleneck's
conv3 reads the identity and writes the output in its epilogue.  An SE block's
conv3 writes its raw output (4 N), the squeeze reads it (4 N), the apply reads
it again (4 N), reads the identity and writes the output: 12 N bytes more.  A
stage's first block also writes and re-reads the projected identity the fused
conv3 + downsample GEMM never stored: 8 N more.

Device events around --iters calls; legs are alternated in one process after a
warm-up, and the median (min - max) over --rounds is reported.

    python tools/senet_bench.py [--rounds 7] [--iters 10] [--conv-math h2]
"""
import argparse
import os
import sys

import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tools"))
from research_image_retrieval_amd import networks, ops  # noqa: E402
from spoc_bench import HBM_COPY, alternated, us  # noqa: E402

STAGES = ((56 * 56, 256, 3), (28 * 28, 512, 4), (14 * 14, 1024, 6), (7 * 7, 2048, 3))  # (hw, c, blocks) of senet50
CLASSES = {1: "GEMM", 3: "elementwise"}


def extra_bytes(b):
    """(the SE launches' extra bytes, the unfused stage entries' extra bytes) per forward."""
    return (sum(12.0 * b * hw * c * nb for hw, c, nb in STAGES), sum(8.0 * b * hw * c for hw, c, _ in STAGES))


def class_times(net, x, iters):
    """ms per forward of each rr_timing class over `iters` forwards."""
    kt = ops.KernelTimer(0)
    net.maps(x)
    torch.cuda.synchronize()
    kt.enable(True)
    for _ in range(iters):
        net.maps(x)
    torch.cuda.synchronize()
    got = {c: kt.collect_ex(c) for c in CLASSES}
    kt.enable(False)
    return {c: (tot / iters, n // iters) for c, (_uni, tot, n) in got.items()}


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--rounds", type=int, default=7)
    ap.add_argument("--iters", type=int, default=10)
    ap.add_argument("--conv-math", default="h2", choices=("h2", "f32"))
    a = ap.parse_args()
    dev = torch.device("cuda:0")
    g = torch.Generator(device=dev).manual_seed(0)
    with torch.no_grad():
        se = networks.SENet("senet50", seed=3, device=dev, conv_math=a.conv_math)
        rn = networks.ResNet("resnet50", seed=3, device=dev, conv_math=a.conv_math)
        for b in (64, 1):
            x = ops.nchw_to_nhwc(torch.randn((b, 3, 224, 224), device=dev, generator=g), out_c=4)
            t = alternated({"senet50": lambda: se.maps(x), "resnet50": lambda: rn.maps(x)}, a.rounds, a.iters)
            over = t["senet50"][0] - t["resnet50"][0]
            eb_se, eb_entry = extra_bytes(b)
            model = (eb_se + eb_entry) / HBM_COPY * 1e3
            print(f"B={b} 224x224 {a.conv_math}: SENet(senet50).maps {t['senet50'][0]:.3f} ms ({t['senet50'][1]:.3f} - "
                  f"{t['senet50'][2]:.3f}) | ResNet(resnet50).maps {t['resnet50'][0]:.3f} ms ({t['resnet50'][1]:.3f} - "
                  f"{t['resnet50'][2]:.3f}) | ratio {t['senet50'][0] / t['resnet50'][0]:.3f} | overhead {over:.3f} ms; "
                  f"byte model {eb_se / 1e6:.1f} MB (SE) + {eb_entry / 1e6:.1f} MB (unfused entries) at the copy rate = "
                  f"{model:.3f} ms; measured / model {over / model:.2f}", flush=True)
            cs, cr = class_times(se, x, a.iters), class_times(rn, x, a.iters)
            for c, name in CLASSES.items():
                print(f"   rr_timing class {c} ({name}): senet50 {cs[c][0]:.3f} ms in {cs[c][1]} launches | resnet50 "
                      f"{cr[c][0]:.3f} ms in {cr[c][1]} launches | difference {cs[c][0] - cr[c][0]:.3f} ms", flush=True)
            tot_sq = tot_ap = tot_fc = 0.0
            for hw, c, nb in STAGES:
                cr_ = c // 16
                y = torch.randn((b, hw, c), device=dev, generator=g)
                idn = torch.relu(torch.randn((b, hw, c), device=dev, generator=g))
                w1 = torch.randn((cr_, c), device=dev, generator=g) / c ** 0.5
                w2 = torch.randn((c, cr_), device=dev, generator=g) / cr_ ** 0.5
                mean = ops.se_squeeze(y)
                hid = ops.linear_splitk(mean, w1, None, act=1)
                rec = ops.amax_records(1, dev)[0]
                # (in place on a clone, as the trunk runs it: values only shrink or stay; the record only grows)
                yc = y.clone()
                tt = alternated({"squeeze": lambda: ops.se_squeeze(y),
                                 "fc1": lambda: ops.linear_splitk(mean, w1, None, act=1),
                                 "apply": lambda: ops.se_apply(yc, hid, w2, idn, out=yc, out_amax=rec)},
                                a.rounds, a.iters)
                n = float(b) * hw * c
                sq_b, ap_b = 4.0 * n + 4.0 * b * c, 12.0 * n
                r_sq, r_ap = sq_b / (tt["squeeze"][0] * 1e-3), ap_b / (tt["apply"][0] * 1e-3)
                print(f"   ({b}, {hw}, {c}) x {nb} blocks: se_squeeze {us(tt['squeeze'])}, {sq_b / 1e6:.2f} MB -> "
                      f"{r_sq / 1e9:.0f} GB/s = {100 * r_sq / HBM_COPY:.1f} % of the copy rate | linear_splitk "
                      f"{us(tt['fc1'])} | se_apply {us(tt['apply'])}, {ap_b / 1e6:.2f} MB -> {r_ap / 1e9:.0f} GB/s = "
                      f"{100 * r_ap / HBM_COPY:.1f} % of the copy rate", flush=True)
                tot_sq += nb * tt["squeeze"][0]
                tot_fc += nb * tt["fc1"][0]
                tot_ap += nb * tt["apply"][0]
            print(f"   per forward, from the launches timed alone: squeeze {tot_sq:.3f} ms + linear_splitk {tot_fc:.3f} ms + "
                  f"apply {tot_ap:.3f} ms = {tot_sq + tot_fc + tot_ap:.3f} ms of the {over:.3f} ms overhead", flush=True)


if __name__ == "__main__":
    main()
