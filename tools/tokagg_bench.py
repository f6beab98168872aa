"""The token aggregator on the device: rr_cls_attn_pool at (b, seq, d, heads) =
(64, 50, 512, 8), (64, 197, 512, 8) and (1, 197, 512, 8) with its bytes (x and
qt read once, out written) and the share of the HBM copy rate they reach; the
folded last encoder layer (TokenModel._folded_last_layer: rr_linear,
rr_cls_attn_pool, rr_linear_splitk_ex, rr_layernorm, the FFN on B rows) against the
same layer over all rows (TokenModel.head(fold_last=False)'s path: QKV
rr_linear_ex, rr_attention, out-proj, LayerNorm, FFN on B seq rows, row 0
gathered), in the same process at those sizes; and TokenWrapper.forward_test
beside GeMWrapper.forward_test at 64 x 224x224 R50 with the head's share.

Device events around --iters calls; legs are alternated in one process after a
warm-up, and the medians over --rounds are reported (DESIGN.md § The token
aggregator).  HBM: 8.0 TB/s spec, 6.29 TB/s measured for a float4 copy; shares
are of the measured figure.

    python tools/tokagg_bench.py [--rounds 7] [--iters 5] [--conv-math h2] [--skip-model]
"""
import argparse
import os
import sys

import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
from research_image_retrieval_amd import models, ops  # noqa: E402
from sos_bench import HBM_COPY, alternated  # noqa: E402

SIZES = ((64, 50), (64, 197), (1, 197))


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
        d, heads = 512, 8
        for b, seq in SIZES:
            x = torch.randn((b, seq, d), device=dev, generator=g)
            qt = torch.randn((b, heads, d), device=dev, generator=g) * (3.0 / d ** 0.5)
            t = alternated({"pool": lambda: ops.cls_attn_pool(x, qt)}, a.rounds, 8 * a.iters)["pool"]
            by = (x.numel() + 2 * qt.numel()) * 4
            print(f"rr_cls_attn_pool (b, seq, d, heads) = ({b}, {seq}, {d}, {heads}): {t * 1e3:.1f} us; x and qt read "
                  f"once and out written = {by / 1e6:.2f} MB -> {by / t / 1e6:.0f} GB/s = "
                  f"{100 * by / (t * 1e-3) / HBM_COPY:.2f} % of the 6.29 TB/s copy rate; "
                  f"{4.0 * b * heads * seq * d / t / 1e6:.1f} GFLOP/s", flush=True)
        net = models.TokenWrapper(8, backbone="resnet50", seed=3, device=dev, conv_math=a.conv_math)
        m = net.backbone
        last = m.num_layers - 1
        for b, seq in SIZES:
            x = torch.randn((b * seq, d), device=dev, generator=g)
            folded = lambda: m._folded_last_layer(x, b, seq, None)  # noqa: E731
            unfolded = lambda: m._full_layer(x, last, b, seq).view(b, seq, d)[:, 0].contiguous()  # noqa: E731
            diff = (folded() - unfolded()).abs().max().item()
            t = alternated({"folded": folded, "unfolded": unfolded}, a.rounds, a.iters)
            print(f"last layer at B {b}, {seq} rows: folded {t['folded'] * 1e3:.1f} us | over all rows "
                  f"{t['unfolded'] * 1e3:.1f} us | ratio {t['unfolded'] / t['folded']:.2f} | max|folded - unfolded| "
                  f"{diff:.2e}", flush=True)
            x3 = x.view(b, seq, d)
            x0 = x3[:, 0].contiguous()
            w = m.w
            qt = ops.linear(x0, w["fold_a"], w["fold_a0"]).view(b, heads, d)
            pooled = ops.cls_attn_pool(x3, qt)
            y = ops.linear_splitk(pooled.view(b, heads * d), w["fold_m"], w["fold_m0"], residual=x0)
            y1 = ops.layernorm(y, w[f"l{last}_n1_g"], w[f"l{last}_n1_b"], 1e-5)
            hid = ops.linear_ex(y1, w[f"l{last}_l1_w"], w[f"l{last}_l1_b"], act=1)
            t = alternated({"row-0 gather": lambda: x3[:, 0].contiguous(),
                            "linear A": lambda: ops.linear(x0, w["fold_a"], w["fold_a0"]),
                            "cls_attn_pool": lambda: ops.cls_attn_pool(x3, qt),
                            "linear_splitk_ex M": lambda: ops.linear_splitk(pooled.view(b, heads * d), w["fold_m"],
                                                                            w["fold_m0"], residual=x0),
                            "(linear_ex M)": lambda: ops.linear_ex(pooled.view(b, heads * d), w["fold_m"], w["fold_m0"],
                                                                   residual=x0),
                            "layernorm": lambda: ops.layernorm(y, w[f"l{last}_n1_g"], w[f"l{last}_n1_b"], 1e-5),
                            "linear_ex 512->2048": lambda: ops.linear_ex(y1, w[f"l{last}_l1_w"], w[f"l{last}_l1_b"],
                                                                         act=1),
                            "linear_splitk_ex 2048->512": lambda: ops.linear_splitk(hid, w[f"l{last}_l2_w"],
                                                                                    w[f"l{last}_l2_b"], residual=y1),
                            "(linear_ex 2048->512)": lambda: ops.linear_ex(hid, w[f"l{last}_l2_w"], w[f"l{last}_l2_b"],
                                                                           residual=y1)},
                           a.rounds, a.iters)
            print("   the folded layer's launches: " + ", ".join(f"{k} {v * 1e3:.1f} us" for k, v in t.items()),
                  flush=True)
        if a.skip_model:
            return
        b, h, wd = 64, 224, 224
        x = torch.randn((b, 3, h, wd), device=dev, generator=g)
        xn = ops.nchw_to_nhwc(x, out_c=4)
        gem = models.GeMWrapper(8, backbone="resnet50", seed=3, device=dev, conv_math=a.conv_math)
        x4, x4a = m.trunk_map(xn)
        t = alternated({"token": lambda: net.forward_test(x), "gem": lambda: gem.forward_test(x),
                        "head": lambda: m.head(x4, x4a), "head unfolded": lambda: m.head(x4, x4a, fold_last=False)},
                       a.rounds, a.iters)
        print(f"B={b} {h}x{wd} R50 {a.conv_math}: TokenWrapper.forward_test {t['token']:.3f} ms | "
              f"GeMWrapper.forward_test {t['gem']:.3f} ms | ratio {t['token'] / t['gem']:.3f} | the head alone "
              f"(input_proj, tokens, {m.num_layers - 1} full layer(s), the folded layer, output_proj, feature_proj) "
              f"{t['head']:.3f} ms = {100 * t['head'] / t['token']:.1f} % | the head with the last layer unfolded "
              f"{t['head unfolded']:.3f} ms", flush=True)


if __name__ == "__main__":
    main()
