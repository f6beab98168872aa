"""Token on the device: Token.forward_test beside GeM.forward_test (same build,
same trunk seed, same input) at batch 64 x 224x224 and batch 1 x 768x1024, the
head's launches one by one, the head beside the float32 torch restatement of it
(tests/token_ref.py on the same device and x4: eager torch on rocBLAS, the
reference's own way of computing the head), and rr_attention_hd128 alone.

Legs are alternated in one process after a warm-up, and the medians over
--rounds are reported (Token head).

    python tools/token_bench.py [--rounds 7] [--iters 5] [--conv-math h2]
"""
import argparse
import os
import statistics
import sys

import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tests"))
import token_ref  # noqa: E402
from research_image_retrieval_amd import ops  # noqa: E402
from research_image_retrieval_amd import weights as W  # noqa: E402
from research_image_retrieval_amd.networks import GeM, Token  # noqa: E402

TRACED = ("conv2d_h2", "conv2d", "attention_hd128", "amax_f32", "token_pool", "linear_ex", "layernorm", "gelu")


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


def trace_head(tr, x4, x4a):
    """One head call with every ops launch recorded: [(label, replay)]."""
    calls, saved = [], {n: getattr(ops, n) for n in TRACED}

    def wrap(name, fn):
        def rec(*a, **k):
            shape = next((tuple(t.shape) for t in a if isinstance(t, torch.Tensor)), ())
            calls.append((f"{len(calls):02d} {name} {shape}", lambda: fn(*a, **k)))
            return fn(*a, **k)
        return rec

    try:
        for n, fn in saved.items():
            setattr(ops, n, wrap(n, fn))
        tr(x4, x4a)
    finally:
        for n, fn in saved.items():
            setattr(ops, n, fn)
    return calls


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--rounds", type=int, default=7)
    ap.add_argument("--iters", type=int, default=5)
    ap.add_argument("--conv-math", default="h2", choices=("h2", "f32"))
    a = ap.parse_args()
    dev = torch.device("cuda:0")
    g = torch.Generator(device=dev).manual_seed(0)
    tok = Token(seed=3, device=dev, conv_math=a.conv_math)
    gem = GeM(seed=3, device=dev, conv_math=a.conv_math)
    head_t = {k: v.to(dev) for k, v in W.token_head_from_state_dict(W.synthetic_token_head(4)).items()}
    for b, h, w in ((64, 224, 224), (1, 768, 1024)):
        x = torch.randn((b, 3, h, w), device=dev, generator=g)
        xn = ops.nchw_to_nhwc(x, out_c=4)
        _, x4, _, x4a = tok.backbone.maps(xn)
        n = x4.shape[1] * x4.shape[2]
        x4_nchw = x4.permute(0, 3, 1, 2).contiguous()
        net = alternated({"token": lambda: tok.forward_test(x), "gem": lambda: gem.forward_test(x)}, a.rounds, a.iters)
        with torch.no_grad():
            head = alternated({"librr head": lambda: tok.tr(x4, x4a),
                               "torch float32 head": lambda: token_ref.refine(x4_nchw, head_t, torch.float32)},
                              a.rounds, 4 * a.iters)
        calls = trace_head(tok.tr, x4, x4a)
        each = alternated(dict(calls), a.rounds, 10 * a.iters)
        print(f"B={b} {h}x{w} ({n} positions) {a.conv_math}: Token.forward_test {net['token']:.3f} ms | "
              f"GeM.forward_test {net['gem']:.3f} ms | ratio {net['token'] / net['gem']:.3f}", flush=True)
        print(f"   head: librr {head['librr head']:.3f} ms | float32 torch restatement {head['torch float32 head']:.3f} ms "
              f"| {len(calls)} launches, sum of the launches alone {sum(each.values()):.3f} ms", flush=True)
        for k, v in each.items():
            print(f"      {k}: {v * 1e3:.1f} us", flush=True)
        del x, xn, x4, x4_nchw, calls, each
    for b, nq, nk in ((64, 49, 49), (1, 768, 768), (64, 4, 49)):
        q = torch.randn((b * nq, 1024), device=dev, generator=g)
        kv = torch.randn((b * nk, 2048), device=dev, generator=g)
        t = alternated({"a": lambda: ops.attention_hd128(q, kv[:, :1024], kv[:, 1024:], b, nq, nk, 8)}, a.rounds,
                       20 * a.iters)["a"]
        flop = 4.0 * b * 8 * nq * nk * 128
        wgs = b * 8 * (1 if nq <= 16 else (nq + 63) // 64)
        print(f"rr_attention_hd128 ({b},{nq},{nk},8): {t * 1e3:.1f} us, {flop / t / 1e9:.3f} TFLOP/s of "
              f"{flop / 1e9:.3f} GFLOP, {wgs} workgroups", flush=True)


if __name__ == "__main__":
    main()
