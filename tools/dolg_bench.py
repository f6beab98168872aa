"""DOLG head on the device: rr_dolg_local_pool's achieved read rate beside
rr_gem_pool's on a map of the same byte count (algorithmic bytes b*hw*c*4,
alternated in one process), and the whole head's time beside the R101 trunk's.

    python tools/dolg_bench.py [--batch 1280] [--size 224] [--rounds 3] [--skip-net]
"""
import argparse
import os
import sys

import torch

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
from research_image_retrieval_amd import ops  # noqa: E402
from research_image_retrieval_amd.networks import DOLG  # noqa: E402


def t_ms(fn, iters, warm=3):
    for _ in range(warm):
        fn()
    torch.cuda.synchronize()
    s, e = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    s.record()
    for _ in range(iters):
        fn()
    e.record()
    torch.cuda.synchronize()
    return s.elapsed_time(e) / iters


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--batch", type=int, default=1280)
    ap.add_argument("--size", type=int, default=224)
    ap.add_argument("--rounds", type=int, default=3)
    ap.add_argument("--skip-net", action="store_true")
    a = ap.parse_args()
    dev = torch.device("cuda:0")
    hw = (a.size // 16) ** 2
    g = torch.Generator(device=dev).manual_seed(0)
    w2 = torch.randn(1024, device=dev, generator=g) * 0.05
    for b, n, c in ((a.batch, hw, 1024), (1, 4096, 1024)):
        y = torch.randn((b, n, c), device=dev, generator=g)
        by = b * n * c * 4
        iters = min(5000, max(20, int(9e11 / by)))  # ~0.3 s windows at 3 TB/s
        for r in range(a.rounds):
            tp = t_ms(lambda: ops.dolg_local_pool(y, w2, 0.1), iters)
            tg = t_ms(lambda: ops.gem_pool(y, 3.0, 1e-6), iters)
            print(f"[{b},{n},{c}] round {r}: dolg_local_pool {tp:.4f} ms {by / tp / 1e6:.0f} GB/s | "
                  f"gem_pool {tg:.4f} ms {by / tg / 1e6:.0f} GB/s  ({iters} launches each)", flush=True)
        del y
    if a.skip_net:
        return
    net = DOLG(seed=3, device=dev, conv_math="h2")
    x = torch.randn((a.batch, a.size, a.size, 4), device=dev, generator=g)
    x[..., 3] = 0
    trunk = lambda: net.globalmodel.maps(x, want_x3=True)  # noqa: E731
    x3, x4, x3a, _ = trunk()
    for r in range(a.rounds):
        tt = t_ms(trunk, 5, warm=1)
        th = t_ms(lambda: net.head(x3, x4, x3a), 20, warm=1)
        tw = t_ms(lambda: net.forward_test_nhwc(x), 5, warm=1)
        print(f"B={a.batch} {a.size}x{a.size} h2 round {r}: R101 trunk {tt:.2f} ms | DOLG head {th:.3f} ms "
              f"({100 * th / tt:.1f} % of the trunk) | whole forward_test {tw:.2f} ms", flush=True)
    ops_t = ops.KernelTimer(0)
    ops_t.enable(True)
    net.head(x3, x4, x3a)
    torch.cuda.synchronize()
    from research_image_retrieval_amd import _lib
    for name, cls in (("gemm (conv1, fc_t, fc)", _lib.TIME_GEMM), ("elementwise (pool, gem, fuse, l2)", _lib.TIME_ELEM)):
        print(f"head, one call, class {name}: {ops_t.collect(cls)}")
    ops_t.enable(False)


if __name__ == "__main__":
    main()
