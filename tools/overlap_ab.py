"""A/B of the C3 trunk's batch split across HIP streams (networks
forward_test_u8_streams, and the native trunk plan's two parts, ops.TrunkPlan)
against the one-stream batch: ms per 1280-image embed, and bit-identity of
the split schedules to the same parts run one after another.
Usage: python tools/overlap_ab.py [reps]"""
import os
import sys
import time

import numpy as np
import torch

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import bench  # noqa: E402
from research_image_retrieval_amd import ops  # noqa: E402

dev = torch.device("cuda:0")
reps = int(sys.argv[1]) if len(sys.argv) > 1 else 3
B = int(os.environ.get("OV_BATCH", "1280"))
net = bench.build_extractor("resnet101", dev)
rs = np.random.RandomState(1234)
imgs = torch.from_numpy(rs.randint(0, 256, size=(B, 224, 224, 3), dtype=np.uint8)).to(dev)
streams = [torch.cuda.Stream(dev) for _ in range(4)]


def timed(fn):
    fn()
    torch.cuda.synchronize()
    t = []
    for _ in range(reps):
        torch.cuda.synchronize()
        t0 = time.perf_counter()
        fn()
        torch.cuda.synchronize()
        t.append((time.perf_counter() - t0) * 1e3)
    return min(t), float(np.median(t))


def one_part(x):
    """forward_test_u8 with the plan held to one part (its pick at this batch is two)."""
    with ops.tuning(dev.index, trunk_parts=1):
        return net.forward_test_u8(x)


def serial(parts):
    cuts = [B * i // parts for i in range(parts + 1)]
    return torch.cat([one_part(imgs[cuts[i]:cuts[i + 1]]) for i in range(parts)])


print("one stream, whole batch  min %.2f med %.2f ms" % timed(lambda: one_part(imgs)), flush=True)
print("one stream, 2 parts      min %.2f med %.2f ms" % timed(lambda: serial(2)), flush=True)
ref2 = serial(2)
ref3 = serial(3)
full = one_part(imgs)

# the native plan: parts 1 against 2 in this process, part 1 `lag` convs behind
trunk = net._trunk()
for lag in (0, 1, 2, 3):
    def planned(parts, lag=lag):
        with ops.tuning(dev.index, trunk_parts=parts):
            x4, x4a = trunk.plan(lag).forward_u8(imgs)
            return net._tail(None, x4, None, x4a)
    m1, d1 = timed(lambda: planned(1))
    m2, d2 = timed(lambda: planned(2))
    same = torch.equal(planned(2).view(torch.int32), ref2.view(torch.int32))
    print(f"plan lag {lag}: 1 part min {m1:.2f} med {d1:.2f} ms, 2 parts min {m2:.2f} med {d2:.2f} ms  "
          f"bit-identical to serial parts: {same}", flush=True)
cases = [(2, l, 0) for l in (0, 1, 2, 3, 4, 6, 9)] + [(3, 1, 0), (3, 3, 0)]
for parts, lag, share in cases:
    f = lambda: net.forward_test_u8_streams(imgs, streams[:parts], lag=lag)  # noqa: E731
    mn, md = timed(f)
    out = f()
    ref = ref2 if parts == 2 else (ref3 if parts == 3 else serial(parts))
    same = torch.equal(out.view(torch.int32), ref.view(torch.int32))
    err = (out - full).abs().max().item()
    print(f"{parts} streams lag {lag:2d}  min {mn:.2f} med {md:.2f} ms  bit-identical to serial parts: {same}  "
          f"max |d - whole batch| {err:.2e}", flush=True)
