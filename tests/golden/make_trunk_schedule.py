"""Records tests/golden/trunk_schedule.json: what weights.resnet_conv_flops,
resnet_conv_bytes, resnet_conv_specs and senet_block_names return, as digests.

Run at the commit whose values are to be pinned (the fixture in git was written
by the last commit that still walked the trunk in each of the four functions):

    python tests/golden/make_trunk_schedule.py

Per case: the entry count, the sum of the values and a sha256 over the
``name=value`` lines in dict (or list) order, so that a changed value, a
changed key and a changed key order all show.  tests/test_trunk_schedule.py
recomputes the same digests (cases() and digest() below) and compares."""
import hashlib
import itertools
import json
import os
import sys

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, os.path.dirname(os.path.dirname(HERE)))
from research_image_retrieval_amd import weights as W  # noqa: E402

PATH = os.path.join(HERE, "trunk_schedule.json")
ARCHS = ("resnet50", "resnet101", "resnet152")
SIZES = ((224, 224), (100, 132), (33, 47))


def digest(lines, total):
    lines = list(lines)
    return {"n": len(lines), "sum": int(total), "sha256": hashlib.sha256("\n".join(lines).encode()).hexdigest()}


def _of_dict(d):
    return digest((f"{k}={v}" for k, v in d.items()), sum(d.values()))


def cases():
    """{case id: digest}: 18 flops cases and 144 bytes cases (162), the specs
    of every arch and the SE block names of every SENet."""
    out = {}
    for arch, so, (h, w) in itertools.product(ARCHS, W.STRIDE_ON, SIZES):
        out[f"flops/{arch}/{so}/{h}x{w}"] = _of_dict(W.resnet_conv_flops(arch, h, w, so))
    for arch, so, (h, w), b, wb, fused in itertools.product(ARCHS, W.STRIDE_ON, SIZES, (1, 3), (4, 6), (False, True)):
        out[f"bytes/{arch}/{so}/{h}x{w}/b{b}/w{wb}/{'fused' if fused else 'plain'}"] = _of_dict(
            W.resnet_conv_bytes(arch, h, w, b, so, wb, fused))
    for arch in ARCHS:
        specs = W.resnet_conv_specs(arch)
        out[f"specs/{arch}"] = digest((f"{c}={bn},{co},{ci},{k}" for c, bn, co, ci, k in specs),
                                      sum(co * ci * k * k for _, _, co, ci, k in specs))
    for arch in W.SENET_TRUNKS:
        names = W.senet_block_names(arch)
        out[f"senet/{arch}"] = digest((f"{p}={c}" for p, c in names), sum(c for _, c in names))
    return out


if __name__ == "__main__":
    got = cases()
    with open(PATH, "w") as f:
        json.dump(got, f, indent=0, sort_keys=True)
        f.write("\n")
    print(f"{len(got)} cases -> {PATH}")
