"""The bottleneck trunk's block schedule (weights.trunk_blocks) and what is
derived from it, without a GPU: resnet_conv_specs, senet_block_names,
resnet_conv_flops and resnet_conv_bytes return what they returned while each
walked the trunk itself (tests/golden/trunk_schedule.json, written by
make_trunk_schedule.py at that commit: count, sum and a sha256 over the
name=value lines in order, 162 flops and bytes cases), and the schedule's own
invariants hold."""
import json
import os
import sys

import pytest

from research_image_retrieval_amd import weights as W

GOLD = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden")
sys.path.insert(0, GOLD)
import make_trunk_schedule as M  # noqa: E402


@pytest.fixture(scope="module")
def stored():
    with open(M.PATH) as f:
        return json.load(f)


def test_every_derived_value_is_the_recorded_one(stored):
    got = M.cases()
    assert sorted(got) == sorted(stored)
    assert sum(k.startswith(("flops/", "bytes/")) for k in got) == 162
    assert [k for k in got if got[k] != stored[k]] == []


@pytest.mark.parametrize("arch", M.ARCHS)
def test_bytes_name_the_launches_flops_names(arch):
    for so in W.STRIDE_ON:
        fl = W.resnet_conv_flops(arch, 100, 132, so)
        for fused in (False, True):
            by = W.resnet_conv_bytes(arch, 100, 132, 3, so, 4, fused)
            assert list(by) == list(fl)
            assert min(by.values()) > 0 and min(fl.values()) > 0


@pytest.mark.parametrize("stride_on", W.STRIDE_ON)
@pytest.mark.parametrize("arch,n", [("resnet50", 16), ("resnet101", 33), ("resnet152", 50)])
def test_schedule_invariants(arch, n, stride_on):
    blocks = W.trunk_blocks(arch, stride_on)
    assert isinstance(blocks, tuple) and len(blocks) == n
    layers = W.RESNET_LAYERS[arch]
    assert [(b.stage, b.index) for b in blocks] == [(li, bi) for li, nb in enumerate(layers) for bi in range(nb)]
    cout = 64  # the stem's
    for b in blocks:
        assert b.prefix == f"layer{b.stage + 1}.{b.index}"
        assert b.entry == (b.index == 0)  # one entry per stage, its first block
        assert b.stage_end == (b.index == layers[b.stage] - 1)
        assert b.stride == (2 if b.entry and b.stage > 0 else 1)
        assert (b.s1, b.s2) == W.block_strides(b.stride, stride_on) and b.s1 * b.s2 == b.stride
        assert b.inplanes == cout
        assert b.planes == 64 << b.stage and b.cout == 4 * b.planes
        cout = b.cout
    assert sum(b.entry for b in blocks) == sum(b.stage_end for b in blocks) == len(layers)
    assert W.trunk_blocks(arch, stride_on) is blocks  # computed once per (arch, stride_on)


def test_schedule_arguments_and_map_sizes():
    with pytest.raises(ValueError):
        W.trunk_blocks("resnet50", "5x5")
    with pytest.raises(KeyError):
        W.trunk_blocks("resnet18")
    assert W.trunk_blocks("resnet50") == W.trunk_blocks("resnet50", "3x3") != W.trunk_blocks("resnet50", "1x1")
    assert [W.conv_out(n, k, s, p) for n, k, s, p in ((224, 7, 2, 3), (112, 3, 2, 1), (7, 1, 2, 0), (9, 3, 1, 1))] == \
        [112, 56, 4, 9]
    for so in W.STRIDE_ON:
        h, w = W.conv_out(W.conv_out(33, 7, 2, 3), 3, 2, 1), W.conv_out(W.conv_out(47, 7, 2, 3), 3, 2, 1)
        for b, (H, Wd), (H1, W1), (Ho, Wo) in W.trunk_block_maps("resnet50", 33, 47, so):
            assert (H, Wd) == (h, w)  # a block reads what the one before it wrote
            assert (H1, W1) == (W.conv_out(H, 1, b.s1, 0), W.conv_out(Wd, 1, b.s1, 0))
            assert (Ho, Wo) == (W.conv_out(H1, 3, b.s2, 1), W.conv_out(W1, 3, b.s2, 1))
            h, w = Ho, Wo
        assert (h, w) == (2, 2)
