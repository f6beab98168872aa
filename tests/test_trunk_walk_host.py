"""The bottleneck trunks' walk (networks._BottleneckTrunk.maps, ResNet and
SENet) and the native plan's conv list (ResNet.plan_convs) without a GPU:
networks.ops is replaced by tests/golden/make_trunk_launches.py's Recorder,
and every ops call, its arguments and the hook calls are what the trunks issued
while each had a stage loop of its own (tests/golden/trunk_launches.json,
recorded by that script at that commit).  Independently of the fixture: every
f16x2 conv reads the record the launch that produced its input wrote, the
hooks fire once each and in order, and x3 is stage 3's last output."""
import json
import os
import sys

import pytest

GOLD = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden")
sys.path.insert(0, GOLD)
import make_trunk_launches as M  # noqa: E402

N_BLOCKS = 16  # resnet50 / senet50


@pytest.fixture(scope="module")
def got():
    return M.record_all()


@pytest.fixture(scope="module")
def stored():
    with open(M.PATH) as f:
        return json.load(f)


def test_the_cases_cover_what_they_should(got):
    w = set(got["walk"])
    for math in ("h2", "f32"):
        for tag in ("resnet50/%s/3x3", "resnet50/%s/1x1", "senet50/%s"):
            for shape in ("2x64x64x4", "1x33x47x4"):
                assert f"{tag % math}/{shape}/x3" in w
        assert f"resnet50/{math}/3x3/2x64x64x4/no_x3" in w
    assert "resnet50/h2/3x3/rgb/2x64x64x3/x3" in w
    for flags in ("fuse_downsample=0,fuse_stem_pool=1", "fuse_downsample=1,fuse_stem_pool=0",
                  "fuse_downsample=0,fuse_stem_pool=0"):
        assert f"resnet50/h2/3x3/{flags}/2x64x64x4/x3" in w
    assert len(got["plan"]) == 8  # four flag combinations x both stride_on


def test_every_launch_is_the_recorded_one(got, stored):
    assert sorted(got["walk"]) == sorted(stored["walk"])
    for case, log in stored["walk"].items():
        mine = json.loads(json.dumps(got["walk"][case]))
        for i, (a, b) in enumerate(zip(mine, log)):
            assert a == b, f"{case}: call {i}"
        assert len(mine) == len(log), case


def test_the_plans_conv_list_is_the_recorded_one(got, stored):
    assert sorted(got["plan"]) == sorted(stored["plan"])
    for case, plan in stored["plan"].items():
        assert got["plan"][case]["fuse_entry"] == plan["fuse_entry"], case
        for i, (a, b) in enumerate(zip(got["plan"][case]["convs"], plan["convs"])):
            assert a == b, f"{case}: conv {i}"
        assert len(got["plan"][case]["convs"]) == len(plan["convs"]) == 1 + 3 * N_BLOCKS + 4 - sum(plan["fuse_entry"])


def _name(t):
    return None if t is None else t.split("[")[0]


def _records(log):
    """The walk's invariants on one log -> (block outputs, hooks): every
    launch that reads a record reads the one its input's producer wrote."""
    wrote, outs, hooks = {}, [], []
    for row in log:
        op, a = row[0], [_name(v) if isinstance(v, str) else v for v in row[1:]]
        if op == "amax_f32":
            wrote[a[0]] = a[1]
        elif op in ("conv2d_h2", "stem_pool_h2"):
            out, x, xa = a[:3]
            assert wrote[x] == xa and xa is not None, row
            wrote[out] = a[-1]
            if op == "conv2d_h2" and a[7] is not None:  # the residual conv3 ends a ResNet block
                outs.append(out)
        elif op == "maxpool2d":
            wrote[a[0]] = wrote.get(a[1])  # the pooled map keeps the stem's record
        elif op == "bottleneck_out_h2":
            out, y, ya, x, xa = a[:5]
            assert wrote[y] == ya and wrote[x] == xa and None not in (ya, xa), row
            wrote[out] = a[-1]
            outs.append(out)
        elif op == "conv2d":
            if a[6] is not None:
                outs.append(a[0])
        elif op == "se_apply":
            assert a[0] == a[1] == a[7], row  # in place on conv3's output
            wrote[a[0]] = a[-1]
            outs.append(a[0])
        elif op == "hook":
            hooks.append(a[0])
    return outs, hooks, wrote


def test_records_hooks_and_x3_follow_the_walk(got):
    for case, log in got["walk"].items():
        log = json.loads(json.dumps(log))
        h2 = "/h2/" in case
        outs, hooks, wrote = _records(log)
        assert len(outs) == N_BLOCKS, case
        assert hooks == (list(range(1 + 3 * N_BLOCKS)) if h2 else []), case
        assert [r for r in log if r[0] == "amax_records"] == ([["amax_records", 2 + 3 * N_BLOCKS]] if h2 else []), case
        x3, x4, x3a, x4a = (_name(v) for v in log[-1][1:])
        assert log[-1][0] == "return" and x4 == outs[-1], case
        assert x4a == (wrote[x4] if h2 else None), case
        if case.endswith("/no_x3"):
            assert x3 is None and x3a is None, case
        else:
            assert x3 == outs[3 + 4 + 6 - 1], case  # stage 3's last block
            assert x3a == (wrote[x3] if h2 else None), case
        if h2:
            # hook(0) right after the stem (its pool, where that is a launch), then one after each counted conv
            ops_seen = [r[0] for r in log]
            first = ops_seen.index("hook")
            assert ops_seen[first - 1] == ("maxpool2d" if "fuse_stem_pool=0" in case else "stem_pool_h2"), case
            assert all(r[-1] is not None for r in log if r[0] == "bottleneck_out_h2"), case


def test_the_flags_are_read_per_call(got):
    w = got["walk"]
    fused = [r[0] for r in w["resnet50/h2/3x3/2x64x64x4/x3"]]
    plain = [r[0] for r in w["resnet50/h2/3x3/fuse_downsample=0,fuse_stem_pool=0/2x64x64x4/x3"]]
    assert fused.count("bottleneck_out_h2") == 4 and fused.count("stem_pool_h2") == 1 and "maxpool2d" not in fused
    assert "bottleneck_out_h2" not in plain and "stem_pool_h2" not in plain and plain.count("maxpool2d") == 1
    assert plain.count("conv2d_h2") == 1 + 3 * N_BLOCKS + 4
