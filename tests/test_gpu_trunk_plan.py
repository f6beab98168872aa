"""The native trunk plan (rr_trunk_h2_*, ops.TrunkPlan): one part is the
launch-by-launch trunk bit for bit, two parts are the one-part plan on each
slice (both also with the stage entries and the stem's pool unfused: the
plan's separate downsample conv and its max-pool op), the join orders the caller's stream behind both parts, the library's
pick stays at one part for small batches, and the class timer returns the
union of the launch intervals."""
import contextlib
import ctypes

import numpy as np
import pytest
import torch

from research_image_retrieval_amd import _lib, ops
from research_image_retrieval_amd.networks import ResNet

pytestmark = pytest.mark.gpu

DEV = "cuda:0"
SIZES = [(64, 64), (96, 80)]  # stage-4 maps 2x2 and 3x3 (the issue's shapes)
N_CONV = 1 + 3 * 16           # resnet50, stem + pool fused, stage entries fused: conv-class launches per part


@pytest.fixture(scope="module")
def nets():
    return {s: ResNet("resnet50", seed=5, device=DEV, stride_on=s) for s in ("3x3", "1x1")}


def _imgs(b, h, w, seed=0):
    rs = np.random.RandomState(seed)
    return torch.from_numpy(rs.randint(0, 256, size=(b, h, w, 3), dtype=np.uint8)).to(DEV)


def _bits(t):
    return t.view(torch.int32)


def _same(a, b):
    return a.shape == b.shape and torch.equal(_bits(a), _bits(b))


# (fuse_downsample, fuse_stem_pool): the plan's ENTRY / STEM_POOL ops, and its
# separate downsample conv into the identity buffer / its MAXPOOL op
FUSIONS = [(True, True), (False, True), (True, False), (False, False)]


@contextlib.contextmanager
def _fusions(net, fuse_downsample, fuse_stem_pool):
    """net with both flags set for the block (the eager trunk reads them per
    call, net.plan() keeps one plan per combination)."""
    saved = net.fuse_downsample, net.fuse_stem_pool
    net.fuse_downsample, net.fuse_stem_pool = fuse_downsample, fuse_stem_pool
    try:
        yield net
    finally:
        net.fuse_downsample, net.fuse_stem_pool = saved


def _one_part_is_the_reference_trunk(net, hw):
    img = _imgs(3, *hw, seed=1)
    ref = net.forward(ops.preprocess_u8(img, out_c=4), return_x3=True, return_x3_amax=True, return_amax=True)
    with ops.tuning(0, trunk_parts=1):
        got = net.plan().forward_u8(img, return_x3=True)
    torch.cuda.synchronize()
    for name, r, g in zip(("x3", "x4"), ref[:2], got[:2]):
        assert _same(r, g), name
    assert torch.equal(ref[2], got[2]), "x3 record"
    assert torch.equal(ref[3], got[3]), "x4 record"
    x4, x4a = net.plan().forward_u8(img)  # without x3: the same x4 and record
    assert _same(ref[1], x4) and torch.equal(ref[3], x4a)


@pytest.mark.parametrize("hw", SIZES)
@pytest.mark.parametrize("stride_on", ["3x3", "1x1"])
def test_one_part_is_the_reference_trunk(nets, stride_on, hw):
    _one_part_is_the_reference_trunk(nets[stride_on], hw)


@pytest.mark.parametrize("fuse_downsample,fuse_stem_pool", FUSIONS)
def test_one_part_is_the_reference_trunk_under_each_fusion(nets, fuse_downsample, fuse_stem_pool):
    with _fusions(nets["3x3"], fuse_downsample, fuse_stem_pool) as net:
        _one_part_is_the_reference_trunk(net, SIZES[0])


def _two_parts_are_the_plan_on_each_slice(net, hw, lag):
    plan = net.plan(lag)
    img = _imgs(5, *hw, seed=2)
    with ops.tuning(0, trunk_parts=1):
        a = plan.forward_u8(img[:2], return_x3=True)
        b = plan.forward_u8(img[2:], return_x3=True)
    before = plan.counters()
    with ops.tuning(0, trunk_parts=2):
        assert plan.parts(5, *hw) == 2
        x3, x4, x3a, x4a = plan.forward_u8(img, return_x3=True)
    torch.cuda.synchronize()
    after = plan.counters()
    assert after[1] == before[1] + 1 and after[2] > before[2]
    assert _same(x4, torch.cat([a[1], b[1]])) and _same(x3, torch.cat([a[0], b[0]]))
    # records hold float bits of values >= 0: integer max is the float max
    assert torch.equal(x4a, torch.maximum(a[3], b[3]))
    # x3's record is folded from the parts' own records: the same maximum
    assert ops.amax_value(x3a) == max(ops.amax_value(a[2]), ops.amax_value(b[2]))


@pytest.mark.parametrize("lag", [1, 0, 3])
@pytest.mark.parametrize("hw", SIZES)
def test_two_parts_are_the_plan_on_each_slice(nets, hw, lag):
    _two_parts_are_the_plan_on_each_slice(nets["3x3"], hw, lag)


@pytest.mark.parametrize("fuse_downsample,fuse_stem_pool", FUSIONS)
def test_two_parts_are_the_plan_on_each_slice_under_each_fusion(nets, fuse_downsample, fuse_stem_pool):
    with _fusions(nets["3x3"], fuse_downsample, fuse_stem_pool) as net:
        _two_parts_are_the_plan_on_each_slice(net, SIZES[0], 1)


@pytest.mark.parametrize("side_stream", [False, True])
def test_join_orders_the_callers_stream(nets, side_stream):
    net = nets["3x3"]
    plan = net.plan()
    img = _imgs(5, 96, 80, seed=3)
    stream = torch.cuda.Stream(DEV) if side_stream else torch.cuda.current_stream(DEV)
    stream.wait_stream(torch.cuda.current_stream(DEV))
    with torch.cuda.stream(stream), ops.tuning(0, trunk_parts=2):
        x4_a, _ = plan.forward_u8(img)
        f_a = ops.l2_normalize(ops.gem_pool(x4_a))  # right behind the forward, no sync
        x4_b, _ = plan.forward_u8(img)
        f_b = ops.l2_normalize(ops.gem_pool(x4_b))
    torch.cuda.synchronize()
    assert _same(x4_a, x4_b) and _same(f_a, f_b)
    assert _same(f_a, ops.l2_normalize(ops.gem_pool(x4_a)))  # what the finished x4 gives
    with ops.tuning(0, trunk_parts=1):
        assert _same(x4_a, torch.cat([plan.forward_u8(img[:2])[0], plan.forward_u8(img[2:])[0]]))


def test_auto_rule_keeps_small_batches_in_one_part():
    net = ResNet("resnet50", seed=6, device=DEV)
    plan = ops.TrunkPlan(net)
    for hw in SIZES:
        assert plan.parts(5, *hw) == 1
        plan.forward_u8(_imgs(5, *hw))
    torch.cuda.synchronize()
    assert plan.counters() == (len(SIZES), 0, 0)  # no plan stream touched
    # the rule itself (include/rr.h): two parts from two 256 x 256 tiles of the
    # last stage's output per compute unit and part
    cus = torch.cuda.get_device_properties(0).multi_processor_count

    def rule(b, h, w):
        rows = (b // 2) * -(-h // 32) * -(-w // 32)
        return 2 if b >= 2 and -(-rows // 256) * (2048 // 256) >= 2 * cus else 1

    for b, h, w in [(1, 224, 224), (2, 224, 224), (128, 224, 224), (640, 224, 224), (659, 224, 224),
                    (660, 224, 224), (1280, 224, 224), (64, 1024, 1024)]:
        assert plan.parts(b, h, w) == rule(b, h, w), (b, h, w)
    with ops.tuning(0, trunk_parts=2):
        assert plan.parts(1, 64, 64) == 1 and plan.parts(2, 64, 64) == 2


def _timed_forward(plan, img, parts):
    timer = ops.KernelTimer(0)
    e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    with ops.tuning(0, trunk_parts=parts):
        plan.forward_u8(img)  # untimed: first-use costs
        torch.cuda.synchronize()
        timer.enable(True)
        try:
            e0.record()
            plan.forward_u8(img)
            e1.record()
            torch.cuda.synchronize()
            uni, tot, n = timer.collect_ex(_lib.TIME_GEMM)
            timer.collect(_lib.TIME_ELEM)
        finally:
            timer.enable(False)
    return uni, tot, n, e0.elapsed_time(e1)


def test_timer_one_part_is_the_sum(nets):
    """On one stream the union is the former formula, the sum over the
    launches of hipEventElapsedTime(start_i, stop_i), which
    rr_timing_collect_ex returns from the same events.  They differ by the
    float rounding of the start offsets at most: an offset below `wall` ms
    carries an error below wall * 2^-24, and two neighbours can be made to
    overlap by twice that, once per launch."""
    uni, tot, n, wall = _timed_forward(nets["3x3"].plan(), _imgs(3, 96, 80, seed=4), 1)
    print(f"one part: union {uni:.6f} ms, sum {tot:.6f} ms, {n} launches, wall {wall:.4f} ms")
    assert n == N_CONV
    assert tot > 0 and abs(uni - tot) <= n * wall * 2.0 ** -23
    # a single launch: the one interval's own duration, whichever formula
    timer = ops.KernelTimer(0)
    x = torch.randn(8, 64, device=DEV)
    w = torch.randn(32, 64, device=DEV)
    timer.enable(True)
    try:
        ops.linear(x, w)
        uni1, tot1, n1 = timer.collect_ex(_lib.TIME_GEMM)
    finally:
        timer.enable(False)
    assert n1 == 1 and uni1 == tot1 > 0


def test_timer_two_parts_is_the_union(nets):
    """Co-running launches: the class time stays within the wall time between
    two events around the forward (plus the offsets' float rounding, as
    above), and the count is both parts' launches."""
    uni, tot, n, wall = _timed_forward(nets["3x3"].plan(), _imgs(5, 96, 80, seed=4), 2)
    print(f"two parts: union {uni:.6f} ms, sum {tot:.6f} ms, {n} launches, wall {wall:.4f} ms")
    assert n == 2 * N_CONV
    assert 0 < uni <= tot
    assert uni <= wall + n * wall * 2.0 ** -23


def test_argument_checks(nets):
    plan = nets["3x3"].plan()
    L, h = _lib.lib(), plan.h
    img = _imgs(2, 64, 64)
    x4 = torch.empty((2, 2, 2, 2048), device=DEV)
    rec = ops.amax_records(1, DEV)
    nbytes = L.rr_trunk_h2_workspace_size(plan.plan, 2, 64, 64, 1)
    assert nbytes > 0 and L.rr_trunk_h2_workspace_size(plan.plan, 2, 64, 64, 2) >= nbytes
    ws = torch.empty(nbytes, dtype=torch.uint8, device=DEV)
    before = plan.counters()

    def call(p, b, hh, ww, wbytes):
        return L.rr_trunk_h2_forward_u8(h, p, img.data_ptr(), b, hh, ww, x4.data_ptr(), rec.data_ptr(), None, None,
                                        ws.data_ptr(), wbytes, None)

    with ops.tuning(0, trunk_parts=1):
        assert call(None, 2, 64, 64, nbytes) == _lib.RR_EINVAL               # null plan
        assert call(plan.plan, 2, 64, 64, nbytes - 1) == _lib.RR_EWORKSPACE   # short workspace
        assert call(plan.plan, 0, 64, 64, nbytes) == _lib.RR_OK               # B = 0: nothing to do
        assert call(plan.plan, -1, 64, 64, nbytes) == _lib.RR_EINVAL
        # (sides that are no multiple of 32 are served, 96 x 80 above: rr.h documents
        # RR_EINVAL for H < 1 or W < 1 only)
        assert call(plan.plan, 2, 0, 64, nbytes) == _lib.RR_EINVAL
        assert call(plan.plan, 2, 64, -32, nbytes) == _lib.RR_EINVAL
    assert plan.counters() == before  # no forward was issued
    for bad in ((2, 0, 64, 1), (2, 64, 64, 3), (-1, 64, 64, 1)):
        assert L.rr_trunk_h2_workspace_size(plan.plan, *bad) == 0
    assert L.rr_trunk_h2_workspace_size(None, 2, 64, 64, 1) == 0
    assert L.rr_trunk_h2_parts(h, None, 2, 64, 64) == _lib.RR_EINVAL
    out = ctypes.c_void_p()
    assert L.rr_trunk_h2_create(h, None, ctypes.byref(out)) == _lib.RR_EINVAL and not out.value
    assert L.rr_set_tuning(h, _lib.TUNE_TRUNK_PARTS, 3) == _lib.RR_EINVAL
