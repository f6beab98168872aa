"""Records tests/golden/trunk_launches.json: every ops call the eager bottleneck
trunks (networks.ResNet, networks.SENet) make per forward, and the conv list
ops.TrunkPlan hands the native plan, without a GPU.

    python tests/golden/make_trunk_launches.py

networks.ops is replaced by a Recorder whose stand-ins return correctly shaped
CPU tensors and log their arguments: tensors and records named by order of
first appearance (t0, t1, ... with their shape; r0, r1, ...), weights by conv
name.  The fixture in git was written by the last commit whose trunks each had
a stage loop of their own; tests/test_trunk_walk_host.py runs the same
recorder (record_all) and compares.

Log rows:
  [amax_records, n]                      [amax_f32, x, rec]
  [conv2d_h2, out, x, xa, w, bias, stride, pad, residual, relu, ya]
  [conv2d, out, x, w, bias, stride, pad, residual, relu]
  [stem_pool_h2, out, x, xa, w, bias, stride, pad, ya]
  [maxpool2d, out, x, k, stride, pad]
  [bottleneck_out_h2, out, y, ya, x, xa, w, stride, out_amax]
  [se_squeeze, out, y]                   [linear_splitk, out, x, w, bias, act]
  [se_apply, out, y, hidden, w2, identity, relu, want_gate, out=, out_amax]
  [hook, i]                              [return, x3, x4, x3_amax, x4_amax]
Plan rows: [w2, w_iscale, bias, cin, cout, kh, kw, stride, pad, residual, relu]."""
import contextlib
import json
import os
import sys
import types

import torch

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, os.path.dirname(os.path.dirname(HERE)))
from research_image_retrieval_amd import _lib, networks, ops  # noqa: E402
from research_image_retrieval_amd import weights as W  # noqa: E402

PATH = os.path.join(HERE, "trunk_launches.json")
INPUTS = ((2, 64, 64, 4), (1, 33, 47, 4))
SEED = 11


def _out(n, k, s, p):
    return (n + 2 * p - k) // s + 1


class _H2Conv:
    def __init__(self, w):
        self.cout, self.kh, self.kw, self.cin = w.shape
        self.planes, self.iscale = torch.zeros(1), torch.zeros(1)


class _H2Bottleneck:
    def __init__(self, w3, b3, wd, bd):
        self.cout, self.planes, self.cin = w3.shape[0], w3.shape[-1], wd.shape[-1]
        self.planes2, self.iscale, self.bias = torch.zeros(1), torch.zeros(1), torch.zeros(1)


class Recorder:
    """What networks.py reads of ops while a bottleneck trunk is built and walked."""
    H2Conv, H2Bottleneck = _H2Conv, _H2Bottleneck

    def __init__(self):
        self.log, self._seen, self._keep, self._weights, self._nets = [], {}, [], {}, []

    def name_weights(self, net):
        """Name net's weights (tensors by address, split weights by identity too)."""
        self._nets.append(net)  # a named address stays that weight's
        for k, (w, b) in net.convs.items():
            self._weights[w.data_ptr()], self._weights[b.data_ptr()] = f"w:{k}", f"b:{k}"
        for k, c in net.convs_h2.items():
            self._weights[id(c)] = f"h2:{k}"
            self._weights[c.planes.data_ptr()], self._weights[c.iscale.data_ptr()] = f"h2:{k}.planes", f"h2:{k}.iscale"
        for k, c in getattr(net, "bneck_h2", {}).items():
            self._weights[id(c)] = f"entry:{k}"
            for a in ("planes2", "iscale", "bias"):
                self._weights[getattr(c, a).data_ptr()] = f"entry:{k}.{a}"
        for k, (w1, w2) in getattr(net, "se", {}).items():
            self._weights[w1.data_ptr()], self._weights[w2.data_ptr()] = f"se1:{k}", f"se2:{k}"

    def weight(self, key):
        return None if key is None else self._weights[key]

    def name(self, t):
        if t is None or isinstance(t, (bool, int, float, str)):
            return t
        if not isinstance(t, torch.Tensor):
            return self._weights[id(t)]
        p = t.data_ptr()
        if p in self._weights:
            return self._weights[p]
        if p not in self._seen:
            kind = "r" if t.dtype == torch.int32 else "t"
            self._seen[p] = f"{kind}{sum(v[0] == kind for v in self._seen.values())}"
            self._keep.append(t)  # no address is reused while the log grows
        n = self._seen[p]
        return n if n[0] == "r" else f"{n}{list(t.shape)}"

    def _row(self, op, *args):
        self.log.append([op] + [self.name(a) for a in args])

    def hook(self, i):
        self.log.append(["hook", i])

    def amax_records(self, n, device):
        self.log.append(["amax_records", n])
        return torch.zeros((n, 64), dtype=torch.int32, device=device)

    def amax_f32(self, x, record):
        self._row("amax_f32", x, record)
        return record

    @staticmethod
    def _conv_out(x, cout, kh, kw, stride, pad):
        b, h, w, _ = x.shape
        return torch.empty((b, _out(h, kh, stride, pad), _out(w, kw, stride, pad), cout))

    def conv2d_h2(self, x, x_amax, wc, bias, stride=1, pad=0, residual=None, relu=False, y_amax=None):
        assert x.shape[-1] == wc.cin
        y = self._conv_out(x, wc.cout, wc.kh, wc.kw, stride, pad)
        assert residual is None or residual.shape == y.shape
        self._row("conv2d_h2", y, x, x_amax, wc, bias, stride, pad, residual, relu, y_amax)
        return y

    def conv2d(self, x, w, bias, stride=1, pad=0, residual=None, relu=False):
        assert x.shape[-1] == w.shape[-1]
        y = self._conv_out(x, w.shape[0], w.shape[1], w.shape[2], stride, pad)
        assert residual is None or residual.shape == y.shape
        self._row("conv2d", y, x, w, bias, stride, pad, residual, relu)
        return y

    def stem_pool_h2(self, x, x_amax, wc, bias, stride=2, pad=3, y_amax=None):
        c = self._conv_out(x, 64, wc.kh, wc.kw, stride, pad)
        y = torch.empty((c.shape[0], _out(c.shape[1], 3, 2, 1), _out(c.shape[2], 3, 2, 1), 64))
        self._row("stem_pool_h2", y, x, x_amax, wc, bias, stride, pad, y_amax)
        return y

    def maxpool2d(self, x, k=3, stride=2, pad=1):
        b, h, w, c = x.shape
        y = torch.empty((b, _out(h, k, stride, pad), _out(w, k, stride, pad), c))
        self._row("maxpool2d", y, x, k, stride, pad)
        return y

    def bottleneck_out_h2(self, y, y_amax, x, x_amax, wb, stride, out_amax=None):
        assert y.shape[-1] == wb.planes and x.shape[-1] == wb.cin
        assert (_out(x.shape[1], 1, stride, 0), _out(x.shape[2], 1, stride, 0)) == tuple(y.shape[1:3])
        out = torch.empty(tuple(y.shape[:3]) + (wb.cout,))
        self._row("bottleneck_out_h2", out, y, y_amax, x, x_amax, wb, stride, out_amax)
        return out

    def se_squeeze(self, y):
        m = torch.empty((y.shape[0], y.shape[-1]))
        self._row("se_squeeze", m, y)
        return m

    def linear_splitk(self, x, w, bias, row_scale=None, act=0, residual=None):
        assert row_scale is None and residual is None and x.shape[1] == w.shape[1]
        y = torch.empty((x.shape[0], w.shape[0]))
        self._row("linear_splitk", y, x, w, bias, act)
        return y

    def se_apply(self, y, hidden, w2, identity=None, relu=True, want_gate=False, out=None, out_amax=None):
        assert identity is None or identity.shape == y.shape
        assert tuple(w2.shape) == (y.shape[-1], hidden.shape[1])
        got = torch.empty_like(y) if out is None else out
        self._row("se_apply", got, y, hidden, w2, identity, relu, want_gate, out, out_amax)
        return (got, torch.empty((y.shape[0], y.shape[-1]))) if want_gate else got


@contextlib.contextmanager
def recording():
    """networks.ops is a fresh Recorder inside the block."""
    rec, real = Recorder(), networks.ops
    networks.ops = rec
    try:
        yield rec
    finally:
        networks.ops = real


def walk(net, rec, shape, want_x3):
    """The log of one net.maps() on a zero input of `shape`."""
    rec.log, rec._seen, rec._keep = [], {}, []
    x3, x4, x3a, x4a = net.maps(torch.zeros(shape), rec.hook, want_x3)
    rec._row("return", x3, x4, x3a, x4a)
    return rec.log


def _plan_convs_before_the_trunk_had_them(net, rec):
    """ops.TrunkPlan.__init__'s conv list where the trunk has no plan_convs()
    yet (the commit the fixture was recorded at): the constructor run against a
    stubbed library, its rr_trunk_conv_t array and descriptor read back."""
    seen = {}

    def create(h, desc, out):
        seen["desc"] = desc._obj
        return 0

    fake = types.SimpleNamespace(rr_trunk_h2_create=create, rr_trunk_h2_destroy=lambda h, p: 0)
    saved = (ops._dev, ops.H2Conv, _lib.handle, _lib.lib)
    ops._dev, ops.H2Conv, _lib.handle, _lib.lib = (lambda t: 0), _H2Conv, (lambda d: None), (lambda: fake)
    try:
        plan = ops.TrunkPlan(net)
    finally:
        ops._dev, ops.H2Conv, _lib.handle, _lib.lib = saved
    d = seen["desc"]
    rows = [[c.w2, c.w_iscale, c.bias, c.cin, c.cout, c.kh, c.kw, c.stride, c.pad, c.residual, c.relu]
            for c in plan._convs]
    return rows, list(d.fuse_entry[:d.n_stages])


def plan_rows(net, rec):
    """{"convs": the plan's conv rows, "fuse_entry": per stage} under net's current flags."""
    if hasattr(net, "plan_convs"):
        convs, fuse_entry = net.plan_convs()
        rows = [[c[0].data_ptr(), c[1].data_ptr(), None if c[2] is None else c[2].data_ptr()] + [int(v) for v in c[3:]]
                for c in convs]
    else:
        rows, fuse_entry = _plan_convs_before_the_trunk_had_them(net, rec)
    return {"convs": [[rec.weight(v) for v in r[:3]] + r[3:] for r in rows], "fuse_entry": [int(v) for v in fuse_entry]}


def record_all():
    """{case: log} for every eager case at both INPUTS, {case: plan rows}."""
    out = {"walk": {}, "plan": {}}
    sd = W.synthetic_resnet_state_dict("resnet50", SEED)
    se_sd = W.synthetic_senet_state_dict("senet50", SEED)

    def shapes(tag, net, rec, want_x3=True, inputs=INPUTS):
        for s in inputs:
            out["walk"][f"{tag}/{'x'.join(map(str, s))}/{'x3' if want_x3 else 'no_x3'}"] = walk(net, rec, s, want_x3)

    with recording() as rec:
        for math in ("h2", "f32"):
            for so in W.STRIDE_ON:
                net = networks.ResNet("resnet50", sd, device="cpu", conv_math=math, stride_on=so)
                rec.name_weights(net)
                shapes(f"resnet50/{math}/{so}", net, rec)
                if so == "3x3":
                    shapes(f"resnet50/{math}/{so}", net, rec, want_x3=False)
                if math != "h2":
                    continue
                if so == "3x3":
                    shapes(f"resnet50/{math}/{so}/rgb", net, rec, inputs=((2, 64, 64, 3),))
                for fd in (True, False):
                    for fsp in (True, False):
                        net.fuse_downsample, net.fuse_stem_pool = fd, fsp
                        try:
                            flags = f"fuse_downsample={int(fd)},fuse_stem_pool={int(fsp)}"
                            out["plan"][f"resnet50/{so}/{flags}"] = plan_rows(net, rec)
                            if so == "3x3" and not (fd and fsp):
                                shapes(f"resnet50/{math}/{so}/{flags}", net, rec)
                        finally:
                            net.fuse_downsample, net.fuse_stem_pool = True, True
            net = networks.SENet("senet50", se_sd, device="cpu", conv_math=math)
            rec.name_weights(net)
            shapes(f"senet50/{math}", net, rec)
    return out


if __name__ == "__main__":
    got = record_all()
    with open(PATH, "w") as f:
        json.dump(got, f, separators=(",", ":"), sort_keys=True)
        f.write("\n")
    print(f"{len(got['walk'])} walks, {len(got['plan'])} plans -> {PATH} ({os.path.getsize(PATH)} bytes)")
