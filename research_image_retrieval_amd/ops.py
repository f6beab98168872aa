"""Torch-tensor wrappers over the librr C-ABI (one function per rr_* entry).

PyTorch is used only for device memory and the current HIP stream; every op
below runs a hand-written gfx950 kernel from librr.so.  Inputs must be
contiguous fp32 (uint8 for images) tensors on a ROCm device.
"""
import collections
import ctypes

import torch

from . import _lib

_NULL = None


def _dev(t):
    if not t.is_cuda:
        raise ValueError("librr ops need ROCm device tensors (got a CPU tensor)")
    return t.device.index if t.device.index is not None else torch.cuda.current_device()


def _ptr(t):
    return None if t is None else ctypes.c_void_p(t.data_ptr())


def _stream(dev):
    return ctypes.c_void_p(torch.cuda.current_stream(dev).cuda_stream)


def _f32(t, name):
    if t.dtype != torch.float32:
        raise TypeError(f"{name}: expected float32, got {t.dtype}")
    if not t.is_contiguous():
        raise ValueError(f"{name}: must be contiguous")
    return t


def preprocess_u8(img_nhwc, mean=(0.485, 0.456, 0.406), std=(0.229, 0.224, 0.225), out_c=3):
    """uint8 [B,H,W,3] -> fp32 NHWC normalised (ToTensor + Normalize); out_c=4
    appends a zero channel (stem-conv tap layout)."""
    if img_nhwc.dtype != torch.uint8 or img_nhwc.dim() != 4 or img_nhwc.shape[3] != 3:
        raise ValueError("preprocess_u8: expected uint8 [B,H,W,3]")
    img_nhwc = img_nhwc.contiguous()
    dev = _dev(img_nhwc)
    b, h, w, _ = img_nhwc.shape
    out = torch.empty((b, h, w, out_c), dtype=torch.float32, device=img_nhwc.device)
    m = (ctypes.c_float * 3)(*mean)
    s = (ctypes.c_float * 3)(*std)
    hd = _lib.handle(dev)
    _lib.check(_lib.lib().rr_preprocess_u8_ex(hd, _ptr(img_nhwc), b, h, w, ctypes.cast(m, ctypes.c_void_p),
                                              ctypes.cast(s, ctypes.c_void_p), int(out_c), _ptr(out), _stream(dev)),
               hd, "rr_preprocess_u8")
    return out


def nchw_to_nhwc(x, out_c=None):
    x = _f32(x.contiguous(), "nchw_to_nhwc")
    dev = _dev(x)
    b, c, h, w = x.shape
    oc = c if out_c is None else int(out_c)
    out = torch.empty((b, h, w, oc), dtype=torch.float32, device=x.device)
    hd = _lib.handle(dev)
    _lib.check(_lib.lib().rr_nchw_to_nhwc_ex(hd, _ptr(x), b, c, h, w, oc, _ptr(out), _stream(dev)), hd,
               "rr_nchw_to_nhwc")
    return out


def conv2d(x, w, bias, stride=1, pad=0, residual=None, relu=False):
    """NHWC conv with fused bias/residual/ReLU; w is [Cout,KH,KW,Cin]."""
    _f32(x, "conv2d x")
    _f32(w, "conv2d w")
    dev = _dev(x)
    b, h, wd, cin = x.shape
    cout, kh, kw, cin_w = w.shape
    if cin_w != cin:
        raise ValueError(f"conv2d: Cin mismatch {cin} vs {cin_w}")
    oh = (h + 2 * pad - kh) // stride + 1
    ow = (wd + 2 * pad - kw) // stride + 1
    y = torch.empty((b, oh, ow, cout), dtype=torch.float32, device=x.device)
    if residual is not None:
        _f32(residual, "conv2d residual")
        if tuple(residual.shape) != tuple(y.shape):
            raise ValueError("conv2d: residual shape mismatch")
    if bias is not None:
        _f32(bias, "conv2d bias")
    hd = _lib.handle(dev)
    _lib.check(_lib.lib().rr_conv2d(hd, _ptr(x), b, h, wd, cin, _ptr(w), _ptr(bias), cout, kh, kw, stride, pad,
                                    _ptr(residual), int(relu), _ptr(y), _stream(dev)), hd, "rr_conv2d")
    return y


AMAX_SLOTS = 64  # RR_AMAX_SLOTS: words of one tensor's max-|x| record


def amax_records(n, device):
    """n zeroed max-|x| records [n, RR_AMAX_SLOTS] (int32 words holding float
    bits) for rr_conv2d_h2's x_amax / y_amax."""
    return torch.zeros((n, AMAX_SLOTS), dtype=torch.int32, device=device)


def amax_f32(x, record):
    """Fold max |x| (finite values) into a zeroed record (rr_amax_f32)."""
    x = _f32(x.contiguous(), "amax_f32")
    if record.dtype != torch.int32 or record.numel() != AMAX_SLOTS or not record.is_contiguous():
        raise ValueError("amax_f32: record must be contiguous int32 [RR_AMAX_SLOTS]")
    dev = _dev(x)
    hd = _lib.handle(dev)
    _lib.check(_lib.lib().rr_amax_f32(hd, _ptr(x), x.numel(), _ptr(record), _stream(dev)), hd, "rr_amax_f32")
    return record


def amax_of(x):
    """A fresh record holding max |x|, for a caller of conv2d_h2 that was given none."""
    return amax_f32(x, amax_records(1, x.device)[0])


def amax_value(record):
    """The max a record holds, as a Python float (host read: tests, tools)."""
    return float(record.view(torch.float32).max().item())


def split2_f16(w, kpad=None):
    """fp16 x2 split of the rows of w ([N, K] or [Cout, KH, KW, Cin]) at a
    per-row power-of-two scale (rr_split2_f16): returns (planes int16 [2, N,
    kpad] of fp16 bit patterns, zero past K; iscale fp32 [N] = 2^-e_n)."""
    w = _f32(w.contiguous(), "split2_f16")
    dev = _dev(w)
    rows = w.shape[0]
    k = w.numel() // max(rows, 1)
    kpad = k if kpad is None else int(kpad)
    if kpad < k:
        raise ValueError("split2_f16: kpad < K")
    planes = torch.empty((2, rows, kpad), dtype=torch.int16, device=w.device)
    iscale = torch.empty((rows,), dtype=torch.float32, device=w.device)
    hd = _lib.handle(dev)
    _lib.check(_lib.lib().rr_split2_f16(hd, _ptr(w), rows, k, kpad, _ptr(planes), _ptr(iscale), _stream(dev)), hd,
               "rr_split2_f16")
    return planes, iscale


class H2Conv:
    """Weights of one conv on the f16x2 split core: planes [2, Cout, Kp],
    inverse row scales [Cout], filter (KH, KW, Cin).  Cin == 4 is the NHWC4
    stem (K = KH*KW*4 zero-padded to a multiple of 32)."""

    def __init__(self, w):
        w = _f32(w.contiguous(), "H2Conv")
        cout, kh, kw, cin = w.shape
        if cin % 32 and cin != 4:
            raise ValueError("H2Conv: Cin must be a multiple of 32, or 4 (NHWC4 stem)")
        k = kh * kw * cin
        self.kpad = (k + 31) // 32 * 32 if cin == 4 else k
        self.planes, self.iscale = split2_f16(w.reshape(cout, k), self.kpad)
        self.cout, self.kh, self.kw, self.cin = cout, kh, kw, cin


def conv2d_h2(x, x_amax, wc, bias, stride=1, pad=0, residual=None, relu=False, y_amax=None):
    """conv2d on the f16x2 split core (rr_conv2d_h2): fp32-accurate, wc an
    H2Conv, x_amax the max-|x| record of x; y_amax (optional, zeroed) gets
    max |y| for the next conv."""
    _f32(x, "conv2d_h2 x")
    if not isinstance(wc, H2Conv):
        raise TypeError("conv2d_h2: wc must be an ops.H2Conv")
    dev = _dev(x)
    b, h, wd, cin = x.shape
    if cin != wc.cin:
        raise ValueError(f"conv2d_h2: Cin mismatch {cin} vs {wc.cin}")
    for r, nm in ((x_amax, "x_amax"), (y_amax, "y_amax")):
        if r is not None and (r.dtype != torch.int32 or r.numel() != AMAX_SLOTS or not r.is_contiguous()):
            raise ValueError(f"conv2d_h2: {nm} must be a contiguous int32 [RR_AMAX_SLOTS] record")
    oh = (h + 2 * pad - wc.kh) // stride + 1
    ow = (wd + 2 * pad - wc.kw) // stride + 1
    y = torch.empty((b, oh, ow, wc.cout), dtype=torch.float32, device=x.device)
    if residual is not None:
        _f32(residual, "conv2d_h2 residual")
        if tuple(residual.shape) != tuple(y.shape):
            raise ValueError("conv2d_h2: residual shape mismatch")
    if bias is not None:
        _f32(bias, "conv2d_h2 bias")
    hd = _lib.handle(dev)
    _lib.check(_lib.lib().rr_conv2d_h2(hd, _ptr(x), _ptr(x_amax), b, h, wd, cin, _ptr(wc.planes), _ptr(wc.iscale),
                                       _ptr(bias), wc.cout, wc.kh, wc.kw, stride, pad, _ptr(residual), int(relu),
                                       _ptr(y), _ptr(y_amax), _stream(dev)), hd, "rr_conv2d_h2")
    return y


H2_ROUTE_FAMILIES = ("tile", "stream", "stream256", "halo", "halo_2d")
_H2_ROUTE_INTS = ("family", "cfg", "wm", "wn", "fm", "fn", "bk", "hr", "tpk", "mf16", "nstg", "acc", "il", "pers", "t2")
H2Route = collections.namedtuple("H2Route", _H2_ROUTE_INTS + ("chunk_rows",))


class _H2RouteT(ctypes.Structure):
    _fields_ = [(n, ctypes.c_int) for n in _H2_ROUTE_INTS] + [("chunk_rows", ctypes.c_longlong)]


def h2_route(b, h, w, cin, cout, kh=1, kw=1, stride=1, pad=0, residual=False, relu=False, s3_cfg=0, s3_cfg_res=0,
             halo_mf=-1, halo_2d=-1, conv_il=-1):
    """The kernel instance conv2d_h2 runs for this shape under these tuning
    values (rr_h2_route; host only, no GPU): an H2Route of the rr_h2_route_t
    fields, family as its number (H2_ROUTE_FAMILIES names them).  ValueError
    for a shape conv2d_h2 rejects or a tuning value set_tuning rejects."""
    shape = (ctypes.c_int * 11)(b, h, w, cin, cout, kh, kw, stride, pad, int(bool(residual)), int(bool(relu)))
    tune = (ctypes.c_int * 5)(s3_cfg, s3_cfg_res, halo_mf, halo_2d, conv_il)
    out = _H2RouteT()
    if _lib.lib().rr_h2_route(ctypes.cast(shape, ctypes.c_void_p), ctypes.cast(tune, ctypes.c_void_p),
                              ctypes.cast(ctypes.pointer(out), ctypes.c_void_p)) != 0:
        raise ValueError(f"h2_route: rr_conv2d_h2 rejects {tuple(shape)} or rr_set_tuning rejects {tuple(tune)}")
    return H2Route(*(getattr(out, n) for n in H2Route._fields))


GEMM_ROUTE_FAMILIES = ("f32", "lp", "lpp", "lpp3", "8p", "sweep128", "sweep64")  # family -1: no instance
GEMM_AMODES = {"dense": 0, "conv": 1, "conv_generic": 2, "conv_c4": 3}
GEMM_EMODES = {"store": 0, "scores_t": 1, "filter": 2}
GEMM_DTYPES = {"f32": 0, "bf16": 1, "fp8": 2}
EP_BIAS, EP_RES, EP_GELU, EP_BF16, EP_STATS, EP_LNFOLD = 1, 2, 8, 16, 128, 256  # GemmRoute.epi's flags
GemmRoute = collections.namedtuple("GemmRoute", ("family", "cfg", "wm", "wn", "fm", "fn", "bk", "minb", "gl", "mf16", "il",
                                                 "epi"))


class _GemmShapeT(ctypes.Structure):
    _fields_ = ([(n, ctypes.c_int) for n in ("amode", "emode", "dtype", "m", "n", "k")] +
                [(n, ctypes.c_longlong) for n in ("lda", "ldb", "ldc")] +
                [(n, ctypes.c_int) for n in ("bias", "residual", "activation", "out_bf16", "stats_in", "stats_out",
                                             "row_scales", "k_split", "sym", "aligned16")])


def gemm_route(m, n, k, dtype="f32", emode="store", amode="dense", lda=None, ldb=None, ldc=None, bias=False,
               residual=False, activation=0, out_bf16=False, stats_in=False, stats_out=False, row_scales=False, k_split=0,
               sym=False, aligned16=True, gemm_cfg=0, gemm_bk=0, lp_cfg=0, sweep_form=-1, sweep_mf16=-1, sweep_il=-1):
    """The kernel instance that serves the GEMM C[m, n] = A[m, k] . B[n, k]^T
    of the fp32, bf16 and fp8 kernels under these tuning values (rr_gemm_route;
    host only, no GPU): a GemmRoute of the rr_gemm_route_t fields, family as
    its number (GEMM_ROUTE_FAMILIES names them).  lda / ldb default to k, ldc
    to n (scores_t: m rounded up to 4).  ValueError for a shape the launch
    rejects or a tuning value set_tuning rejects."""
    em = GEMM_EMODES[emode]
    shape = _GemmShapeT(GEMM_AMODES[amode], em, GEMM_DTYPES[dtype], m, n, k, k if lda is None else lda,
                        k if ldb is None else ldb, ((m + 3) // 4 * 4 if em == 1 else n) if ldc is None else ldc, int(bool(bias)),
                        int(bool(residual)), int(activation), int(bool(out_bf16)), int(bool(stats_in)), int(bool(stats_out)),
                        int(bool(row_scales)), k_split, int(bool(sym)), int(bool(aligned16)))
    tune = (ctypes.c_int * 6)(gemm_cfg, gemm_bk, lp_cfg, sweep_form, sweep_mf16, sweep_il)
    out = (ctypes.c_int * len(GemmRoute._fields))()
    if _lib.lib().rr_gemm_route(ctypes.cast(ctypes.pointer(shape), ctypes.c_void_p), ctypes.cast(tune, ctypes.c_void_p),
                                ctypes.cast(out, ctypes.c_void_p)) != 0:
        raise ValueError(f"gemm_route: the launch rejects {m} x {n} x {k} ({dtype}, {emode}, {amode}) or rr_set_tuning "
                         f"rejects {tuple(tune)}")
    return GemmRoute(*out)


def stem_pool_h2(x, x_amax, wc, bias, stride=2, pad=3, y_amax=None):
    """The NHWC4 stem conv + bias + ReLU with the 3x3/2 padding-1 max-pool
    fused (rr_stem_pool_h2): [B,H,W,4] -> pooled [B,PH,PW,64], the same bits
    as conv2d_h2(..., relu=True) followed by maxpool2d for finite inputs."""
    _f32(x, "stem_pool_h2 x")
    if not isinstance(wc, H2Conv) or wc.cin != 4 or wc.cout != 64:
        raise TypeError("stem_pool_h2: wc must be an ops.H2Conv with Cin 4 and Cout 64")
    dev = _dev(x)
    b, h, wd, cin = x.shape
    if cin != 4:
        raise ValueError("stem_pool_h2: x must be NHWC4")
    oh = (h + 2 * pad - wc.kh) // stride + 1
    ow = (wd + 2 * pad - wc.kw) // stride + 1
    y = torch.empty((b, (oh - 1) // 2 + 1, (ow - 1) // 2 + 1, 64), dtype=torch.float32, device=x.device)
    if bias is not None:
        _f32(bias, "stem_pool_h2 bias")
    hd = _lib.handle(dev)
    _lib.check(_lib.lib().rr_stem_pool_h2(hd, _ptr(x), _ptr(x_amax), b, h, wd, _ptr(wc.planes), _ptr(wc.iscale),
                                          _ptr(bias), 64, wc.kh, wc.kw, stride, pad, _ptr(y), _ptr(y_amax),
                                          _stream(dev)), hd, "rr_stem_pool_h2")
    return y


class H2Bottleneck:
    """Weights of a stage-entry bottleneck's conv3 + downsample projection as
    one f16x2 GEMM (rr_bottleneck_out_h2): rows [W3 | Wd] split together,
    bias = b3 + bd."""

    def __init__(self, w3, b3, wd, bd):
        w3, wd = _f32(w3.contiguous(), "H2Bottleneck w3"), _f32(wd.contiguous(), "H2Bottleneck wd")
        cout, planes = w3.shape[0], w3.numel() // w3.shape[0]
        cin = wd.numel() // wd.shape[0]
        if wd.shape[0] != cout or tuple(w3.shape[1:3]) != (1, 1) or tuple(wd.shape[1:3]) != (1, 1):
            raise ValueError("H2Bottleneck: 1x1 conv3 and downsample with the same Cout")
        self.planes, self.cin, self.cout = planes, cin, cout
        self.planes2, self.iscale = split2_f16(torch.cat([w3.reshape(cout, planes), wd.reshape(cout, cin)], 1))
        self.bias = (b3.double() + bd.double()).float().contiguous() if b3 is not None else bd.contiguous()


def bottleneck_out_h2(y, y_amax, x, x_amax, wb, stride, out_amax=None):
    """ReLU(conv3(y) + downsample(x)) of a stage-entry bottleneck as one f16x2
    GEMM (rr_bottleneck_out_h2): y [B,OH,OW,planes], x [B,H,W,cin]."""
    _f32(y, "bottleneck_out_h2 y")
    _f32(x, "bottleneck_out_h2 x")
    if not isinstance(wb, H2Bottleneck):
        raise TypeError("bottleneck_out_h2: wb must be an ops.H2Bottleneck")
    b, oh, ow, planes = y.shape
    bx, hx, wx, cin = x.shape
    if planes != wb.planes or cin != wb.cin or bx != b:
        raise ValueError("bottleneck_out_h2: shape mismatch")
    dev = _dev(y)
    out = torch.empty((b, oh, ow, wb.cout), dtype=torch.float32, device=y.device)
    hd = _lib.handle(dev)
    _lib.check(_lib.lib().rr_bottleneck_out_h2(hd, _ptr(y), _ptr(y_amax), b, oh, ow, planes, _ptr(x), _ptr(x_amax),
                                               hx, wx, cin, int(stride), _ptr(wb.planes2), _ptr(wb.iscale),
                                               _ptr(wb.bias), wb.cout, _ptr(out), _ptr(out_amax), _stream(dev)),
               hd, "rr_bottleneck_out_h2")
    return out


class TrunkPlan:
    """A networks.ResNet's f16x2 trunk as one native call per forward
    (rr_trunk_h2_*, include/rr.h): uint8 pixels -> x4 (and x3) with their
    max-|x| records, through the launches ResNet.maps issues, for the
    whole batch on the current stream or, where the batch is large enough
    (rr.h's rule; ``ops.tuning(dev, trunk_parts=1 | 2)`` forces it), in two
    parts on the plan's two streams, part 1 ``lag`` convs behind part 0.  The
    plan reads the ResNet's split weights in place, so it keeps the net
    alive."""

    def __init__(self, net, lag=1):
        if net.conv_math != "h2":
            raise ValueError("TrunkPlan: the native plan runs the f16x2 trunk (conv_math='h2')")
        self.net = net
        convs, fuse_entry = net.plan_convs()
        self.dev = _dev(convs[0][0])
        convs = [_lib.TrunkConv(w2.data_ptr(), iscale.data_ptr(), None if bias is None else bias.data_ptr(),
                                *(int(v) for v in c)) for w2, iscale, bias, *c in convs]
        self._convs = (_lib.TrunkConv * len(convs))(*convs)
        d = _lib.TrunkDesc()
        d.n_stages = len(net.layers)
        for i, nb in enumerate(net.layers):
            d.blocks[i], d.fuse_entry[i] = nb, int(fuse_entry[i])
        d.stride_on = 0 if net.stride_on == "3x3" else 1
        d.fuse_stem_pool = int(bool(net.fuse_stem_pool and convs[0].cout == 64))
        d.lag = int(lag)
        d.mean[:] = (0.485, 0.456, 0.406)
        d.std[:] = (0.229, 0.224, 0.225)
        d.n_convs = len(convs)
        d.convs = ctypes.cast(self._convs, ctypes.POINTER(_lib.TrunkConv))
        self.h = _lib.handle(self.dev)
        self.out_c = convs[-1].cout
        self.plan = ctypes.c_void_p()
        _lib.check(_lib.lib().rr_trunk_h2_create(self.h, ctypes.byref(d), ctypes.byref(self.plan)), self.h,
                   "rr_trunk_h2_create")

    def __del__(self):
        plan = getattr(self, "plan", None)
        if plan:
            self.plan = None
            try:
                _lib.lib().rr_trunk_h2_destroy(self.h, plan)
            except Exception:  # interpreter shutdown: the module's globals may be gone
                pass

    def parts(self, b, h, w):
        """The number of parts a forward of [b, h, w, 3] images will run in."""
        n = _lib.lib().rr_trunk_h2_parts(self.h, self.plan, int(b), int(h), int(w))
        if n < 0:
            _lib.check(n, self.h, "rr_trunk_h2_parts")
        return n

    def counters(self):
        """(forwards, two-part forwards, operations issued on the plan's own streams)."""
        out = (ctypes.c_longlong * 3)()
        _lib.check(_lib.lib().rr_trunk_h2_counters(self.plan, out), self.h, "rr_trunk_h2_counters")
        return tuple(out)

    def forward_u8(self, img_nhwc_u8, return_x3=False):
        """uint8 [B,H,W,3] -> (x4, x4's record), or with
        return_x3 (x3, x4, x3's record, x4's record), on the current stream."""
        img = img_nhwc_u8
        if img.dtype != torch.uint8 or img.dim() != 4 or img.shape[3] != 3:
            raise ValueError("TrunkPlan.forward_u8: expected uint8 [B,H,W,3]")
        if _dev(img) != self.dev:
            raise ValueError("TrunkPlan.forward_u8: images on another device than the plan's weights")
        img = img.contiguous()
        b, h, w, _ = img.shape
        if h < 1 or w < 1:
            raise ValueError("TrunkPlan.forward_u8: empty images")
        L = _lib.lib()

        def halved(n, times):  # every stride-2 step (7x7/2 pad 3, 3x3/2 pad 1, 1x1/2) maps n to (n - 1) // 2 + 1
            for _ in range(times):
                n = (n - 1) // 2 + 1
            return n

        n2 = 1 + len(self.net.layers)  # the stem, its pool, every stage but the first
        x4 = torch.empty((b, halved(h, n2), halved(w, n2), self.out_c), dtype=torch.float32, device=img.device)
        # (the forward zeroes the records it publishes)
        rec = torch.empty((2 if return_x3 else 1, AMAX_SLOTS), dtype=torch.int32, device=img.device) if b else \
            amax_records(2 if return_x3 else 1, img.device)
        x3 = None
        if return_x3:
            x3 = torch.empty((b, halved(h, 4), halved(w, 4), self.net.outputdim_block4), dtype=torch.float32,
                             device=img.device)
        if b:
            nbytes = L.rr_trunk_h2_workspace_size(self.plan, b, h, w, self.parts(b, h, w))
            ws = torch.empty(nbytes, dtype=torch.uint8, device=img.device)
            _lib.check(L.rr_trunk_h2_forward_u8(self.h, self.plan, _ptr(img), b, h, w, _ptr(x4), _ptr(rec[-1]),
                                                _ptr(x3), _ptr(rec[0]) if return_x3 else None, _ptr(ws), nbytes,
                                                _stream(self.dev)), self.h, "rr_trunk_h2_forward_u8")
        return (x3, x4, rec[0], rec[1]) if return_x3 else (x4, rec[0])


def resize_bilinear(x_nhwc, out_h, out_w, scale_factor=None):
    """NHWC bilinear resize, align_corners=False.  With ``scale_factor`` the
    source index uses 1/scale_factor, as F.interpolate(scale_factor=s) does."""
    _f32(x_nhwc, "resize_bilinear")
    dev = _dev(x_nhwc)
    b, h, w, c = x_nhwc.shape
    y = torch.empty((b, out_h, out_w, c), dtype=torch.float32, device=x_nhwc.device)
    inv = 0.0 if scale_factor is None else float(1.0 / scale_factor)
    hd = _lib.handle(dev)
    _lib.check(_lib.lib().rr_resize_bilinear(hd, _ptr(x_nhwc), b, h, w, c, int(out_h), int(out_w), inv, inv, _ptr(y),
                                             _stream(dev)), hd, "rr_resize_bilinear")
    return y


def maxpool2d(x, k=3, stride=2, pad=1):
    _f32(x, "maxpool2d")
    dev = _dev(x)
    b, h, w, c = x.shape
    oh = (h + 2 * pad - k) // stride + 1
    ow = (w + 2 * pad - k) // stride + 1
    y = torch.empty((b, oh, ow, c), dtype=torch.float32, device=x.device)
    hd = _lib.handle(dev)
    _lib.check(_lib.lib().rr_maxpool2d(hd, _ptr(x), b, h, w, c, k, stride, pad, _ptr(y), _stream(dev)), hd,
               "rr_maxpool2d")
    return y


def gem_pool(x_nhwc, p=3.0, eps=1e-6):
    """[B,H,W,C] (or [B,HW,C]) -> [B,C] GeM."""
    _f32(x_nhwc, "gem_pool")
    dev = _dev(x_nhwc)
    b, c = x_nhwc.shape[0], x_nhwc.shape[-1]
    hw = x_nhwc.numel() // (b * c) if b * c else 0
    out = torch.empty((b, c), dtype=torch.float32, device=x_nhwc.device)
    hd = _lib.handle(dev)
    _lib.check(_lib.lib().rr_gem_pool(hd, _ptr(x_nhwc), b, hw, c, float(p), float(eps), _ptr(out), _stream(dev)), hd,
               "rr_gem_pool")
    return out


def linear(x, w, bias=None):
    """y = x @ w.T + bias, x [M,K], w [N,K]."""
    _f32(x, "linear x")
    _f32(w, "linear w")
    dev = _dev(x)
    m, k = x.shape
    n = w.shape[0]
    y = torch.empty((m, n), dtype=torch.float32, device=x.device)
    hd = _lib.handle(dev)
    _lib.check(_lib.lib().rr_linear(hd, _ptr(x), m, k, _ptr(w), _ptr(bias), n, _ptr(y), _stream(dev)), hd,
               "rr_linear")
    return y


def l2_normalize(x, eps=1e-12, out=None):
    _f32(x, "l2_normalize")
    dev = _dev(x)
    m, d = x.shape
    y = torch.empty_like(x) if out is None else out
    hd = _lib.handle(dev)
    _lib.check(_lib.lib().rr_l2_normalize(hd, _ptr(x), m, d, float(eps), _ptr(y), _stream(dev)), hd,
               "rr_l2_normalize")
    return y


def dolg_local_pool(y_nhwc, w2, b2):
    """DOLG local branch after conv1+BN (rr_dolg_local_pool): y [B,H,W,C] (or
    [B,HW,C], pre-ReLU), conv2 weight w2 [C] and bias b2 (python float) ->
    m [B,C] = mean_p softplus(w2 . relu(y_p) + b2) y_p / max(||y_p||, 1e-12)."""
    _f32(y_nhwc, "dolg_local_pool y")
    _f32(w2, "dolg_local_pool w2")
    dev = _dev(y_nhwc)
    b, c = y_nhwc.shape[0], y_nhwc.shape[-1]
    if w2.numel() != c:
        raise ValueError(f"dolg_local_pool: w2 has {w2.numel()} weights for {c} channels")
    hw = y_nhwc.numel() // (b * c) if b * c else 1
    out = torch.empty((b, c), dtype=torch.float32, device=y_nhwc.device)
    hd = _lib.handle(dev)
    _lib.check(_lib.lib().rr_dolg_local_pool(hd, _ptr(y_nhwc), b, hw, c, _ptr(w2), float(b2), _ptr(out), _stream(dev)),
               hd, "rr_dolg_local_pool")
    return out


def dolg_orth_fuse(fg, m):
    """[fg | m - fg (fg . m) / (fg . fg)]: fg, m [B,C] -> [B,2C] (rr_dolg_orth_fuse)."""
    _f32(fg, "dolg_orth_fuse fg")
    _f32(m, "dolg_orth_fuse m")
    if fg.dim() != 2 or tuple(fg.shape) != tuple(m.shape):
        raise ValueError("dolg_orth_fuse: fg and m must both be [B,C]")
    dev = _dev(fg)
    b, c = fg.shape
    out = torch.empty((b, 2 * c), dtype=torch.float32, device=fg.device)
    hd = _lib.handle(dev)
    _lib.check(_lib.lib().rr_dolg_orth_fuse(hd, _ptr(fg), _ptr(m), b, c, _ptr(out), _stream(dev)), hd,
               "rr_dolg_orth_fuse")
    return out


def soa_attention(fgh, c):
    """SOLAR's second-order attention (rr_soa_attention): fgh [B,H,W,3c] (or
    [B,HW,3c]) = one 1x1 conv's output [f | g | h], f and g pre-ReLU with their
    BN folded -> softmax(c^-0.5 relu(f) relu(g)^T) h, shaped as fgh with c
    channels."""
    _f32(fgh, "soa_attention fgh")
    c = int(c)
    if fgh.dim() not in (3, 4) or fgh.shape[-1] != 3 * c:
        raise ValueError(f"soa_attention: expected [B,H,W,{3 * c}] or [B,HW,{3 * c}], got {tuple(fgh.shape)}")
    dev = _dev(fgh)
    b = fgh.shape[0]
    hw = fgh.numel() // (b * 3 * c) if b * c else 1
    out = torch.empty(tuple(fgh.shape[:-1]) + (c,), dtype=torch.float32, device=fgh.device)
    hd = _lib.handle(dev)
    _lib.check(_lib.lib().rr_soa_attention(hd, _ptr(fgh), b, hw, c, _ptr(out), _stream(dev)), hd, "rr_soa_attention")
    return out


def _rows128(t, rows, heads, name):
    """A [rows, heads * 128] fp32 operand of attention_hd128: a 2-D tensor or a
    column slice of one (unit column stride, any row stride) -> its row stride."""
    if t.dtype != torch.float32:
        raise TypeError(f"attention_hd128 {name}: expected float32, got {t.dtype}")
    if t.dim() != 2 or tuple(t.shape) != (rows, heads * 128):
        raise ValueError(f"attention_hd128 {name}: expected [{rows},{heads * 128}], got {tuple(t.shape)}")
    ld = t.stride(0) if rows > 1 else max(t.stride(0), heads * 128)
    if t.stride(1) != 1 or ld < heads * 128:
        raise ValueError(f"attention_hd128 {name}: columns must be contiguous and rows at least {heads * 128} apart")
    if ld % 4 or t.data_ptr() % 16:
        raise ValueError(f"attention_hd128 {name}: row stride % 4 == 0 and a 16-B aligned first element")
    return ld


def attention_hd128(q, k, v, b, nq, nk, heads):
    """Multi-head attention at head width 128 (rr_attention_hd128): q [b nq,
    heads 128], k and v [b nk, heads 128], each a 2-D fp32 tensor or a column
    slice of a wider one (e.g. qkv[:, :1024]) -> softmax(128^-0.5 q k^T) v,
    dense [b nq, heads 128]."""
    b, nq, nk, heads = int(b), int(nq), int(nk), int(heads)
    if b < 0 or heads < 1 or not 1 <= nq <= 65535 or not 1 <= nk <= 65535:
        raise ValueError("attention_hd128: b >= 0, heads >= 1, 1 <= nq, nk <= 65535")
    ldq = _rows128(q, b * nq, heads, "q")
    ldk = _rows128(k, b * nk, heads, "k")
    ldv = _rows128(v, b * nk, heads, "v")
    dev = _dev(q)
    if k.device != q.device or v.device != q.device:
        raise ValueError("attention_hd128: q, k and v must be on one device")
    out = torch.empty((b * nq, heads * 128), dtype=torch.float32, device=q.device)
    if b == 0:
        return out
    hd = _lib.handle(dev)
    _lib.check(_lib.lib().rr_attention_hd128(hd, _ptr(q), ldq, _ptr(k), ldk, _ptr(v), ldv, b, nq, nk, heads, _ptr(out),
                                             _stream(dev)), hd, "rr_attention_hd128")
    return out


def token_pool(x, query):
    """Object-token pooling (rr_token_pool): x [B,H,W,C] (or [B,HW,C]), query
    [n_obj,C] -> [B,n_obj,C] = sum_p softmax_o(query_o . x_p) x_p, the softmax
    over the objects."""
    _f32(x, "token_pool x")
    _f32(query, "token_pool query")
    if x.dim() not in (3, 4) or query.dim() != 2 or query.shape[1] != x.shape[-1]:
        raise ValueError(f"token_pool: x [B,H,W,C] or [B,HW,C] and query [n_obj,C], got {tuple(x.shape)} and "
                         f"{tuple(query.shape)}")
    b, c, n_obj = x.shape[0], x.shape[-1], query.shape[0]
    if c % 256 or not 256 <= c <= 1024 or not 1 <= n_obj <= 8:
        raise ValueError("token_pool: c % 256 == 0, 256 <= c <= 1024, 1 <= n_obj <= 8")
    hw = x.numel() // (b * c) if b else 1
    if hw < 1:
        raise ValueError("token_pool: an empty map")
    dev = _dev(x)
    out = torch.empty((b, n_obj, c), dtype=torch.float32, device=x.device)
    hd = _lib.handle(dev)
    _lib.check(_lib.lib().rr_token_pool(hd, _ptr(x), b, hw, c, _ptr(query), n_obj, _ptr(out), _stream(dev)), hd,
               "rr_token_pool")
    return out


def _how_args(name, x, centroids):
    _f32(x, f"{name} x")
    _f32(centroids, f"{name} centroids")
    if x.dim() not in (3, 4) or centroids.dim() != 2 or centroids.shape[1] != x.shape[-1]:
        raise ValueError(f"{name}: x [B,N,D] or [B,H,W,D] and centroids [K,D], got {tuple(x.shape)} and "
                         f"{tuple(centroids.shape)}")
    b, d, k = x.shape[0], x.shape[-1], centroids.shape[0]
    if d % 32 or not 32 <= d <= 256 or not 1 <= k <= 128:
        raise ValueError(f"{name}: d % 32 == 0, 32 <= d <= 256, 1 <= k <= 128")
    n = x.numel() // (b * d) if b else 1
    if not 1 <= n <= 65535:
        raise ValueError(f"{name}: 1 <= positions <= 65535")
    if centroids.device != x.device:
        raise ValueError(f"{name}: x and centroids must be on one device")
    return b, n, d, k


def how_vlad(x, centroids, alpha=100.0):
    """HOW's VLAD pooling (rr_how_vlad): x [B,N,D] (or NHWC [B,H,W,D]), the RAW
    local_proj rows, centroids [K,D] -> [B, K D] = sum_p softmax_c(-alpha
    ||x^_p - c||)[c] (x^_p - c) with x^ = x / max(||x||, 1e-12).  The final L2 over
    the K D values is the caller's l2_normalize."""
    b, n, d, k = _how_args("how_vlad", x, centroids)
    dev = _dev(x)
    out = torch.empty((b, k * d), dtype=torch.float32, device=x.device)
    if b == 0:
        return out
    hd = _lib.handle(dev)
    _lib.check(_lib.lib().rr_how_vlad(hd, _ptr(x), b, n, d, _ptr(centroids), k, float(alpha), _ptr(out), _stream(dev)),
               hd, "rr_how_vlad")
    return out


def how_asmk(x, centroids, weights):
    """HOW's ASMK pooling (rr_how_asmk): x as how_vlad's, centroids [K,D],
    weights [K] -> [B,K], weights[c] x the number of positions nearest to
    centroid c whose distance is below the image's mean + std of those
    distances.  The final L2 is the caller's l2_normalize."""
    b, n, d, k = _how_args("how_asmk", x, centroids)
    _f32(weights, "how_asmk weights")
    if weights.dim() != 1 or weights.shape[0] != k or weights.device != x.device:
        raise ValueError(f"how_asmk: weights must be [{k}] on x's device, got {tuple(weights.shape)}")
    dev = _dev(x)
    out = torch.empty((b, k), dtype=torch.float32, device=x.device)
    if b == 0:
        return out
    hd = _lib.handle(dev)
    _lib.check(_lib.lib().rr_how_asmk(hd, _ptr(x), b, n, d, _ptr(centroids), _ptr(weights), k, _ptr(out), _stream(dev)),
               hd, "rr_how_asmk")
    return out


def sos_cov(z, hid, w3, b3, want_att=False):
    """SoSNet's attention-weighted covariance pooling (rr_sos_cov): z [B,N,C] (or
    NHWC [B,H,W,C]), the RAW rows of the second-order projection WITHOUT its
    bias; hid [B,N,DH] (or NHWC), the ReLU'd second layer of the attention MLP,
    w3 [DH] and b3 (python float) its last layer; hid None: no attention (a = 1)
    -> (out [B, C (C + 1) / 2], the UN-normalised packed upper triangle of the
    centred covariance of a_p z_p in torch.triu_indices order, inv_norm [B] =
    1 / max(||out row||, 1e-12)), and att [B,N] as a third value with
    want_att."""
    _f32(z, "sos_cov z")
    if z.dim() not in (3, 4):
        raise ValueError(f"sos_cov: z [B,N,C] or [B,H,W,C], got {tuple(z.shape)}")
    b, c = z.shape[0], z.shape[-1]
    if c % 32 or not 32 <= c <= 512:
        raise ValueError("sos_cov: c % 32 == 0, 32 <= c <= 512")
    n = z.numel() // (b * c) if b else 2
    if not 2 <= n <= 65535:
        raise ValueError("sos_cov: 2 <= positions <= 65535 (one position: the reference divides by N - 1 = 0 and "
                         "returns NaN)")
    dh = 0
    if hid is not None:
        _f32(hid, "sos_cov hid")
        _f32(w3, "sos_cov w3")
        dh = hid.shape[-1]
        if hid.dim() not in (3, 4) or hid.shape[0] != b or hid.numel() != b * n * dh or w3.numel() != dh:
            raise ValueError(f"sos_cov: hid [B,N,DH] for z's positions and w3 [DH], got {tuple(hid.shape)} and "
                             f"{tuple(w3.shape)}")
        if dh % 4 or not 4 <= dh <= 512:
            raise ValueError("sos_cov: dh % 4 == 0, 4 <= dh <= 512")
        if hid.device != z.device or w3.device != z.device:
            raise ValueError("sos_cov: z, hid and w3 must be on one device")
    dev = _dev(z)
    out = torch.empty((b, c * (c + 1) // 2), dtype=torch.float32, device=z.device)
    inv = torch.empty((b,), dtype=torch.float32, device=z.device)
    att = torch.empty((b, n), dtype=torch.float32, device=z.device) if want_att else None
    if b:
        hd = _lib.handle(dev)
        _lib.check(_lib.lib().rr_sos_cov(hd, _ptr(z), b, n, c, _ptr(hid), dh, _ptr(w3) if hid is not None else None,
                                         float(b3), _ptr(att), _ptr(out), _ptr(inv), _stream(dev)), hd, "rr_sos_cov")
    return (out, inv, att) if want_att else (out, inv)


def linear_splitk(x, w, bias, row_scale=None, act=0, residual=None):
    """y = act(row_scale[:, None] * (x @ w.T) + bias + residual) on the split-K
    path (rr_linear_splitk; with a residual [M,N] rr_linear_splitk_ex): x [M,K],
    w [N,K], K % 4 == 0; bias [N], row_scale [M] and residual may be None; act 0
    none, 1 ReLU, 2 QuickGELU."""
    _f32(x, "linear_splitk x")
    _f32(w, "linear_splitk w")
    if x.dim() != 2 or w.dim() != 2 or w.shape[1] != x.shape[1]:
        raise ValueError(f"linear_splitk: x [M,K] and w [N,K], got {tuple(x.shape)} and {tuple(w.shape)}")
    m, k = x.shape
    n = w.shape[0]
    if k % 4 or k == 0 or n == 0:
        raise ValueError("linear_splitk: k % 4 == 0, k > 0, n > 0")
    if bias is not None and (_f32(bias, "linear_splitk bias").numel() != n or bias.device != x.device):
        raise ValueError(f"linear_splitk: bias must be [{n}] on x's device")
    if row_scale is not None and (_f32(row_scale, "linear_splitk row_scale").numel() != m or
                                  row_scale.device != x.device):
        raise ValueError(f"linear_splitk: row_scale must be [{m}] on x's device")
    if residual is not None and (tuple(_f32(residual, "linear_splitk residual").shape) != (m, n) or
                                 residual.device != x.device):
        raise ValueError(f"linear_splitk: residual must be [{m},{n}] on x's device")
    if int(act) not in (0, 1, 2):
        raise ValueError("linear_splitk: act must be 0, 1 or 2")
    dev = _dev(x)
    if w.device != x.device:
        raise ValueError("linear_splitk: x and w must be on one device")
    y = torch.empty((m, n), dtype=torch.float32, device=x.device)
    if m == 0:
        return y
    hd = _lib.handle(dev)
    if residual is None:
        _lib.check(_lib.lib().rr_linear_splitk(hd, _ptr(x), m, k, _ptr(w), n, _ptr(row_scale), _ptr(bias), int(act),
                                               _ptr(y), _stream(dev)), hd, "rr_linear_splitk")
    else:
        _lib.check(_lib.lib().rr_linear_splitk_ex(hd, _ptr(x), m, k, _ptr(w), n, _ptr(row_scale), _ptr(bias),
                                                  _ptr(residual), int(act), _ptr(y), _stream(dev)), hd,
                   "rr_linear_splitk_ex")
    return y


def cls_attn_pool(x, qt, want_p=False):
    """The token aggregator's folded last-layer attention (rr_cls_attn_pool):
    x [B,seq,D] the layer's input rows, qt [B,heads,D] the folded scaled
    queries -> out [B,heads,D] = sum_j softmax_j(qt_h . x_j) x_j, and p
    [B,heads,seq] as a second value with want_p."""
    _f32(x, "cls_attn_pool x")
    _f32(qt, "cls_attn_pool qt")
    if x.dim() != 3 or qt.dim() != 3 or qt.shape[0] != x.shape[0] or qt.shape[2] != x.shape[2]:
        raise ValueError(f"cls_attn_pool: x [B,seq,D] and qt [B,heads,D], got {tuple(x.shape)} and {tuple(qt.shape)}")
    b, seq, d = x.shape
    heads = qt.shape[1]
    if d % 64 or not 64 <= d <= 1024 or not 1 <= heads <= 16 or not 1 <= seq <= 256:
        raise ValueError("cls_attn_pool: d % 64 == 0, 64 <= d <= 1024, 1 <= heads <= 16, 1 <= seq <= 256")
    dev = _dev(x)
    if qt.device != x.device:
        raise ValueError("cls_attn_pool: x and qt must be on one device")
    out = torch.empty((b, heads, d), dtype=torch.float32, device=x.device)
    p = torch.empty((b, heads, seq), dtype=torch.float32, device=x.device) if want_p else None
    if b:
        hd = _lib.handle(dev)
        _lib.check(_lib.lib().rr_cls_attn_pool(hd, _ptr(x), b, seq, d, _ptr(qt), heads, _ptr(p), _ptr(out),
                                               _stream(dev)), hd, "rr_cls_attn_pool")
    return (out, p) if want_p else out


def _levels(levels, name):
    lv = [int(v) for v in levels]
    if not 1 <= len(lv) <= 8 or any(v < 1 for v in lv):
        raise ValueError(f"{name}: 1 <= len(levels) <= 8, every level >= 1")
    return (ctypes.c_int * len(lv))(*lv), len(lv)


def spp_regions(hgt, wid, levels):
    """Regions of the reference's max-pool pyramid on an hgt x wid map
    (rr_spp_regions): per level L, (hgt // (hgt // L)) * (wid // (wid // L));
    ValueError where a level is above hgt or wid (the reference raises "stride
    should not be zero")."""
    arr, n = _levels(levels, "spp_regions")
    r = _lib.lib().rr_spp_regions(int(hgt), int(wid), ctypes.cast(arr, ctypes.c_void_p), n)
    if r < 0:
        raise ValueError(f"spp_regions: a level of {list(levels)} is above the {hgt} x {wid} map (the reference's "
                         "max_pool2d raises: stride should not be zero)")
    return r


def spp_max(x_nhwc, levels):
    """SpoC's spatial pyramid of max-pools (rr_spp_max): x NHWC [B,H,W,C],
    C % 4 == 0 -> pooled [B,R,C], regions in the reference's order (row-major
    per level, the levels one after another; floor-mode windows)."""
    _f32(x_nhwc, "spp_max x")
    if x_nhwc.dim() != 4:
        raise ValueError(f"spp_max: x [B,H,W,C], got {tuple(x_nhwc.shape)}")
    b, h, w, c = x_nhwc.shape
    if c % 4 or c == 0:
        raise ValueError("spp_max: c % 4 == 0, c > 0")
    arr, n = _levels(levels, "spp_max")
    r = spp_regions(h, w, levels)
    dev = _dev(x_nhwc)
    out = torch.empty((b, r, c), dtype=torch.float32, device=x_nhwc.device)
    if b:
        hd = _lib.handle(dev)
        _lib.check(_lib.lib().rr_spp_max(hd, _ptr(x_nhwc), b, h, w, c, ctypes.cast(arr, ctypes.c_void_p), n, _ptr(out),
                                         _stream(dev)), hd, "rr_spp_max")
    return out


def spoc_refine(u, ctx, w_att, b_att, w_c, bias, want_att=False, out=None):
    """SpoC's gated refine (rr_spoc_refine): u [M,C] (or NHWC), the RAW product
    Wx x of feature_refine's input half WITHOUT its bias; ctx [M,DC] (or NHWC),
    the context encoder's output; w_att [DC] and b_att (python float) the
    attention conv; w_c [C,DC] feature_refine's context half, bias [C] ->
    y = sigmoid(ctx . w_att + b_att)[:, None] * u + ctx @ w_c.T + bias, shaped
    as u, and att [M] as a second value with want_att.  out: None (a new
    tensor) or u itself (in place)."""
    _f32(u, "spoc_refine u")
    _f32(ctx, "spoc_refine ctx")
    _f32(w_att, "spoc_refine w_att")
    _f32(w_c, "spoc_refine w_c")
    _f32(bias, "spoc_refine bias")
    if u.dim() < 2 or ctx.dim() < 2:
        raise ValueError(f"spoc_refine: u [M,C] and ctx [M,DC], got {tuple(u.shape)} and {tuple(ctx.shape)}")
    c, dc = u.shape[-1], ctx.shape[-1]
    if dc % 32 or not 32 <= dc <= 2048:
        raise ValueError("spoc_refine: dc % 32 == 0, 32 <= dc <= 2048")
    if c % 4 or c == 0:
        raise ValueError("spoc_refine: c % 4 == 0, c > 0")
    m = u.numel() // c
    if ctx.numel() != m * dc or tuple(ctx.shape[:-1]) != tuple(u.shape[:-1]):
        raise ValueError(f"spoc_refine: ctx must hold u's rows, got {tuple(u.shape)} and {tuple(ctx.shape)}")
    if w_att.numel() != dc or tuple(w_c.shape) != (c, dc) or bias.numel() != c:
        raise ValueError(f"spoc_refine: w_att [{dc}], w_c [{c},{dc}] and bias [{c}], got {tuple(w_att.shape)}, "
                         f"{tuple(w_c.shape)} and {tuple(bias.shape)}")
    if out is not None and out is not u:
        raise ValueError("spoc_refine: out must be None or u itself")
    if any(t.device != u.device for t in (ctx, w_att, w_c, bias)):
        raise ValueError("spoc_refine: every tensor must be on one device")
    dev = _dev(u)
    y = u if out is u else torch.empty_like(u)
    att = torch.empty((m,), dtype=torch.float32, device=u.device) if want_att else None
    if m:
        hd = _lib.handle(dev)
        _lib.check(_lib.lib().rr_spoc_refine(hd, _ptr(u), _ptr(ctx), m, c, dc, _ptr(w_att), float(b_att), _ptr(w_c),
                                             _ptr(bias), _ptr(att), _ptr(y), _stream(dev)), hd, "rr_spoc_refine")
    return (y, att) if want_att else y


def linear_groupmax(x, w, bias, act=0):
    """out[i] = max over image i's rows of act(x[i] @ w.T + bias)
    (rr_linear_groupmax): x [B,R,K] with 1 <= R <= 64 and K % 4 == 0, w [N,K],
    bias [N] or None, act 0 none / 1 ReLU -> [B,N]; the [B,R,N] product never
    reaches memory."""
    _f32(x, "linear_groupmax x")
    _f32(w, "linear_groupmax w")
    if x.dim() != 3 or w.dim() != 2 or w.shape[1] != x.shape[2]:
        raise ValueError(f"linear_groupmax: x [B,R,K] and w [N,K], got {tuple(x.shape)} and {tuple(w.shape)}")
    b, r, k = x.shape
    n = w.shape[0]
    if not 1 <= r <= 64:
        raise ValueError("linear_groupmax: 1 <= r <= 64 rows per image")
    if k % 4 or k == 0 or n == 0:
        raise ValueError("linear_groupmax: k % 4 == 0, k > 0, n > 0")
    if bias is not None and (_f32(bias, "linear_groupmax bias").numel() != n or bias.device != x.device):
        raise ValueError(f"linear_groupmax: bias must be [{n}] on x's device")
    if int(act) not in (0, 1):
        raise ValueError("linear_groupmax: act must be 0 or 1")
    if w.device != x.device:
        raise ValueError("linear_groupmax: x and w must be on one device")
    dev = _dev(x)
    out = torch.empty((b, n), dtype=torch.float32, device=x.device)
    if b:
        hd = _lib.handle(dev)
        _lib.check(_lib.lib().rr_linear_groupmax(hd, _ptr(x), b, r, k, _ptr(w), _ptr(bias), n, int(act), _ptr(out),
                                                 _stream(dev)), hd, "rr_linear_groupmax")
    return out


def se_squeeze(y_nhwc):
    """The SE block's squeeze (rr_se_squeeze): y NHWC [B,H,W,C] (or [B,HW,C]),
    signed, C % 256 == 0 -> the per-channel spatial mean [B,C]."""
    _f32(y_nhwc, "se_squeeze y")
    if y_nhwc.dim() not in (3, 4):
        raise ValueError(f"se_squeeze: y [B,H,W,C] or [B,HW,C], got {tuple(y_nhwc.shape)}")
    b, c = y_nhwc.shape[0], y_nhwc.shape[-1]
    if c % 256 or c == 0:
        raise ValueError("se_squeeze: c % 256 == 0, c > 0")
    hw = 1
    for v in y_nhwc.shape[1:-1]:
        hw *= v
    if hw < 1:
        raise ValueError("se_squeeze: at least one position per image")
    dev = _dev(y_nhwc)
    out = torch.empty((b, c), dtype=torch.float32, device=y_nhwc.device)
    if b:
        hd = _lib.handle(dev)
        _lib.check(_lib.lib().rr_se_squeeze(hd, _ptr(y_nhwc), b, hw, c, _ptr(out), _stream(dev)), hd, "rr_se_squeeze")
    return out


def se_apply(y, hidden, w2, identity=None, relu=True, want_gate=False, out=None, out_amax=None):
    """The SE block's gate, identity add and ReLU (rr_se_apply): y NHWC
    [B,H,W,C] (or [B,HW,C]), hidden [B,CR] = relu(W1 mean), w2 [C,CR] ->
    act(y * sigmoid(hidden @ w2.T)[:, None, :] + identity), shaped as y, and the
    gates [B,C] as a second value with want_gate.  C % 64 == 0, CR % 4 == 0,
    4 <= CR <= 512.  identity: None or a tensor shaped as y.  out: None (a new
    tensor), y or identity (in place).  out_amax: a zeroed record that receives
    max |out| (as conv2d_h2's y_amax)."""
    _f32(y, "se_apply y")
    _f32(hidden, "se_apply hidden")
    _f32(w2, "se_apply w2")
    if y.dim() not in (3, 4) or hidden.dim() != 2 or w2.dim() != 2:
        raise ValueError(f"se_apply: y [B,H,W,C], hidden [B,CR] and w2 [C,CR], got {tuple(y.shape)}, "
                         f"{tuple(hidden.shape)} and {tuple(w2.shape)}")
    b, c = y.shape[0], y.shape[-1]
    cr = hidden.shape[1]
    if c % 64 or c == 0:
        raise ValueError("se_apply: c % 64 == 0, c > 0")
    if cr % 4 or not 4 <= cr <= 512:
        raise ValueError("se_apply: cr % 4 == 0, 4 <= cr <= 512")
    if hidden.shape[0] != b or tuple(w2.shape) != (c, cr):
        raise ValueError(f"se_apply: hidden [{b},{cr}] and w2 [{c},{cr}], got {tuple(hidden.shape)} and "
                         f"{tuple(w2.shape)}")
    hw = 1
    for v in y.shape[1:-1]:
        hw *= v
    if hw < 1:
        raise ValueError("se_apply: at least one position per image")
    if identity is not None and tuple(_f32(identity, "se_apply identity").shape) != tuple(y.shape):
        raise ValueError("se_apply: identity must be shaped as y")
    if out is not None and out is not y and out is not identity:
        raise ValueError("se_apply: out must be None, y or identity")
    if out_amax is not None and (out_amax.dtype != torch.int32 or out_amax.numel() != AMAX_SLOTS or
                                 not out_amax.is_contiguous()):
        raise ValueError("se_apply: out_amax must be a contiguous int32 [RR_AMAX_SLOTS] record")
    if any(t is not None and t.device != y.device for t in (hidden, w2, identity, out_amax)):
        raise ValueError("se_apply: every tensor must be on one device")
    dev = _dev(y)
    o = torch.empty_like(y) if out is None else out
    gate = torch.empty((b, c), dtype=torch.float32, device=y.device) if want_gate else None
    if b:
        hd = _lib.handle(dev)
        _lib.check(_lib.lib().rr_se_apply(hd, _ptr(y), _ptr(hidden), _ptr(w2), _ptr(identity), b, hw, c, cr, int(bool(relu)),
                                          _ptr(gate), _ptr(o), _ptr(out_amax), _stream(dev)), hd, "rr_se_apply")
    return (o, gate) if want_gate else o


def gelu(x, out=None):
    """Exact (erf) GELU (rr_gelu), elementwise; out=x runs in place."""
    _f32(x, "gelu")
    y = torch.empty_like(x) if out is None else out
    if y is not x and (y.dtype != torch.float32 or not y.is_contiguous() or y.numel() != x.numel()):
        raise ValueError("gelu: out must be contiguous float32 of x's size")
    dev = _dev(x)
    hd = _lib.handle(dev)
    _lib.check(_lib.lib().rr_gelu(hd, _ptr(x), x.numel(), _ptr(y), _stream(dev)), hd, "rr_gelu")
    return y


def cosine_topk_workspace_size(nq, n, d, k):
    return int(_lib.lib().rr_cosine_topk_workspace_size(int(nq), int(n), int(d), int(k)))


# ---- bounded ranker workspaces (rr.h "Bounded workspaces") ----------------
# kind -> C functions: worst-case size, size for a cap, cap for a size,
# per-query counts offset, overflow-count offset
_WS_FUNCS = {
    "exact": ("rr_cosine_topk_workspace_size", "rr_cosine_topk_workspace_size_cap", "rr_cosine_topk_cap_for",
              "rr_cosine_topk_counts_offset", "rr_cosine_topk_overflow_offset"),
    "prefilter": ("rr_cosine_topk_prefilter_workspace_size", "rr_cosine_topk_prefilter_workspace_size_cap",
                  "rr_cosine_topk_prefilter_cap_for", "rr_cosine_topk_prefilter_counts_offset",
                  "rr_cosine_topk_prefilter_overflow_offset"),
}


def _wsf(kind, i):
    return getattr(_lib.lib(), _WS_FUNCS[kind][i])


def ranker_workspace_bounds(kind, nq, n, d, k):
    """(minimum bytes = a cap of k candidates per query, worst-case bytes) of
    a ranker workspace; kind 'exact' (cosine_topk / cosine_topk_lp) or
    'prefilter'."""
    a = (int(nq), int(n), int(d), int(k))
    return int(_wsf(kind, 1)(*a, int(k))), int(_wsf(kind, 0)(*a))


def _ranker_workspace(kind, nq, n, d, k, workspace, max_workspace_bytes, device):
    """The workspace a ranker call runs with: the caller's if large enough,
    else a new one of the worst-case size or, with max_workspace_bytes, of at
    most that many bytes (never below the k-candidate minimum).  Returns
    (workspace, bounded)."""
    lo, full = ranker_workspace_bounds(kind, nq, n, d, k)
    budget = full if max_workspace_bytes is None else max(lo, min(full, int(max_workspace_bytes)))
    if workspace is None or workspace.numel() < budget:
        workspace = torch.empty(budget, dtype=torch.uint8, device=device)
    return workspace, workspace.numel() < full


def _recover_overflow(kind, nq, n, d, k, workspace, rerun, os_, oi):
    """After a bounded-workspace call: re-run every query whose candidates
    overflowed the buffer (rr.h) with a worst-case workspace for just those
    queries, in chunks that fit the same workspace, and write their rows.
    rerun(query_index_tensor, workspace) -> (scores, idx).  One device->host
    read of the overflow count (a stream sync); returns the re-run count."""
    a = (int(nq), int(n), int(d), int(k))
    ovf_off = int(_wsf(kind, 4)(*a))
    if int(workspace[ovf_off:ovf_off + 4].view(torch.int32).item()) == 0:
        return 0
    cap = int(_wsf(kind, 2)(*a, workspace.numel()))
    cnt_off = int(_wsf(kind, 3)(*a))
    bad = torch.nonzero(workspace[cnt_off:cnt_off + 4 * int(nq)].view(torch.int32) > cap).flatten()
    c = max(1, bad.numel())
    while c > 1 and int(_wsf(kind, 0)(c, int(n), int(d), int(k))) > workspace.numel():
        c = (c + 1) // 2
    need = int(_wsf(kind, 0)(c, int(n), int(d), int(k)))
    ws = workspace if need <= workspace.numel() else torch.empty(need, dtype=torch.uint8, device=workspace.device)
    for part in bad.split(c):
        s_, i_ = rerun(part, ws)
        os_[part] = s_
        oi[part] = i_
    return int(bad.numel())


def cosine_topk(queries, gallery, k, idx_offset=0, workspace=None, max_workspace_bytes=None):
    """Exact stable top-k of queries [nq,D] against gallery [N,D] -> (scores [nq,k] fp32, idx [nq,k] int64).
    max_workspace_bytes: run with a bounded candidate buffer (rr.h) and re-run
    overflowed queries; results are identical either way."""
    _f32(queries, "cosine_topk queries")
    _f32(gallery, "cosine_topk gallery")
    dev = _dev(queries)
    nq, d = queries.shape
    n = gallery.shape[0]
    if gallery.shape[1] != d:
        raise ValueError("cosine_topk: descriptor dims differ")
    workspace, bounded = _ranker_workspace("exact", nq, n, d, k, workspace, max_workspace_bytes, queries.device)
    os_ = torch.empty((nq, k), dtype=torch.float32, device=queries.device)
    oi = torch.empty((nq, k), dtype=torch.int64, device=queries.device)
    hd = _lib.handle(dev)
    _lib.check(_lib.lib().rr_cosine_topk(hd, _ptr(queries), nq, _ptr(gallery), n, d, k, int(idx_offset), _ptr(os_),
                                         _ptr(oi), _ptr(workspace), workspace.numel(), _stream(dev)), hd,
               "rr_cosine_topk")
    if bounded and nq > 0:
        _recover_overflow("exact", nq, n, d, k, workspace,
                          lambda r, ws: cosine_topk(queries[r].contiguous(), gallery, k, idx_offset, ws), os_, oi)
    return os_, oi


def cosine_scores(queries, gallery):
    """Dense scores, gallery-major [N, nq] (= similarity.T of iris_evaluate.py:383)."""
    _f32(queries, "cosine_scores queries")
    _f32(gallery, "cosine_scores gallery")
    dev = _dev(queries)
    nq, d = queries.shape
    n = gallery.shape[0]
    out = torch.empty((n, nq), dtype=torch.float32, device=queries.device)
    hd = _lib.handle(dev)
    _lib.check(_lib.lib().rr_cosine_scores(hd, _ptr(queries), nq, _ptr(gallery), n, d, _ptr(out), _stream(dev)), hd,
               "rr_cosine_scores")
    return out


def topk_merge(part_scores, part_idx, k_out):
    """[P,nq,kin] partial lists -> stable top-k_out per query."""
    _f32(part_scores, "topk_merge scores")
    if part_idx.dtype != torch.int64 or not part_idx.is_contiguous():
        raise TypeError("topk_merge: idx must be contiguous int64")
    dev = _dev(part_scores)
    p, nq, kin = part_scores.shape
    os_ = torch.empty((nq, k_out), dtype=torch.float32, device=part_scores.device)
    oi = torch.empty((nq, k_out), dtype=torch.int64, device=part_scores.device)
    hd = _lib.handle(dev)
    _lib.check(_lib.lib().rr_topk_merge(hd, _ptr(part_scores), _ptr(part_idx), p, nq, kin, k_out, _ptr(os_), _ptr(oi),
                                        _stream(dev)), hd, "rr_topk_merge")
    return os_, oi


_TUNE_KEYS = {name: key for name, (key, _) in _lib.TUNING.items()}
_TUNE_DEFAULT = {name: default for name, (_, default) in _lib.TUNING.items()}  # the library's own pick


class tuning:
    """Force kernel tile configs on a device's handle for the duration of a
    ``with`` block (rr_set_tuning; tests and tuning tools only):
    ``with ops.tuning(0, s3_cfg=6): ...``.  Values revert to the library's
    own pick on exit."""

    def __init__(self, device_index, **kw):
        for k in kw:
            if k not in _TUNE_KEYS:
                raise ValueError(f"unknown tuning key {k!r}")
        self.h = _lib.handle(device_index)
        self.kw = kw

    def __enter__(self):
        for k, v in self.kw.items():
            _lib.check(_lib.lib().rr_set_tuning(self.h, _TUNE_KEYS[k], int(v)), self.h, "rr_set_tuning")
        return self

    def __exit__(self, *exc):
        for k in self.kw:
            _lib.lib().rr_set_tuning(self.h, _TUNE_KEYS[k], _TUNE_DEFAULT[k])
        return False


class KernelTimer:
    """HIP-event timing of librr kernel classes on their launch stream."""

    def __init__(self, device_index):
        self.h = _lib.handle(device_index)

    def enable(self, on=True):
        _lib.check(_lib.lib().rr_timing_enable(self.h, int(on)), self.h, "rr_timing_enable")

    def collect(self, cls):
        ms = ctypes.c_double()
        n = ctypes.c_longlong()
        _lib.check(_lib.lib().rr_timing_collect(self.h, cls, ctypes.byref(ms), ctypes.byref(n)), self.h,
                   "rr_timing_collect")
        return ms.value, n.value

    def collect_ex(self, cls):
        """(union ms, sum of the per-launch ms, launches): rr_timing_collect_ex.
        collect() returns the union; the two differ where launches co-ran."""
        uni, tot = ctypes.c_double(), ctypes.c_double()
        n = ctypes.c_longlong()
        _lib.check(_lib.lib().rr_timing_collect_ex(self.h, cls, ctypes.byref(uni), ctypes.byref(tot), ctypes.byref(n)),
                   self.h, "rr_timing_collect_ex")
        return uni.value, tot.value, n.value


def linear_ex(x, w, bias=None, residual=None, act=0):
    """y = act(x @ w.T + bias + residual); act 0 none, 1 ReLU, 2 QuickGELU."""
    _f32(x, "linear_ex x")
    _f32(w, "linear_ex w")
    dev = _dev(x)
    m, k = x.shape
    n = w.shape[0]
    y = torch.empty((m, n), dtype=torch.float32, device=x.device)
    if residual is not None:
        _f32(residual, "linear_ex residual")
        if tuple(residual.shape) != (m, n):
            raise ValueError("linear_ex: residual shape mismatch")
    hd = _lib.handle(dev)
    _lib.check(_lib.lib().rr_linear_ex(hd, _ptr(x), m, k, _ptr(w), _ptr(bias), n, _ptr(residual), int(act), _ptr(y),
                                       _stream(dev)), hd, "rr_linear_ex")
    return y


def layernorm(x, gamma, beta, eps=1e-5, rows=None, row_stride=None):
    """LayerNorm over the last dim of x [..., D]; with rows/row_stride, LN of
    ``rows`` rows spaced ``row_stride`` floats apart (e.g. the CLS tokens)."""
    _f32(x, "layernorm")
    dev = _dev(x)
    d = x.shape[-1]
    m = x.numel() // d if rows is None else int(rows)
    ld = d if row_stride is None else int(row_stride)
    y = torch.empty((m, d), dtype=torch.float32, device=x.device)
    hd = _lib.handle(dev)
    _lib.check(_lib.lib().rr_layernorm(hd, _ptr(x), ld, m, d, _ptr(gamma), _ptr(beta), float(eps), _ptr(y),
                                       _stream(dev)), hd, "rr_layernorm")
    return y


def patchify(x_nhwc, patch, out_bf16=False):
    """NHWC image -> patch rows (fp32, or bf16 RNE for the bf16 patch GEMM)."""
    _f32(x_nhwc, "patchify")
    dev = _dev(x_nhwc)
    b, h, w, c = x_nhwc.shape
    y = torch.empty((b * (h // patch) * (w // patch), patch * patch * c),
                    dtype=torch.bfloat16 if out_bf16 else torch.float32, device=x_nhwc.device)
    hd = _lib.handle(dev)
    _lib.check(_lib.lib().rr_patchify_ex(hd, _ptr(x_nhwc), b, h, w, c, patch, int(out_bf16), _ptr(y), _stream(dev)),
               hd, "rr_patchify_ex")
    return y


def vit_tokens(patches, b, cls, pos, ln=None, eps=1e-5):
    """[cls; patches] + pos per image; with ln = (gamma, beta), ln_pre fused."""
    _f32(patches, "vit_tokens")
    dev = _dev(patches)
    width = patches.shape[1]
    npatch = patches.shape[0] // b
    y = torch.empty((b * (npatch + 1), width), dtype=torch.float32, device=patches.device)
    hd = _lib.handle(dev)
    gamma, beta = ln if ln is not None else (None, None)
    _lib.check(_lib.lib().rr_vit_tokens_ex(hd, _ptr(patches), b, npatch, width, _ptr(cls), _ptr(pos), _ptr(gamma),
                                           _ptr(beta), float(eps), _ptr(y), _stream(dev)), hd, "rr_vit_tokens_ex")
    return y


def attention(qkv, b, seq, heads, head_dim=64):
    _f32(qkv, "attention")
    dev = _dev(qkv)
    out = torch.empty((b * seq, heads * head_dim), dtype=torch.float32, device=qkv.device)
    hd = _lib.handle(dev)
    _lib.check(_lib.lib().rr_attention(hd, _ptr(qkv), b, seq, heads, head_dim, _ptr(out), _stream(dev)), hd,
               "rr_attention")
    return out


# ---- low precision (C4 bf16 / C5 fp8) --------------------------------------
DT_BF16, DT_FP8 = 1, 2
_LP = {"bf16": DT_BF16, "fp8": DT_FP8}


def quantize_rows(x, dtype):
    """fp32 [rows, d] -> (bf16 tensor, None) or (fp8-e4m3 bytes as uint8, per-row fp32 scales)."""
    _f32(x, "quantize_rows")
    dev = _dev(x)
    dt = _LP[dtype]
    rows, d = x.shape
    if dt == DT_BF16:
        y = torch.empty((rows, d), dtype=torch.bfloat16, device=x.device)
        sc = None
    else:
        y = torch.empty((rows, d), dtype=torch.uint8, device=x.device)
        sc = torch.empty(rows, dtype=torch.float32, device=x.device)
    hd = _lib.handle(dev)
    _lib.check(_lib.lib().rr_quantize_rows(hd, _ptr(x), rows, d, dt, _ptr(y), _ptr(sc), _stream(dev)), hd,
               "rr_quantize_rows")
    return y, sc


def _lp_rows(t, sc, dtype, name):
    """Validate quantised rows as quantize_rows makes them: bf16 [rows, d]
    (no scales) or fp8-e4m3 bytes uint8 [rows, d] + fp32 scales [rows]."""
    if t.dim() != 2 or not t.is_contiguous():
        raise ValueError(f"{name}: expected contiguous [rows, d]")
    if dtype == "bf16":
        if t.dtype != torch.bfloat16:
            raise TypeError(f"{name}: bf16 rows must be torch.bfloat16, got {t.dtype}")
    else:
        if t.dtype not in (torch.uint8, torch.float8_e4m3fn):
            raise TypeError(f"{name}: fp8 rows must be uint8 (e4m3 bytes), got {t.dtype}")
        if sc is None or sc.dtype != torch.float32 or not sc.is_contiguous() or sc.numel() != t.shape[0]:
            raise ValueError(f"{name}: fp8 rows need contiguous fp32 scales, one per row")


def cosine_topk_lp(q, q_scale, g, g_scale, k, dtype, idx_offset=0, workspace=None, max_workspace_bytes=None):
    """Fused top-k on bf16 / fp8 rows (fp32 accumulate); scores dequantised.
    max_workspace_bytes: bounded candidate buffer, as in cosine_topk."""
    if dtype not in _LP:
        raise ValueError("cosine_topk_lp: dtype must be 'bf16' or 'fp8'")
    _lp_rows(q, q_scale, dtype, "cosine_topk_lp queries")
    _lp_rows(g, g_scale, dtype, "cosine_topk_lp gallery")
    if q.shape[1] != g.shape[1]:
        raise ValueError("cosine_topk_lp: descriptor dims differ")
    dev = _dev(q)
    dt = _LP[dtype]
    nq, d = q.shape
    n = g.shape[0]
    workspace, bounded = _ranker_workspace("exact", nq, n, d, k, workspace, max_workspace_bytes, q.device)
    os_ = torch.empty((nq, k), dtype=torch.float32, device=q.device)
    oi = torch.empty((nq, k), dtype=torch.int64, device=q.device)
    hd = _lib.handle(dev)
    _lib.check(_lib.lib().rr_cosine_topk_lp(hd, _ptr(q), _ptr(q_scale), nq, _ptr(g), _ptr(g_scale), n, d, dt, k,
                                            int(idx_offset), _ptr(os_), _ptr(oi), _ptr(workspace), workspace.numel(),
                                            _stream(dev)), hd, "rr_cosine_topk_lp")
    if bounded and nq > 0:
        _recover_overflow("exact", nq, n, d, k, workspace,
                          lambda r, ws: cosine_topk_lp(q[r].contiguous(), None if q_scale is None else
                                                       q_scale[r].contiguous(), g, g_scale, k, dtype, idx_offset, ws),
                          os_, oi)
    return os_, oi


def linear_bf16(x, w, bias=None, residual=None, act=0, out_bf16=False):
    """bf16 x [M,K] . bf16 w [N,K]^T -> fp32 (or bf16) with fused epilogue."""
    if x.dtype != torch.bfloat16 or w.dtype != torch.bfloat16:
        raise TypeError("linear_bf16: x and w must be bfloat16")
    if x.dim() != 2 or w.dim() != 2 or not x.is_contiguous() or not w.is_contiguous() or x.shape[1] != w.shape[1]:
        raise ValueError("linear_bf16: contiguous x [M,K] and w [N,K] with matching K")
    dev = _dev(x)
    m, k = x.shape
    n = w.shape[0]
    if bias is not None and (_f32(bias, "linear_bf16 bias").numel() != n):
        raise ValueError("linear_bf16: bias must have N entries")
    if residual is not None and tuple(_f32(residual, "linear_bf16 residual").shape) != (m, n):
        raise ValueError("linear_bf16: residual shape mismatch")
    y = torch.empty((m, n), dtype=torch.bfloat16 if out_bf16 else torch.float32, device=x.device)
    hd = _lib.handle(dev)
    _lib.check(_lib.lib().rr_linear_bf16(hd, _ptr(x), m, k, _ptr(w), _ptr(bias), n, _ptr(residual), int(act),
                                         int(out_bf16), _ptr(y), _stream(dev)), hd, "rr_linear_bf16")
    return y


def linear_bf16_ln_produce(x, w, bias, residual):
    """The residual GEMM of a ViT block with the next LayerNorm's inputs
    produced in its epilogue (rr_linear_bf16_ln, stats_out): returns (y fp32
    [M,N] = x.w^T + bias + residual, bf16(y - mean_t) with mean_t the mean of
    the row's 256-column tile, the per-row tile LayerNorm partials
    [M, N/256, 2] = (mean_t, M2_t))."""
    if x.dtype != torch.bfloat16 or w.dtype != torch.bfloat16:
        raise TypeError("linear_bf16_ln_produce: x and w must be bfloat16")
    if x.dim() != 2 or w.dim() != 2 or not x.is_contiguous() or not w.is_contiguous() or x.shape[1] != w.shape[1]:
        raise ValueError("linear_bf16_ln_produce: contiguous x [M,K] and w [N,K] with matching K")
    dev = _dev(x)
    m, k = x.shape
    n = w.shape[0]
    if n % 256:
        raise ValueError("linear_bf16_ln_produce: N % 256 == 0")
    if _f32(bias, "bias").numel() != n or tuple(_f32(residual, "residual").shape) != (m, n):
        raise ValueError("linear_bf16_ln_produce: bias [N] and residual [M,N]")
    y = torch.empty((m, n), dtype=torch.float32, device=x.device)
    yb = torch.empty((m, n), dtype=torch.bfloat16, device=x.device)
    st = torch.empty((m, n // 256, 2), dtype=torch.float32, device=x.device)
    hd = _lib.handle(dev)
    _lib.check(_lib.lib().rr_linear_bf16_ln(hd, _ptr(x), m, k, _ptr(w), _ptr(bias), n, _ptr(residual), 0, 0, _ptr(y),
                                            None, None, 0.0, _ptr(st), _ptr(yb), _stream(dev)), hd, "rr_linear_bf16_ln")
    return y, yb, st


# widest K the fold's consumer serves: rr_linear_bf16_ln stages LN_TMAX = 3
# column-sum tiles of 256 (csrc/gemm_epilogue.hpp; rr.h: stats_in needs k <= 768)
LN_FOLD_MAX_K = 768


def ln_fold_supported(width, dtype):
    """Whether the ViT LayerNorm fold (rr_linear_bf16_ln) serves a width:
    bf16, 256-column tiles, and K = width within the consumer's limit."""
    return dtype == "bf16" and width % 256 == 0 and width <= LN_FOLD_MAX_K


def linear_bf16_ln_fold(xb, stats, w_folded, colsum, bias_folded, act=0, eps=1e-5):
    """act(LayerNorm(x) . W^T + b) -> bf16 with the LayerNorm folded into the
    GEMM (rr_linear_bf16_ln, stats_in): xb = the tile-centred bf16 rows of x
    and their partials (linear_bf16_ln_produce / ln_partials_bf16), w_folded =
    bf16(W o gamma), colsum = its fp32 row sums per 256-deep k tile
    [ceil(K/256), N], bias_folded = b + W beta (ln_fold_weights); K <= 768."""
    if xb.dtype != torch.bfloat16 or w_folded.dtype != torch.bfloat16:
        raise TypeError("linear_bf16_ln_fold: xb and w_folded must be bfloat16")
    dev = _dev(xb)
    m, k = xb.shape
    n = w_folded.shape[0]
    t = (k + 255) // 256
    if tuple(stats.shape) != (m, t, 2) or w_folded.shape[1] != k or tuple(colsum.shape) != (t, n):
        raise ValueError("linear_bf16_ln_fold: stats [M, ceil(K/256), 2], w_folded [N, K], colsum [ceil(K/256), N]")
    y = torch.empty((m, n), dtype=torch.bfloat16, device=xb.device)
    hd = _lib.handle(dev)
    _lib.check(_lib.lib().rr_linear_bf16_ln(hd, _ptr(xb), m, k, _ptr(w_folded), _ptr(bias_folded), n, None, int(act),
                                            1, _ptr(y), _ptr(stats), _ptr(colsum), float(eps), None, None,
                                            _stream(dev)), hd, "rr_linear_bf16_ln")
    return y


def ln_partials_bf16(x):
    """(bf16(x - mean_t), the LayerNorm partials [M, D/256, 2]) of fp32 rows x
    [M, D], each 256-column tile t centred on its own mean mean_t
    (rr_ln_partials_bf16): the first block's ln_1 input, which no GEMM wrote."""
    _f32(x, "ln_partials_bf16")
    dev = _dev(x)
    d = x.shape[-1]
    m = x.numel() // d
    xb = torch.empty((m, d), dtype=torch.bfloat16, device=x.device)
    st = torch.empty((m, d // 256, 2), dtype=torch.float32, device=x.device)
    hd = _lib.handle(dev)
    _lib.check(_lib.lib().rr_ln_partials_bf16(hd, _ptr(x), m, d, _ptr(xb), _ptr(st), _stream(dev)), hd,
               "rr_ln_partials_bf16")
    return xb, st


def ln_fold_weights(w, b, gamma, beta):
    """Fold a LayerNorm (gamma, beta) into the following linear (w [N,K] fp32,
    b [N]): (bf16(w o gamma), the fp32 row sums of that bf16 matrix per
    256-deep k tile [ceil(K/256), N], b + w beta)."""
    wf = (w.float() * gamma.float()[None, :]).to(torch.bfloat16).contiguous()
    n, k = wf.shape
    t = (k + 255) // 256
    colsum = torch.nn.functional.pad(wf.float(), (0, 256 * t - k)).view(n, t, 256).sum(dim=2).t().contiguous()
    bf = (b.double() + w.double() @ beta.double()).float().contiguous()
    return wf, colsum, bf


def layernorm_bf16(x, gamma, beta, eps=1e-5):
    _f32(x, "layernorm_bf16")
    dev = _dev(x)
    d = x.shape[-1]
    m = x.numel() // d
    y = torch.empty((m, d), dtype=torch.bfloat16, device=x.device)
    hd = _lib.handle(dev)
    _lib.check(_lib.lib().rr_layernorm_ex(hd, _ptr(x), d, m, d, _ptr(gamma), _ptr(beta), float(eps), 1, _ptr(y),
                                          _stream(dev)), hd, "rr_layernorm_ex")
    return y


def attention_bf16(qkv, b, seq, heads, head_dim=64, bf16_math=True):
    """Attention core for the bf16 ViT: bf16 output; bf16 MFMA with fp32
    softmax (rr_attention_bf16; bf16 qkv rows: rr_attention_bf16_qkv16), or
    fp32 MFMA (bf16_math=False, fp32 qkv)."""
    dev = _dev(qkv)
    if qkv.dtype == torch.bfloat16 and bf16_math:
        if not qkv.is_contiguous():
            raise ValueError("attention_bf16: qkv must be contiguous")
        fn = _lib.lib().rr_attention_bf16_qkv16
    else:
        _f32(qkv, "attention_bf16")
        fn = _lib.lib().rr_attention_bf16 if bf16_math else _lib.lib().rr_attention_ex
    out = torch.empty((b * seq, heads * head_dim), dtype=torch.bfloat16, device=qkv.device)
    hd = _lib.handle(dev)
    _lib.check(fn(hd, _ptr(qkv), b, seq, heads, head_dim, 1, _ptr(out), _stream(dev)), hd, "rr_attention_bf16")
    return out


def alpha_qe(queries, gallery, top_idx, top_scores, n=2, alpha=3.0, idx_offset=0):
    """alpha-QE new queries (see include/rr.h rr_alpha_qe)."""
    _f32(queries, "alpha_qe queries")
    _f32(gallery, "alpha_qe gallery")
    dev = _dev(queries)
    nq, d = queries.shape
    k = top_idx.shape[1]
    out = torch.empty_like(queries)
    hd = _lib.handle(dev)
    if gallery.shape[1] != d or top_idx.dtype != torch.int64 or top_scores.dtype != torch.float32:
        raise TypeError("alpha_qe: gallery [N, d] fp32, top_idx int64, top_scores fp32")
    _lib.check(_lib.lib().rr_alpha_qe(hd, _ptr(queries), nq, _ptr(gallery), gallery.shape[0], d,
                                      _ptr(top_idx.contiguous()),
                                      _ptr(top_scores.contiguous()), k, int(n), float(alpha), int(idx_offset),
                                      _ptr(out), _stream(dev)), hd, "rr_alpha_qe")
    return out


def pcaw_gram(x):
    """Column mean and centred Gram sum_i (x_i - m)(x_i - m)^T of fp32 rows
    x [n, d] on the device (include/rr.h rr_pcaw_gram) -> (mean fp64 [d],
    gram fp64 [d, d])."""
    _f32(x, "pcaw_gram")
    dev = _dev(x)
    n, d = x.shape
    if n == 0:
        raise ValueError("pcaw_gram: empty descriptor set")
    L = _lib.lib()
    ws = torch.empty(L.rr_pcaw_gram_workspace_size(n, d), dtype=torch.uint8, device=dev)
    mean = torch.empty(d, dtype=torch.float64, device=dev)
    gram = torch.empty((d, d), dtype=torch.float64, device=dev)
    hd = _lib.handle(dev)
    _lib.check(L.rr_pcaw_gram(hd, _ptr(x), n, d, _ptr(ws), ws.numel(), _ptr(mean), _ptr(gram), _stream(dev)),
               hd, "rr_pcaw_gram")
    return mean, gram


def prefilter_gallery_bound(gallery, gallery_bf16):
    """Row-norm maxima (|g|, |g - bf16(g)|, |bf16(g)|) as fp64 [3] on the device."""
    _f32(gallery, "prefilter_gallery_bound")
    dev = _dev(gallery)
    n, d = gallery.shape
    out = torch.empty(3, dtype=torch.float64, device=gallery.device)
    hd = _lib.handle(dev)
    _lib.check(_lib.lib().rr_prefilter_gallery_bound(hd, _ptr(gallery), _ptr(gallery_bf16), n, d, _ptr(out),
                                                     _stream(dev)), hd, "rr_prefilter_gallery_bound")
    return out


def cosine_topk_prefilter_workspace_size(nq, n, d, k):
    return int(_lib.lib().rr_cosine_topk_prefilter_workspace_size(nq, n, d, k))


def prefilter_survivors(workspace, nq, n, d, k):
    """Per-query count of rows that passed the bf16 filter in the last
    cosine_topk_prefilter call on this workspace (int32 [nq], device)."""
    off = int(_lib.lib().rr_cosine_topk_prefilter_counts_offset(int(nq), int(n), int(d), int(k)))
    return workspace[off:off + 4 * int(nq)].view(torch.int32)


def cosine_topk_prefilter(q, g, g_bf16, bound3, k, idx_offset=0, workspace=None, max_workspace_bytes=None):
    """Exact top-k (bit-identical to cosine_topk) via the bf16 prefilter.
    max_workspace_bytes: bounded candidate buffer + re-run of overflowed
    queries, as in cosine_topk."""
    _f32(q, "cosine_topk_prefilter q")
    _f32(g, "cosine_topk_prefilter g")
    dev = _dev(q)
    nq, d = q.shape
    n = g.shape[0]
    workspace, bounded = _ranker_workspace("prefilter", nq, n, d, k, workspace, max_workspace_bytes, q.device)
    s = torch.empty((nq, k), dtype=torch.float32, device=q.device)
    i = torch.empty((nq, k), dtype=torch.int64, device=q.device)
    hd = _lib.handle(dev)
    _lib.check(_lib.lib().rr_cosine_topk_prefilter(hd, _ptr(q), nq, _ptr(g), _ptr(g_bf16), _ptr(bound3), n, d, k,
                                                   int(idx_offset), _ptr(s), _ptr(i), _ptr(workspace),
                                                   workspace.numel(), _stream(dev)), hd, "rr_cosine_topk_prefilter")
    if bounded and nq > 0:
        _recover_overflow("prefilter", nq, n, d, k, workspace,
                          lambda r, ws: cosine_topk_prefilter(q[r].contiguous(), g, g_bf16, bound3, k, idx_offset, ws),
                          s, i)
    return s, i
