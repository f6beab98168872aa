"""Plain-torch restatement of the SpoC head (models/spoc.py:12-195), a test
helper.  head_forward writes the reference's own sequence, LITERALLY, on the
folded weights of weights.spoc_head_from_state_dict, in NCHW and in any dtype:
the two 3x3 convs with ReLU, the 1x1 attention conv and the sigmoid, x * a, the
cat, the 1x1 refine conv over the concatenation (:76-94), one F.max_pool2d per
level with kernel = stride = (H // L, W // L), view and cat (:20-49), Conv1d(1)
+ ReLU + max over the regions (:131-136, the BatchNorm1d folded), feature_proj
(:139-144) and F.normalize (:194).  It is independent of the identity the
kernels use (refined_p = a_p (Wx x_p) + Wc ctx_p + b, no concatenation).
tests/test_spoc_host.py pins it to the reference's own output
(tests/golden/spoc.npz), so the GPU tests may use it at other shapes and in
float64.
"""
import torch
import torch.nn.functional as F


def regions(h, w, levels):
    """Regions of the pyramid on an h x w map, or ValueError where the reference raises."""
    r = 0
    for lv in levels:
        if lv < 1 or lv > h or lv > w:
            raise ValueError("stride should not be zero")
        r += (h // (h // lv)) * (w // (w // lv))
    return r


def spp(x, levels, ceil_mode=False):
    """SpatialPyramidPooling.forward (:20-49), pool_type 'max': x [B,C,H,W] ->
    [B,C,R].  ceil_mode=True is the sensitivity tests' wrong window rule."""
    b, c, h, w = x.shape
    parts = []
    for lv in levels:
        k = (h // lv, w // lv)
        parts.append(F.max_pool2d(x, kernel_size=k, stride=k, ceil_mode=ceil_mode).reshape(b, c, -1))
    return torch.cat(parts, dim=2)


def head_forward(x4, head, dtype=torch.float64, levels=(1, 2, 4), gate=True, ctx_half=True, ceil_mode=False,
                 agg="max", relu=True, pad_rows=False):
    """Everything after the trunk on x4 [B,Cin,H,W] (NCHW), literal form: dict(att
    [B,N] (absent without the context head), refined [B,H,W,C], pooled [B,R,C],
    agg [B,F], hidden, features, out [B,F]).  The switches each disable one
    piece (the sensitivity tests): gate=False (a = 1), ctx_half=False (the
    context half of the refine conv dropped), ceil_mode=True, agg="mean" (the
    max over regions replaced by their mean), relu=False (no ReLU in the
    aggregation), pad_rows=True (zero rows up to 64 admitted to the max, as a
    64-row tile would without its mask)."""
    b, cin, h, w = x4.shape
    x = x4.to(dtype)
    d = lambda k: head[k].to(dtype)  # noqa: E731
    got = {}
    refined = x
    if "ce0_w" in head:
        ctx = F.relu(F.conv2d(x, d("ce0_w").permute(0, 3, 1, 2), d("ce0_b"), padding=1))
        ctx = F.relu(F.conv2d(ctx, d("ce1_w").permute(0, 3, 1, 2), d("ce1_b"), padding=1))     # :80
        dc = ctx.shape[1]
        a = torch.sigmoid(F.conv2d(ctx, d("att_w").reshape(1, dc, 1, 1)) + head["att_b"])     # :83
        got["att"] = a.reshape(b, h * w)
        if not gate:
            a = torch.ones_like(a)
        combined = torch.cat([x * a, ctx if ctx_half else torch.zeros_like(ctx)], dim=1)       # :86-89
        wr = torch.cat([d("refine_wx").reshape(-1, cin), d("refine_wc")], dim=1)
        refined = F.conv2d(combined, wr.reshape(wr.shape[0], cin + dc, 1, 1), d("refine_b"))   # :92
    got["refined"] = refined.permute(0, 2, 3, 1).contiguous()
    pooled = spp(refined, levels, ceil_mode)                                                   # :164
    got["pooled"] = pooled.transpose(1, 2).contiguous()
    if pad_rows:
        pooled = torch.cat([pooled, torch.zeros(b, pooled.shape[1], 64 - pooled.shape[2], dtype=dtype)], dim=2)
    y = F.conv1d(pooled, d("agg_w").unsqueeze(2), d("agg_b"))                                  # :132-133
    y = F.relu(y) if relu else y
    got["agg"] = y.amax(dim=2) if agg == "max" else y.mean(dim=2)                              # :135
    got["hidden"] = F.relu(F.linear(got["agg"], d("fp0_w"), d("fp0_b")))
    got["features"] = F.linear(got["hidden"], d("fp3_w"), d("fp3_b"))
    got["out"] = F.normalize(got["features"], p=2, dim=1)
    return got
