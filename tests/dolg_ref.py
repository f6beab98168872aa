"""Plain-torch restatement of the DOLG head (networks/RetrievalNet.py:409-474,
with_aspp=False), a test helper.  It writes out the reference's PER-PIXEL
sequence (normalise, ReLU, conv2, softplus, expand-multiply, the two bmm, the
division, the subtraction, the average pool), not the linearised form the
kernels use, and takes the folded weight format of
weights.dolg_head_from_state_dict.  tests/test_dolg_host.py pins it to the
reference's own output (tests/golden/dolg.npz), so the GPU tests may use it
at other shapes and in float64.
"""
import torch
import torch.nn.functional as F


def local_map(y, w2, b2):
    """SpatialAttention2d after the BN (:466-474): y [B,HW,C] (conv1+BN output,
    pre-ReLU) -> (fl [B,HW,C], att [B,HW])."""
    fmn = F.normalize(y, p=2, dim=2)                      # eps 1e-12 on the norm
    logit = F.relu(y) @ w2.to(y.dtype) + b2
    att = F.softplus(logit, beta=1, threshold=20)
    return att.unsqueeze(2).expand_as(fmn) * fmn, att


def local_pool(y, w2, b2, dtype=torch.float64):
    """m [B,C] = mean over pixels of the local map, in `dtype`."""
    fl, _ = local_map(y.to(dtype), w2, float(b2))
    return fl.mean(dim=1)


def orth_pool(fg, fl):
    """DOLG.forward_test :418-426: fg [B,C], fl [B,HW,C] -> fo [B,C]."""
    flc = fl.transpose(1, 2)                              # [B,C,HW], the reference's flatten(fl, 2)
    fg_norm = torch.norm(fg, p=2, dim=1)
    proj = torch.bmm(fg.unsqueeze(1), flc)
    proj = torch.bmm(fg.unsqueeze(2), proj)
    proj = proj / (fg_norm * fg_norm).view(-1, 1, 1)
    return (flc - proj).mean(dim=2)


def tail(fg, fo, head):
    """:428-431: F.normalize(fc(cat(fg, fo)))."""
    f = F.linear(torch.cat((fg, fo), 1), head["fc_w"].to(fg.dtype), head["fc_b"].to(fg.dtype))
    return F.normalize(f, dim=-1)


def head_forward(x3, x4, head, dtype=torch.float32):
    """The whole head on trunk outputs x3 [B,1024,h,w], x4 [B,2048,h',w'] (NCHW)
    with folded weights `head`; returns dict(out, fg, fo, m, att)."""
    t = lambda a: a.to(dtype)  # noqa: E731
    b, c, h, w = x3.shape
    xr = t(x3).permute(0, 2, 3, 1).reshape(b, h * w, c)
    y = xr @ t(head["conv1_w"]).reshape(-1, c).t() + t(head["conv1_b"])
    fl, att = local_map(y, head["conv2_w"], head["conv2_b"])
    x4 = t(x4)
    g = F.avg_pool2d(x4.clamp(min=1e-6).pow(3.0), (x4.size(-2), x4.size(-1))).pow(1.0 / 3.0).flatten(1)
    fg = F.linear(g, t(head["fc_t_w"]), t(head["fc_t_b"]))
    fo = orth_pool(fg, fl)
    return {"out": tail(fg, fo, head), "fg": fg, "fo": fo, "m": fl.mean(dim=1), "att": att.reshape(b, h, w)}
