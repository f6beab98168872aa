"""Plain-torch restatement of the SOLAR head (networks/RetrievalNet.py:534-590),
a test helper.  It writes the reference's own sequence (the three 1x1 convs,
ReLU, two bmm around a softmax, v, + x, gem, normalize, whiten, normalize) on
the folded weight format of weights.solar_head_from_state_dict, in any dtype.
tests/test_solar_host.py pins it to the reference's own output
(tests/golden/solar.npz), so the GPU tests may use it at other shapes and in
float64.
"""
import torch
import torch.nn.functional as F


def attention(fgh, c, dtype=torch.float64, uniform=False):
    """SOABlock_GeM.forward :558-564 from the fused conv's output fgh [B,N,3c]
    ([f | g | h], f and g pre-ReLU): (attn [B,N,N], attn . h^T [B,N,c]).
    uniform=True replaces the softmax by 1/N (the sensitivity tests)."""
    fgh = fgh.to(dtype)
    f_x = F.relu(fgh[..., :c]).permute(0, 2, 1)           # B * mid_ch * N, as the reference's views
    g_x = F.relu(fgh[..., c:2 * c]).permute(0, 2, 1)
    h_x = fgh[..., 2 * c:].permute(0, 2, 1)
    z = torch.bmm(f_x.permute(0, 2, 1), g_x)
    # the Python float c ** -.5 times a tensor: torch rounds the scalar to the tensor's dtype
    attn = F.softmax((c ** -.50) * z, dim=-1)
    if uniform:
        attn = torch.full_like(attn, 1.0 / attn.shape[-1])
    return attn, torch.bmm(attn, h_x.permute(0, 2, 1))


def block(x4, head, dtype=torch.float64, uniform=False, zero_v=False):
    """SOABlock_GeM on x4 [B,Cin,H,W] (NCHW) with folded weights `head`:
    dict(att [B,N,N], ah [B,N,c], pooled [B,Cin])."""
    t = lambda a: a.to(dtype)  # noqa: E731
    b, cin, h, w = x4.shape
    c = head["fgh_w"].shape[0] // 3
    x = t(x4).permute(0, 2, 3, 1).reshape(b, h * w, cin)
    fgh = x @ t(head["fgh_w"]).reshape(3 * c, cin).t() + t(head["fgh_b"])
    att, ah = attention(fgh, c, dtype, uniform)
    v_w, v_b = t(head["v_w"]).reshape(cin, c), t(head["v_b"])
    if zero_v:
        v_w, v_b = torch.zeros_like(v_w), torch.zeros_like(v_b)
    z = (ah @ v_w.t() + v_b + x).permute(0, 2, 1).reshape(b, cin, h, w)
    pooled = F.avg_pool2d(z.clamp(min=1e-6).pow(3.0), (h, w)).pow(1.0 / 3.0).flatten(1)
    return {"att": att, "ah": ah, "pooled": pooled}


def tail(pooled, head):
    """SOLAR.forward_test :587-590."""
    f = F.normalize(pooled, p=2.0, dim=1)
    f = F.linear(f, head["whiten_w"].to(f.dtype), head["whiten_b"].to(f.dtype))
    return F.normalize(f, dim=-1)


def head_forward(x4, head, dtype=torch.float64, uniform=False, zero_v=False):
    """Everything after the trunk: dict(out [B,2048], pooled, att, ah)."""
    got = block(x4, head, dtype, uniform, zero_v)
    got["out"] = tail(got["pooled"], head)
    return got
