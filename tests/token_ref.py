"""Plain-torch restatement of the Token head (networks/RetrievalNet.py:94-187
and forward_test's F.normalize, :300-305), a test helper.  It writes the
reference's own sequence on the folded weight format of
weights.token_head_from_state_dict, in any dtype.  tests/test_token_host.py
pins it to the reference's own output (tests/golden/token.npz), so the GPU tests
may use it at other shapes and in float64.

Each switch replaces one piece by a degenerate one (the sensitivity tests):
enc_uniform, cross_uniform, self_uniform (that attention's softmax -> 1/nk),
slot_uniform (the slot softmax -> 1/n_obj), quick_gelu (erf-GELU -> x
sigmoid(1.702 x)).
"""
import torch
import torch.nn.functional as F

HEADS = 8


def mha(q, k, v, heads=HEADS, uniform=False):
    """Attention.forward :118-124 after the projections: q [B,Nq,D], k and v
    [B,Nk,D] -> [B,Nq,D]."""
    b, nq, d = q.shape
    nk = k.shape[1]
    hd = d // heads
    qh = q.reshape(b, nq, heads, hd).permute(0, 2, 1, 3)
    kh = k.reshape(b, nk, heads, hd).permute(0, 2, 1, 3)
    vh = v.reshape(b, nk, heads, hd).permute(0, 2, 1, 3)
    # the Python float hd ** -0.5 times a tensor: torch rounds the scalar to the tensor's dtype
    attn = F.softmax((qh @ kh.transpose(-2, -1)) * (hd ** -0.5), dim=-1)
    if uniform:
        attn = torch.full_like(attn, 1.0 / nk)
    return (attn @ vh).transpose(1, 2).reshape(b, nq, d)


def layernorm(x, g, b):
    return F.layer_norm(x, (x.shape[-1],), g, b, 1e-5)


def refine(x4, head, dtype=torch.float64, enc_uniform=False, slot_uniform=False, cross_uniform=False,
           self_uniform=False, quick_gelu=False):
    """Token_Refine.forward on x4 [B,2048,H,W] (NCHW) with folded weights:
    dict(X [B,N,mid] the encoder output, A [B,n_obj,N] the slot weights, tn the
    tokens after token_norm, dec0 / dec1 the tokens after each decoder, pre
    [B,1024] the head's output before F.normalize)."""
    w = {k: v.to(dtype) for k, v in head.items()}
    lin = lambda x, n: x @ w[n + "_w"].reshape(w[n + "_w"].shape[0], -1).t() + w[n + "_b"]  # noqa: E731
    b, cin, hh, ww = x4.shape
    mid = w["conv_w"].shape[0]
    x = lin(x4.to(dtype).permute(0, 2, 3, 1).reshape(b, hh * ww, cin), "conv")
    qkv = lin(x, "enc_qkv")
    x = x + lin(mha(qkv[..., :mid], qkv[..., mid:2 * mid], qkv[..., 2 * mid:], uniform=enc_uniform), "enc_proj")
    x = x + lin(x, "enc_mlp")
    a = F.softmax(torch.matmul(w["query"], x.permute(0, 2, 1)), dim=1)
    if slot_uniform:
        a = torch.full_like(a, 1.0 / a.shape[1])
    t0 = torch.bmm(a, x)
    t = layernorm(lin(t0, "tn"), w["tn_g"], w["tn_beta"])
    got = {"X": x, "A": a, "T0": t0, "tn": t}
    kv = lin(x, "dec_kv")
    for i in (0, 1):
        p = f"d{i}_"
        k, v = kv[..., 2 * i * mid:(2 * i + 1) * mid], kv[..., (2 * i + 1) * mid:(2 * i + 2) * mid]
        q = lin(layernorm(t, w[p + "ln1_g"], w[p + "ln1_b"]), p + "cq")
        t = t + lin(mha(q, k, v, uniform=cross_uniform), p + "cproj")
        hdn = lin(t, p + "fc1")
        hdn = hdn * torch.sigmoid(1.702 * hdn) if quick_gelu else F.gelu(hdn)
        t = t + lin(hdn, p + "fc2")
        sq = lin(layernorm(t, w[p + "ln2_g"], w[p + "ln2_b"]), p + "sqkv")
        t = t + lin(mha(sq[..., :mid], sq[..., mid:2 * mid], sq[..., 2 * mid:], uniform=self_uniform), p + "sproj")
        got[f"dec{i}"] = t
    got["pre"] = lin(t.reshape(b, -1), "out")
    return got


def head_forward(x4, head, dtype=torch.float64, **switches):
    """Everything after the trunk: refine(...) plus out [B,1024] = F.normalize(pre)."""
    got = refine(x4, head, dtype, **switches)
    got["out"] = F.normalize(got["pre"], dim=-1)
    return got
