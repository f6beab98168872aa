"""Plain-torch restatement of the token aggregator's head (models/token_based.py
:13-159), a test helper.  head_forward writes the reference's own sequence,
LITERALLY and unfolded: input_proj per position (:68), + pe[i] (:32, :71), the
global token in front (:74-75), every post-norm encoder layer over every row
(nn.TransformerEncoderLayer, norm_first=False, ReLU, eps 1e-5: in_proj, per-head
softmax(q k^T / sqrt(e)) v, out_proj, + residual, norm1, linear1, ReLU, linear2,
+ residual, norm2), row 0 (:81), output_proj (:84), feature_proj (:135) and
F.normalize (:158), on the weight format of weights.tokagg_head_from_state_dict,
in any dtype.  It is independent of the fold the kernels use;
last_layer_folded writes that.  tests/test_tokagg_host.py pins both to the
reference's own output (tests/golden/tokagg.npz), so the GPU tests may use them
at other shapes and in float64.

This is the aggregator of models/token_based.py, not networks.Token
(tests/token_ref.py).
"""
import math

import torch
import torch.nn.functional as F

from research_image_retrieval_amd import weights as W

EPS_LN = 1e-5


def cls_attn_pool(x, qt, dtype=torch.float64, subtract_max=True):
    """What rr_cls_attn_pool computes: x [B,seq,d], qt [B,heads,d] -> (out
    [B,heads,d], p [B,heads,seq]).  subtract_max=False: the naive exp / sum
    (overflows in float32 on large scores)."""
    x, qt = x.to(dtype), qt.to(dtype)
    s = torch.einsum("bhd,bjd->bhj", qt, x)
    if subtract_max:
        p = torch.softmax(s, dim=-1)
    else:
        e = torch.exp(s)
        p = e / e.sum(dim=-1, keepdim=True)
    return torch.einsum("bhj,bjd->bhd", p, x), p


def attention_probs(x, layer, heads, dtype):
    """softmax(q k^T / sqrt(e)) of nn.MultiheadAttention on rows x [B,seq,d]: (p
    [B,heads,seq,seq], v [B,heads,seq,e])."""
    b, seq, d = x.shape
    e = d // heads
    qkv = F.linear(x, layer["qkv_w"].to(dtype), layer["qkv_b"].to(dtype))
    q, k, v = (t.reshape(b, seq, heads, e).transpose(1, 2) for t in qkv.split(d, dim=2))
    return torch.softmax(q @ k.transpose(2, 3) / math.sqrt(e), dim=-1), v


def encoder_layer(x, layer, heads, dtype=torch.float64, uniform=False, taps=None):
    """One post-norm nn.TransformerEncoderLayer, eval mode, on x [B,seq,d]:
    every row.  uniform=True replaces the softmax by 1 / seq (a sensitivity
    switch).  taps receives p0 [B,heads,seq], the global token's row of the
    attention, and pooled [B,heads,d] = sum_j p0_hj x_j."""
    b, seq, d = x.shape
    g = lambda k: layer[k].to(dtype)  # noqa: E731
    p, v = attention_probs(x, layer, heads, dtype)
    if uniform:
        p = torch.full_like(p, 1.0 / seq)
    if taps is not None:
        taps["p"] = p[:, :, 0, :]
        taps["pooled"] = torch.einsum("bhj,bjd->bhd", p[:, :, 0, :], x)
    att = (p @ v).transpose(1, 2).reshape(b, seq, d)
    x = F.layer_norm(x + F.linear(att, g("out_w"), g("out_b")), (d,), g("n1_g"), g("n1_b"), EPS_LN)
    ff = F.linear(F.relu(F.linear(x, g("l1_w"), g("l1_b"))), g("l2_w"), g("l2_b"))
    return F.layer_norm(x + ff, (d,), g("n2_g"), g("n2_b"), EPS_LN)


def tokens(x4, head, dtype=torch.float64, positional=True, global_token=True):
    """x4 [B,Cin,H,W] -> [B,1+HW,d]: input_proj, + pe, the global token in front."""
    b, cin, h, w = x4.shape
    n = h * w
    if n > head["pe"].shape[0]:
        raise ValueError(f"{n} positions exceed max_len = {head['pe'].shape[0]}")
    x = x4.to(dtype).reshape(b, cin, n).permute(0, 2, 1)                       # :65 (batch first)
    x = F.linear(x, head["in_w"].to(dtype), head["in_b"].to(dtype))            # :68
    if positional:
        x = x + head["pe"][:n].to(dtype)                                        # :32
    gt = head["global_token"].to(dtype) if global_token else torch.zeros_like(head["global_token"], dtype=dtype)
    return torch.cat([gt.expand(b, 1, -1), x], dim=1)                           # :74-75


def head_forward(x4, head, heads, dtype=torch.float64, uniform_last=False, positional=True, global_token=True,
                 skip_layer0=False):
    """Everything after the trunk on x4 [B,Cin,H,W] (NCHW), literal unfolded
    form: dict(tokens [B,seq,d], layer_out (the LAST layer's input), p
    [B,heads,seq] and pooled [B,heads,d] (the last layer's global-token row),
    agg [B,Cin], features, out).  The switches each disable one piece (the
    sensitivity tests)."""
    got = {"tokens": tokens(x4, head, dtype, positional, global_token)}
    x = got["tokens"]
    n_layers = W.tokagg_num_layers(head)
    for i in range(n_layers):
        last = i == n_layers - 1
        if last:
            got["layer_out"] = x
        if i == 0 and skip_layer0 and not last:
            continue
        x = encoder_layer(x, W.tokagg_layer(head, i), heads, dtype, uniform=uniform_last and last,
                          taps=got if last else None)
    got["agg"] = F.linear(x[:, 0], head["op_w"].to(dtype), head["op_b"].to(dtype))         # :81-84
    got["features"] = F.linear(got["agg"], head["fp_w"].to(dtype), head["fp_b"].to(dtype))  # :135
    got["out"] = F.normalize(got["features"], p=2, dim=1)                                    # :158
    return got


def last_layer_folded(x, layer, heads, dtype=torch.float32, taps=None):
    """Row 0 of encoder_layer(x) as the kernels compute it: q~ = A x0 + a0,
    cls_attn_pool, M . + m0 + x0, norm1, the FFN on B rows, norm2.  [B,d]."""
    b, seq, d = x.shape
    x = x.to(dtype)
    a, a0, m, m0 = W.tokagg_fold_last_layer(layer, heads, dtype)
    g = lambda k: layer[k].to(dtype)  # noqa: E731
    x0 = x[:, 0]
    qt = F.linear(x0, a, a0).view(b, heads, d)
    pooled, p = cls_attn_pool(x, qt, dtype)
    if taps is not None:
        taps.update(p=p, pooled=pooled)
    y = F.layer_norm(F.linear(pooled.reshape(b, heads * d), m, m0) + x0, (d,), g("n1_g"), g("n1_b"), EPS_LN)
    ff = F.linear(F.relu(F.linear(y, g("l1_w"), g("l1_b"))), g("l2_w"), g("l2_b"))
    return F.layer_norm(y + ff, (d,), g("n2_g"), g("n2_b"), EPS_LN)
