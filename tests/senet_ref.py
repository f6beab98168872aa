"""Plain-torch restatement of the SE-ResNet trunk and the G2+ head
(models/senet_g2.py:12-213), a test helper.  It writes the reference's own
sequence on folded weights (weights.folded_resnet, the eval-mode BN folded into
each conv in float64), in NCHW and in any dtype: per SEBottleneck (:51-72)
conv1 + ReLU, conv2 (the stride on the 3x3) + ReLU, conv3, the SE block
(:25-29: the spatial mean, Linear + ReLU, Linear + sigmoid, x * y), the
downsample projection on a stage's first block, the add and the ReLU; the stem
and its max-pool (:118-122); G2Pooling (:144-153: clamp, pow p, mean, pow 1 / p,
alpha * g + beta, UNFOLDED), feature_proj (:189) and F.normalize (:212).
tests/test_senet_host.py pins it to the reference's own output
(tests/golden/senet_g2.npz), so the GPU tests may use it at other shapes and in
float64.
"""
import torch
import torch.nn.functional as F

from research_image_retrieval_amd import weights as W


def fold(sd, arch, reduction=16):
    """A SENet state dict -> {"conv1": (w, b), "blocks": [(prefix, stride,
    block_weights)]}: block_weights holds conv1 / conv2 / conv3 (and downsample
    on a stage's first block) as folded (w [Cout,KH,KW,Cin], b) and se_w1
    [c / r, c], se_w2 [c, c / r]."""
    tv = W.to_torchvision_keys(sd)
    convs = W.folded_resnet(tv, W.SENET_TRUNKS[arch])
    se = W.senet_se_from_state_dict(sd, arch, reduction)
    blocks = []
    for p, _c in W.senet_block_names(arch):
        li, bi = int(p[5]) - 1, int(p.split(".")[1])
        bw = {k: convs[f"{p}.{k}"] for k in ("conv1", "conv2", "conv3")}
        if bi == 0:
            bw["downsample"] = convs[f"{p}.downsample.0"]
        bw["se_w1"], bw["se_w2"] = se[p]
        blocks.append((p, 2 if (bi == 0 and li > 0) else 1, bw))
    return {"conv1": convs["conv1"], "blocks": blocks}


def _conv(x, wb, dtype, stride=1, pad=0):
    w, b = wb
    return F.conv2d(x, w.to(dtype).permute(0, 3, 1, 2), b.to(dtype), stride=stride, padding=pad)


def block_forward(x, block_weights, stride, dtype=torch.float64):
    """One SEBottleneck on x [B,Cin,H,W] (NCHW): dict(conv3 [B,C,H',W'] (after
    bn3), mean [B,C], hidden [B,C/r], gate [B,C], out [B,C,H',W'])."""
    bw = block_weights
    x = x.to(dtype)
    y = F.relu(_conv(x, bw["conv1"], dtype))
    y = F.relu(_conv(y, bw["conv2"], dtype, stride, 1))
    y = _conv(y, bw["conv3"], dtype)
    mean = y.mean(dim=(2, 3))
    hidden = F.relu(F.linear(mean, bw["se_w1"].to(dtype)))
    gate = torch.sigmoid(F.linear(hidden, bw["se_w2"].to(dtype)))
    idn = _conv(x, bw["downsample"], dtype, stride) if "downsample" in bw else x
    out = F.relu(y * gate[:, :, None, None] + idn)
    return {"conv3": y, "mean": mean, "hidden": hidden, "gate": gate, "out": out}


def trunk_forward(x, folded, dtype=torch.float64, gates=None):
    """SENet.forward (:118-129) on x [B,3,H,W] -> x4 [B,2048,h,w].  gates: a
    dict that receives every block's gate [B,C] under its prefix."""
    x = F.relu(_conv(x.to(dtype), folded["conv1"], dtype, 2, 3))
    x = F.max_pool2d(x, 3, 2, 1)
    for p, stride, bw in folded["blocks"]:
        got = block_forward(x, bw, stride, dtype)
        x = got["out"]
        if gates is not None:
            gates[p] = got["gate"]
    return x


def head_forward(x4, head, dtype=torch.float64, eps=1e-6):
    """Everything after the trunk on x4 [B,C,H,W], literal and unfolded (head:
    weights.senet_g2_head_from_state_dict): dict(pooled [B,C] (the GeM before
    alpha and beta), features [B,F], out [B,F])."""
    x = x4.to(dtype)
    p = torch.tensor(head["p"], dtype=dtype)
    pooled = F.avg_pool2d(x.clamp(min=eps).pow(p), (x.size(-2), x.size(-1))).pow(1.0 / p).flatten(1)
    enhanced = head["alpha"] * pooled + head["beta"]
    feats = F.linear(enhanced, head["proj_w"].to(dtype), head["proj_b"].to(dtype))
    return {"pooled": pooled, "features": feats, "out": F.normalize(feats, p=2, dim=1)}
