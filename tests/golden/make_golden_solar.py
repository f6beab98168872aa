"""Generate tests/golden/solar.npz from the REFERENCE's own SOLAR.forward_test
(networks/RetrievalNet.py:572-590) and SOABlock_GeM (:534-569).

Run where make_golden_dolg.py runs (it imports the reference tree, which the
GPU box does not have):
    PYTHONDONTWRITEBYTECODE=1 python tests/golden/make_golden_solar.py
The reference's SOLAR constructor builds a torchvision trunk, and torchvision
is absent, so the module is assembled without it: SOLAR.__new__ +
nn.Module.__init__, the reference's own SOABlock_GeM(2048, 2), a whiten
Conv2d(2048, 2048, 1) and backbone = a wrapper returning x4 of the reference's
torchvision-free ResNet_DOLG (the "1x1" stride placement).  Trunk weights and
inputs are the trunk fixture's (inputs.TRUNK_WEIGHT_SEED / TRUNK_CASES), head
weights weights.synthetic_solar_head(SOLAR_HEAD_SEED).  Only data is written:
seeds and the outputs / hooked intermediates of the reference's modules.

Two groups:
 (a) end to end, forward_test on inputs.TRUNK_CASES: descriptor and pooled
     vector per case.  This pins WIRING ONLY: the seeded trunk's x4 is almost
     the same at every position, so the attention stays within about 10 % of
     uniform there and a wrong softmax would hardly move the descriptor.
 (b) head only, the reference block -> normalize -> whiten -> normalize on
     inputs.feature_map(7000 + h w, b, 2048, h, w) for HEAD_CASES, where the
     attention is far from uniform (row maxima printed below): descriptor and
     pooled vector per case and, for (1, 5, 9), the attention [1,45,45] and
     attn . h^T [1,45,1024].  Inputs are regenerated from seeds, not stored.
"""
import os
import sys

import numpy as np
import torch

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, HERE)
import inputs as I  # noqa: E402
from make_golden import REF, _stub_torchvision  # noqa: E402  (the same torchvision stub)

SOLAR_HEAD_SEED = 93
HEAD_CASES = ((2, 7, 7), (1, 5, 9), (1, 17, 19))


def head_tag(b, h, w):
    return f"head_b{b}_{h}x{w}"


def head_input(b, h, w):
    return torch.from_numpy(I.feature_map(7000 + h * w, b, 2048, h, w))


def build_reference_solar():
    import torch.nn as nn
    from networks.RetrievalNet import SOLAR, SOABlock_GeM
    from networks.backbone import ResNet_DOLG
    sys.path.insert(0, os.path.dirname(os.path.dirname(HERE)))
    from research_image_retrieval_amd.weights import synthetic_resnet_state_dict, synthetic_solar_head, to_dolg_keys

    class Trunk(nn.Module):
        def __init__(self):
            super().__init__()
            self.net = ResNet_DOLG()

        def forward(self, x):
            return self.net(x)[1]

    net = SOLAR.__new__(SOLAR)
    nn.Module.__init__(net)
    net.backbone = Trunk()
    net.pooling = SOABlock_GeM(in_ch=2048, k=2)
    net.whiten = nn.Conv2d(2048, 2048, kernel_size=(1, 1), stride=1, padding=0, bias=True)
    net.outputdim = 2048
    net.backbone.net.load_state_dict(to_dolg_keys(synthetic_resnet_state_dict("resnet101", I.TRUNK_WEIGHT_SEED)),
                                     strict=True)
    head = synthetic_solar_head(SOLAR_HEAD_SEED)
    for n in "fg":
        head[f"pooling.{n}.1.num_batches_tracked"] = torch.tensor(0, dtype=torch.int64)
    missing, unexpected = net.load_state_dict(head, strict=False)
    assert not unexpected and all(k.startswith("backbone.") for k in missing), (missing, unexpected)
    net.eval()
    return net


def main():
    _stub_torchvision()
    sys.path.insert(0, REF)
    torch.set_num_threads(8)
    import torch.nn.functional as F
    net = build_reference_solar()
    seen = {}
    net.pooling.register_forward_hook(lambda _m, _i, o: seen.__setitem__("pooled", o.flatten(1)))
    out = {"weight_seed": I.TRUNK_WEIGHT_SEED, "head_seed": SOLAR_HEAD_SEED}
    with torch.no_grad():
        for tag, (seed, b, h, w) in I.TRUNK_CASES.items():
            desc = net.forward_test(I.trunk_input(seed, b, h, w))
            out[tag + "_out"] = desc.numpy()
            out[tag + "_pooled"] = seen["pooled"].numpy()
            out[tag + "_case"] = np.array([seed, b, h, w])
            print(tag, "descriptor", tuple(desc.shape))
        # (b): the same modules after the trunk, in forward_test's order (:586-589)
        blk = net.pooling
        for b, h, w in HEAD_CASES:
            x = head_input(b, h, w)
            tag = head_tag(b, h, w)
            f = F.normalize(blk(x), p=2.0, dim=1)
            desc = F.normalize(net.whiten(f).squeeze(-1).squeeze(-1), dim=-1)
            out[tag + "_out"] = desc.numpy()
            out[tag + "_pooled"] = seen["pooled"].numpy()
            # the reference's own intermediates, by its own lines :558-564
            n = h * w
            f_x = blk.f(x).view(b, blk.mid_ch, n)
            g_x = blk.g(x).view(b, blk.mid_ch, n)
            h_x = blk.h(x).view(b, blk.mid_ch, n)
            attn = F.softmax((blk.mid_ch ** -.50) * torch.bmm(f_x.permute(0, 2, 1), g_x), dim=-1)
            print(tag, "attention row maxima", float(attn.amax(-1).min()), "to", float(attn.amax(-1).max()),
                  "uniform", 1.0 / n)
            if (b, h, w) == (1, 5, 9):
                out[tag + "_att"] = attn.numpy()
                out[tag + "_ah"] = torch.bmm(attn, h_x.permute(0, 2, 1)).numpy()
    np.savez_compressed(os.path.join(HERE, "solar.npz"), **out)
    print("solar.npz written to", HERE)


if __name__ == "__main__":
    main()
