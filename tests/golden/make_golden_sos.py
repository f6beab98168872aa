"""Generate tests/golden/sos.npz from the REFERENCE's own SoSNetModel
(models/sosnet.py:95-183) with its SimilarityAttention (:58-92) and
SecondOrderPooling (:12-55).

Run where make_golden_how.py runs (it imports the reference tree, which the
GPU box does not have):
    PYTHONDONTWRITEBYTECODE=1 python tests/golden/make_golden_sos.py
SoSNetModel's constructor builds a torchvision trunk, and torchvision is
absent, so the module is assembled without it, exactly as make_golden_how.py
does: models/sosnet.py is loaded by file under the torchvision stub, then
SoSNetModel.__new__ + nn.Module.__init__, the reference's own
SimilarityAttention(2048), SecondOrderPooling(2048, 32, normalize=True),
feature_proj = Sequential(Linear(528, 2048), ReLU, Dropout, Linear(2048,
2048)), classifier, and backbone = a wrapper returning x4 of the reference's
torchvision-free ResNet_DOLG with each stage-entry stride moved to the 3x3 (its
x4 is tests/golden/resnet_dolg_v15.npz).  second_order_dim = 32: the default
512 would need 269 M weights in feature_proj's first Linear.  Trunk weights and
inputs are the trunk fixture's (inputs.TRUNK_WEIGHT_SEED / TRUNK_CASES), head
weights weights.synthetic_sos_head(SOS_HEAD_SEED, 32, 8).  Only data is
written: seeds and the outputs / intermediates of the reference's modules.

Two groups:
 (a) end to end, extract_descriptor on inputs.TRUNK_CASES (wiring: the seeded
     trunk's x4 is almost the same at every position);
 (b) head only, the reference's similarity_attention -> second_order_pool ->
     feature_proj -> normalize on inputs.feature_map(12000 + h w, b, 2048, h, w)
     for HEAD_CASES: the descriptor per case and, for (1, 5, 9), att [1,45],
     vhat [1,528] and features [1,2048].  Inputs are regenerated from seeds.
For every stored case the range of a and the float32-vs-float64 restatement
error (tests/sos_ref.py) are printed; every head case's a must span
[<= 0.2, >= 0.8] (a condition on the synthetic head: a constant a cancels in the
L2, so a head that ignored the attention would pass).
"""
import importlib.util
import os
import sys

import numpy as np
import torch

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, HERE)
sys.path.insert(0, os.path.dirname(HERE))
sys.path.insert(0, os.path.dirname(os.path.dirname(HERE)))
import inputs as I  # noqa: E402
from make_golden import REF, _stub_torchvision  # noqa: E402  (the same torchvision stub)

SOS_HEAD_SEED = 131
SOS_DIM = 32
HEAD_CASES = ((2, 7, 7), (1, 5, 9), (1, 17, 19))


def head_tag(b, h, w):
    return f"head_b{b}_{h}x{w}"


def head_input(b, h, w):
    return torch.from_numpy(I.feature_map(12000 + h * w, b, 2048, h, w))


def load_reference_module():
    spec = importlib.util.spec_from_file_location("ref_sosnet", os.path.join(REF, "models", "sosnet.py"))
    mod = importlib.util.module_from_spec(spec)
    spec.loader.exec_module(mod)
    return mod


def build_reference_sosnet(ref):
    import torch.nn as nn
    from networks.backbone import ResNet_DOLG, ResBlock
    from research_image_retrieval_amd.weights import synthetic_sos_head, synthetic_resnet_state_dict, to_dolg_keys

    class Trunk(nn.Module):
        def __init__(self):
            super().__init__()
            self.net = ResNet_DOLG()

        def forward(self, x):
            return self.net(x)[1]

    net = ref.SoSNetModel.__new__(ref.SoSNetModel)
    nn.Module.__init__(net)
    net.backbone = Trunk()
    net.backbone.net.load_state_dict(to_dolg_keys(synthetic_resnet_state_dict("resnet101", I.TRUNK_WEIGHT_SEED)),
                                     strict=True)
    moved = 0
    for m in net.backbone.net.modules():
        if isinstance(m, ResBlock) and m.f.a.stride != (1, 1):
            m.f.b.stride, m.f.a.stride = m.f.a.stride, (1, 1)
            moved += 1
    assert moved == 3, moved
    net.use_attention = True
    net.similarity_attention = ref.SimilarityAttention(2048)
    net.second_order_pool = ref.SecondOrderPooling(input_dim=2048, output_dim=SOS_DIM, normalize=True)
    so = SOS_DIM * (SOS_DIM + 1) // 2
    net.feature_proj = nn.Sequential(nn.Linear(so, 2048), nn.ReLU(inplace=True), nn.Dropout(0.5),
                                     nn.Linear(2048, 2048))
    net.classifier = nn.Linear(2048, 8)
    head = synthetic_sos_head(SOS_HEAD_SEED, SOS_DIM, 8)
    missing, unexpected = net.load_state_dict(head, strict=False)
    assert not unexpected and all(k.startswith("backbone.") for k in missing), (missing, unexpected)
    net.eval()
    return net, head


def main():
    _stub_torchvision()
    sys.path.insert(0, REF)
    torch.set_num_threads(8)
    import torch.nn.functional as F
    import sos_ref
    from research_image_retrieval_amd.weights import sos_head_from_state_dict
    ref = load_reference_module()
    net, raw = build_reference_sosnet(ref)
    head = sos_head_from_state_dict(raw)
    out = {"weight_seed": I.TRUNK_WEIGHT_SEED, "head_seed": SOS_HEAD_SEED, "second_order_dim": SOS_DIM}
    seen = {}
    net.backbone.register_forward_hook(lambda _m, _i, o: seen.__setitem__("x4", o))

    def report(tag, x4, must_span):
        r64, r32 = sos_ref.head_forward(x4, head, torch.float64), sos_ref.head_forward(x4, head, torch.float32)
        a = r64["att"]
        d = (r32["out"].double() - r64["out"]).abs().max().item()
        print(f"   {tag}: a in [{float(a.min()):.4f}, {float(a.max()):.4f}]; float32 vs float64 restatement {d:.3e}")
        if must_span:
            assert float(a.min()) <= 0.2 and float(a.max()) >= 0.8, (tag, float(a.min()), float(a.max()))

    with torch.no_grad():
        for tag, (seed, b, h, w) in I.TRUNK_CASES.items():
            desc = net.extract_descriptor(I.trunk_input(seed, b, h, w))
            out[f"{tag}_out"] = desc.numpy()
            out[f"{tag}_case"] = np.array([seed, b, h, w])
            print(tag, "descriptor", tuple(desc.shape))
            report(tag, seen["x4"], False)
        # (b): the same modules after the trunk, in extract_features' order (:149-161, :182)
        for b, h, w in HEAD_CASES:
            tag = head_tag(b, h, w)
            x4 = head_input(b, h, w)
            attended, att = net.similarity_attention(x4)
            vhat = net.second_order_pool(attended)
            feats = net.feature_proj(vhat)
            out[f"{tag}_out"] = F.normalize(feats, p=2, dim=1).numpy()
            print(tag, "descriptor", tuple(feats.shape))
            report(tag, x4, True)
            if (b, h, w) == (1, 5, 9):
                out[f"{tag}_att"] = att.reshape(b, h * w).numpy()
                out[f"{tag}_vhat"] = vhat.numpy()
                out[f"{tag}_features"] = feats.numpy()
    np.savez_compressed(os.path.join(HERE, "sos.npz"), **out)
    print("sos.npz written to", HERE, os.path.getsize(os.path.join(HERE, "sos.npz")), "bytes")


if __name__ == "__main__":
    main()
