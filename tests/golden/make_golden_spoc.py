"""Generate tests/golden/spoc.npz from the REFERENCE's own SpoCModel
(models/spoc.py:97-195) with its ContextualAttention (:52-94) and
SpatialPyramidPooling (:12-49).

Run where make_golden_sos.py runs (it imports the reference tree, which the
GPU box does not have):
    PYTHONDONTWRITEBYTECODE=1 python tests/golden/make_golden_spoc.py
SpoCModel's constructor builds a torchvision trunk, and torchvision is absent,
so the module is assembled without it, exactly as make_golden_sos.py does:
models/spoc.py is loaded by file under the torchvision stub, then
SpoCModel.__new__ + nn.Module.__init__, the reference's own
ContextualAttention(2048, 512), SpatialPyramidPooling([1, 2, 4], 'max'), and
feature_aggregation / feature_proj / classifier as :131-147 builds them, and
backbone = a wrapper returning x4 of the reference's torchvision-free
ResNet_DOLG with each stage-entry stride moved to the 3x3 (its x4 is
tests/golden/resnet_dolg_v15.npz).  Trunk weights and inputs are the trunk
fixture's (inputs.TRUNK_WEIGHT_SEED / TRUNK_CASES), head weights
weights.synthetic_spoc_head(SPOC_HEAD_SEED).  Only data is written: seeds and
the outputs / intermediates of the reference's modules.

Three groups:
 (a) end to end, extract_descriptor on inputs.TRUNK_CASES (b1_odd's x4 is
     4 x 5, the smallest legal map);
 (b) head only, contextual_attention -> spp -> feature_aggregation ->
     feature_proj -> normalize on inputs.feature_map(13000 + h w, b, 2048, h, w)
     for HEAD_CASES: the descriptor per case and, for (1, 5, 9), att [1,45],
     agg [1,2048], features [1,2048] and the first 64 channels of pooled
     ([1,25,64]) with the same channels of the refined map they were pooled
     from ([1,5,9,64], NHWC): pooling the one gives the other value for value,
     which pins the region order and the floor mode (the restatement's own
     refined map differs from the reference's in the last bits, the BNs being
     folded, so its pooled values can only be close);
 (c) one use_context=False descriptor on (1, 5, 9): a second model without the
     contextual attention, weights synthetic_spoc_head(SPOC_HEAD_SEED, 512, 8,
     use_context=False).
Conditions on the synthetic head, asserted here and printed: in every head
case a spans [<= 0.2, >= 0.8] and each pyramid level supplies the winning
region of at least one agg column; at least one agg column is exactly 0.
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

SPOC_HEAD_SEED = 146
LEVELS = [1, 2, 4]
HEAD_CASES = ((2, 7, 7), (1, 5, 9), (1, 17, 19), (1, 4, 4))


def head_tag(b, h, w):
    return f"head_b{b}_{h}x{w}"


def head_input(b, h, w):
    return torch.from_numpy(I.feature_map(13000 + h * w, b, 2048, h, w))


def load_reference_module():
    spec = importlib.util.spec_from_file_location("ref_spoc", os.path.join(REF, "models", "spoc.py"))
    mod = importlib.util.module_from_spec(spec)
    spec.loader.exec_module(mod)
    return mod


def build_reference_spoc(ref, use_context=True):
    import torch.nn as nn
    from networks.backbone import ResNet_DOLG, ResBlock
    from research_image_retrieval_amd.weights import synthetic_spoc_head, synthetic_resnet_state_dict, to_dolg_keys

    class Trunk(nn.Module):
        def __init__(self):
            super().__init__()
            self.net = ResNet_DOLG()

        def forward(self, x):
            return self.net(x)[1]

    net = ref.SpoCModel.__new__(ref.SpoCModel)
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
    net.use_context = use_context
    if use_context:
        net.contextual_attention = ref.ContextualAttention(2048, 512)
    net.pyramid_levels = LEVELS
    net.spp = ref.SpatialPyramidPooling(levels=LEVELS, pool_type='max')
    net.feature_aggregation = nn.Sequential(nn.Conv1d(2048, 2048, 1), nn.BatchNorm1d(2048), nn.ReLU(inplace=True),
                                            nn.AdaptiveMaxPool1d(1))
    net.feature_proj = nn.Sequential(nn.Linear(2048, 2048), nn.ReLU(inplace=True), nn.Dropout(0.5),
                                     nn.Linear(2048, 2048))
    net.classifier = nn.Linear(2048, 8)
    head = synthetic_spoc_head(SPOC_HEAD_SEED, 512, 8, use_context)
    missing, unexpected = net.load_state_dict(head, strict=False)
    assert not unexpected and all(k.startswith("backbone.") or k.endswith("num_batches_tracked") for k in missing), \
        (missing, unexpected)
    net.eval()
    return net, head


def main():
    _stub_torchvision()
    sys.path.insert(0, REF)
    torch.set_num_threads(8)
    import torch.nn.functional as F
    import spoc_ref
    from research_image_retrieval_amd.weights import spoc_head_from_state_dict
    ref = load_reference_module()
    net, raw = build_reference_spoc(ref)
    head = spoc_head_from_state_dict(raw)
    out = {"weight_seed": I.TRUNK_WEIGHT_SEED, "head_seed": SPOC_HEAD_SEED, "levels": np.array(LEVELS)}
    seen = {}
    net.backbone.register_forward_hook(lambda _m, _i, o: seen.__setitem__("x4", o))
    zero_cols = 0

    def report(tag, x4, must):
        nonlocal zero_cols
        r64, r32 = spoc_ref.head_forward(x4, head, torch.float64), spoc_ref.head_forward(x4, head, torch.float32)
        a = r64["att"]
        d = (r32["out"].double() - r64["out"]).abs().max().item()
        h, w = x4.shape[2:]
        # the region that wins each agg column, per image, mapped to its level
        y = F.relu(F.conv1d(r64["pooled"].transpose(1, 2), head["agg_w"].double().unsqueeze(2), head["agg_b"].double()))
        win = y.argmax(dim=2)
        edges = np.cumsum([0] + [spoc_ref.regions(h, w, [lv]) for lv in LEVELS])
        live = y.amax(dim=2) > 0
        per_level = [int(((win >= int(edges[i])) & (win < int(edges[i + 1])) & live).sum()) for i in range(len(LEVELS))]
        zeros = int((r64["agg"] == 0).sum())
        zero_cols += zeros
        print(f"   {tag}: a in [{float(a.min()):.4f}, {float(a.max()):.4f}]; winning regions per level {per_level}; "
              f"agg columns exactly 0: {zeros}; float32 vs float64 restatement {d:.3e}")
        if must:
            assert float(a.min()) <= 0.2 and float(a.max()) >= 0.8, (tag, float(a.min()), float(a.max()))
            assert min(per_level) >= 1, (tag, per_level)

    with torch.no_grad():
        for tag, (seed, b, h, w) in I.TRUNK_CASES.items():
            desc = net.extract_descriptor(I.trunk_input(seed, b, h, w))
            out[f"{tag}_out"] = desc.numpy()
            out[f"{tag}_case"] = np.array([seed, b, h, w])
            print(tag, "descriptor", tuple(desc.shape), "x4", tuple(seen["x4"].shape))
            report(tag, seen["x4"], False)
        # (b): the same modules after the trunk, in extract_features' order (:157-171, :194)
        for b, h, w in HEAD_CASES:
            tag = head_tag(b, h, w)
            x4 = head_input(b, h, w)
            refined, att = net.contextual_attention(x4)
            pooled = net.spp(refined)
            agg = net.feature_aggregation(pooled).squeeze(2)
            feats = net.feature_proj(agg)
            out[f"{tag}_out"] = F.normalize(feats, p=2, dim=1).numpy()
            print(tag, "descriptor", tuple(feats.shape), "regions", pooled.shape[2])
            report(tag, x4, True)
            if (b, h, w) == (1, 5, 9):
                out[f"{tag}_att"] = att.reshape(b, h * w).numpy()
                out[f"{tag}_agg"] = agg.numpy()
                out[f"{tag}_features"] = feats.numpy()
                out[f"{tag}_pooled64"] = pooled[:, :64].transpose(1, 2).contiguous().numpy()
                out[f"{tag}_refined64"] = refined[:, :64].permute(0, 2, 3, 1).contiguous().numpy()
        assert zero_cols >= 1, zero_cols
        # (c): use_context=False
        plain, _ = build_reference_spoc(ref, use_context=False)
        x4 = head_input(1, 5, 9)
        feats = plain.feature_proj(plain.feature_aggregation(plain.spp(x4)).squeeze(2))
        out["nocontext_b1_5x9_out"] = F.normalize(feats, p=2, dim=1).numpy()
    np.savez_compressed(os.path.join(HERE, "spoc.npz"), **out)
    print("spoc.npz written to", HERE, os.path.getsize(os.path.join(HERE, "spoc.npz")), "bytes")


if __name__ == "__main__":
    main()
