"""Generate tests/golden/senet_g2.npz from the REFERENCE's own SENetG2Wrapper
(models/senet_g2.py:216-251: SENet :75-129 of SEBottlenecks :32-72 with
SEBlocks :12-29, G2Pooling :132-153, feature_proj).

Run where make_golden_spoc.py runs (it imports the reference tree, which the
GPU box does not have):
    PYTHONDONTWRITEBYTECODE=1 python tests/golden/make_golden_senet.py
models/senet_g2.py imports only torch, so it is loaded by file path and needs
no torchvision stub.  The wrapper is built as the reference builds it and
loaded, strictly, with weights.synthetic_senet_state_dict(arch,
inputs.TRUNK_WEIGHT_SEED) under backbone.backbone.* and
weights.synthetic_senet_g2_head(SENET_HEAD_SEED, 8, FEATURE_DIM, P, ALPHA, BETA)
under backbone.*; p, alpha and beta sit away from the reference's initial 3 / 1
/ 0, so the powf path of the GeM and the alpha / beta fold are exercised.  Only
data is written: seeds and outputs / intermediates of the reference's modules.

Contents: senet50 descriptors on both inputs.TRUNK_CASES (b1_odd's x4 is
4 x 5), senet101's on b1_odd; for senet50 / b1_odd the gates [B,C] of layer1.0,
layer2.0 (a stage entry with a stride) and layer4.2 (forward hooks on
SEBlock.fc), the first 64 channels of x4 (NHWC) and the pooled vector
(G2Pooling's output, alpha * GeM + beta).
Condition on the synthetic SE weights, asserted here and printed: in every SE
block of every case the gates span [<= 0.2, >= 0.8].
"""
import importlib.util
import os
import sys

import numpy as np
import torch

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, HERE)
sys.path.insert(0, os.path.dirname(os.path.dirname(HERE)))
import inputs as I  # noqa: E402
from make_golden import REF  # noqa: E402

SENET_HEAD_SEED = 151
FEATURE_DIM = 256
NUM_CLASSES = 8
P, ALPHA, BETA = 2.5, 1.3, 0.07
GATE_BLOCKS = ("layer1.0", "layer2.0", "layer4.2")
CASES = (("senet50", "b2_224"), ("senet50", "b1_odd"), ("senet101", "b1_odd"))


def load_reference_module():
    spec = importlib.util.spec_from_file_location("ref_senet_g2", os.path.join(REF, "models", "senet_g2.py"))
    mod = importlib.util.module_from_spec(spec)
    spec.loader.exec_module(mod)
    return mod


def wrapper_state_dict(arch):
    """The synthetic trunk and head under the wrapper's keys."""
    from research_image_retrieval_amd import weights as W
    sd = {f"backbone.backbone.{k}": v for k, v in W.synthetic_senet_state_dict(arch, I.TRUNK_WEIGHT_SEED).items()}
    sd.update({f"backbone.{k}": v for k, v in
               W.synthetic_senet_g2_head(SENET_HEAD_SEED, NUM_CLASSES, FEATURE_DIM, P, ALPHA, BETA).items()})
    return sd


def save_npz(path, arrays):
    """np.savez_compressed's layout with a fixed member date (numpy stamps the
    current time), so that the file regenerates byte for byte."""
    import zipfile
    with zipfile.ZipFile(path, "w", zipfile.ZIP_DEFLATED) as z:
        for k, v in arrays.items():
            info = zipfile.ZipInfo(k + ".npy", date_time=(1980, 1, 1, 0, 0, 0))
            info.compress_type = zipfile.ZIP_DEFLATED
            with z.open(info, "w", force_zip64=True) as f:
                np.lib.format.write_array(f, np.asanyarray(v), allow_pickle=False)


def main():
    torch.set_num_threads(8)
    ref = load_reference_module()
    out = {"weight_seed": I.TRUNK_WEIGHT_SEED, "head_seed": SENET_HEAD_SEED, "feature_dim": FEATURE_DIM,
           "num_classes": NUM_CLASSES, "g2": np.array([P, ALPHA, BETA], dtype=np.float64)}
    nets = {}
    with torch.no_grad():
        for arch, tag in CASES:
            if arch not in nets:
                net = ref.SENetG2Wrapper(NUM_CLASSES, backbone=arch, feature_dim=FEATURE_DIM)
                net.load_state_dict(wrapper_state_dict(arch), strict=True)
                nets[arch] = net.eval()
            net = nets[arch]
            gates, seen, hooks = {}, {}, []
            trunk = net.backbone.backbone
            for name, m in trunk.named_modules():
                if isinstance(m, ref.SEBlock):
                    hooks.append(m.fc.register_forward_hook(
                        lambda _m, _i, o, name=name[:-3]: gates.__setitem__(name, o.clone())))
            hooks.append(trunk.register_forward_hook(lambda _m, _i, o: seen.__setitem__("x4", o)))
            hooks.append(net.backbone.g2_pool.register_forward_hook(lambda _m, _i, o: seen.__setitem__("g2", o)))
            seed, b, h, w = I.TRUNK_CASES[tag]
            desc = net.extract_global_descriptor(I.trunk_input(seed, b, h, w))
            for hk in hooks:
                hk.remove()
            key = f"{arch}_{tag}"
            out[f"{key}_out"] = desc.numpy()
            out[f"{key}_case"] = np.array([seed, b, h, w])
            x4 = seen["x4"]
            lo = max(float(g.min()) for g in gates.values())
            hi = min(float(g.max()) for g in gates.values())
            print(f"{key}: descriptor {tuple(desc.shape)}, x4 {tuple(x4.shape)} max {float(x4.max()):.3f} zeros "
                  f"{float((x4 == 0).float().mean()):.2f}; {len(gates)} SE blocks, largest gate minimum {lo:.4f}, "
                  f"smallest gate maximum {hi:.4f}")
            for name, g in gates.items():
                assert float(g.min()) <= 0.2 and float(g.max()) >= 0.8, (key, name, float(g.min()), float(g.max()))
            if (arch, tag) == ("senet50", "b1_odd"):
                for name in GATE_BLOCKS:
                    out[f"{key}_gate_{name}"] = gates[name].numpy()
                out[f"{key}_x4_64"] = x4[:, :64].permute(0, 2, 3, 1).contiguous().numpy()
                out[f"{key}_pooled"] = seen["g2"].flatten(1).numpy()  # G2Pooling's output: alpha * GeM + beta
    path = os.path.join(HERE, "senet_g2.npz")
    save_npz(path, out)
    print("senet_g2.npz written to", HERE, os.path.getsize(path), "bytes")


if __name__ == "__main__":
    main()
