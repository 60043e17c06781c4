"""Generate tests/golden/caption_gradcam.npz from the reference's own gradCAM_for_captioning_lm, run on the CPU.

    python tools/gen_golden_caption_gradcam.py [REFERENCE_CHECKOUT]

The reference function (analysis_tools/multimodal_visualization.py:9-49) is driven on a stub model: the reference's real
TextEncoder(captioning=True) + LanguageModel at toy size (V = 50, E = H = 32; formula-filled as tools/gen_golden_captioning.py
fills them, output bias ce_bias), and a trunk stub whose ``layer4`` is the identity on a given map [C = 48, 7, 7], followed by the
mean pool and a formula-filled ``fc`` (weight tag 200 scale 0.3, bias tag 201 scale 0.2).  ``calculate_ce_loss`` of the stub = trunk,
optional F.normalize, language_model.calculate_ce_loss.  B = 6 captions of L = 9 tokens with variable lengths (one full-length,
gen_golden_captioning.ce_tokens), both normalize_features settings.  The reference is called caption by caption, trimmed to the
caption's length; positions behind a caption's last word are filled with zeros here.

The file holds data only: the map, tokens, lengths, and per case (``plain``, ``normalized``) the maps of the reference's float64
run (``model.double()``; the expected values), those of its fp32 run, and ref32_dev = max|cam32 - cam64| / max|cam64|.  The test
rebuilds the weights from the formula.  Fixed zip timestamps: re-running reproduces the archive byte for byte.
"""
import os
import sys
import types

import numpy as np
import torch
import torch.nn as nn
import torch.nn.functional as F

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(ROOT, "oracle"))
sys.path.insert(0, os.path.join(ROOT, "tools"))
import gen_golden  # noqa: E402
import gen_golden_captioning as GC  # noqa: E402

V, E, C, HW, B, L = 50, 32, 48, 7, 6, 9
FC_FILL = {"weight": (200, 0.3), "bias": (201, 0.2)}


class Trunk(nn.Module):
    def __init__(self):
        super().__init__()
        self.layer4 = nn.Identity()
        self.fc = nn.Linear(C, E)
        for k, (tag, scale) in FC_FILL.items():
            gen_golden.formula_fill_(getattr(self.fc, k).data, tag, scale)

    def forward(self, fmap):
        return self.fc(self.layer4(fmap).mean(dim=(2, 3)))


class StubModel(nn.Module):
    """What gradCAM_for_captioning_lm touches of a MultiModalLitModel."""

    def __init__(self, language_model, normalize_features):
        super().__init__()
        self.vision_encoder = nn.Module()
        self.vision_encoder.model = Trunk()
        self.language_model = language_model
        self.normalize_features = normalize_features

    def calculate_ce_loss(self, y, y_len, x=None, tokenwise=False):
        f = self.vision_encoder.model(x)
        n = F.normalize(f, p=2, dim=1) if self.normalize_features else f
        return self.language_model.calculate_ce_loss(y, y_len, image_features=n, tokenwise=tokenwise)


def feature_map():
    g = torch.Generator().manual_seed(31)
    return torch.randn(B, C, HW, HW, generator=g).clamp_min(0.0) * 1.5          # a post-ReLU map


def run(viz, model, fmap, y, y_len):
    cams = np.zeros((B, L - 1, HW, HW), dtype=np.float64)
    for b in range(B):
        n = int(y_len[b])
        maps = viz.gradCAM_for_captioning_lm(model, fmap[b].clone(), y[b, :n].clone(), y_len[b].clone())
        assert len(maps) == n and maps[0] is None
        for step in range(1, n):
            assert maps[step].shape == (HW, HW)
            cams[b, step - 1] = maps[step]
    return cams


def main():
    if len(sys.argv) > 1:
        gen_golden.REF = sys.argv[1]
    gen_golden.install_stubs()
    if "cv2" not in sys.modules:
        try:
            import cv2  # noqa: F401
        except ImportError:
            sys.modules["cv2"] = types.ModuleType("cv2")
    from multimodal import multimodal as mm
    from analysis_tools import multimodal_visualization as viz
    torch.set_num_threads(4)
    fmap = feature_map()
    y, y_len = GC.ce_tokens(B, L, V, seed=B + L)
    out = {"map": fmap.numpy(), "y": y.numpy(), "y_len": y_len.numpy(), "cases": np.array(["plain", "normalized"])}
    for name, normalize in (("plain", False), ("normalized", True)):
        te, lm = GC.build(mm, True, V=V, E=E)
        with torch.no_grad():
            lm.output_layer.bias.copy_(GC.ce_bias(V))
        model = StubModel(lm, normalize).eval()
        cam32 = run(viz, model, fmap, y, y_len)
        model.double()
        cam64 = run(viz, model, fmap.double(), y, y_len)
        dev = float(np.abs(cam32 - cam64).max() / np.abs(cam64).max())
        inside = np.concatenate([cam64[b, :int(y_len[b]) - 1].ravel() for b in range(B)])
        print(f"{name}: ref fp32 vs float64 {dev:.2e}; in-caption entries positive {np.mean(inside > 0):.1%}, zero {np.mean(inside == 0):.1%}; "
              f"max {cam64.max():.4f}")
        out[f"{name}.cam64"] = cam64
        out[f"{name}.cam32"] = cam32.astype(np.float32)
        out[f"{name}.ref32_dev"] = np.array([dev])
    path = os.path.join(ROOT, "tests", "golden", "caption_gradcam.npz")
    GC.write_npz(path, out)
    print(f"wrote {path} ({os.path.getsize(path) / 1024:.1f} KiB)")


if __name__ == "__main__":
    main()
