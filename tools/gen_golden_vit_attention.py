"""Write tests/golden/vit_attention.npz from the reference's own VisionTransformer (CPU, build container only).

    python tools/gen_golden_vit_attention.py [--reference DIR]

The reference's multimodal/vision_transformer_dino_mugs.py is loaded as a file (it imports torch alone).  The tiny ViT of
tests/golden/vit_tiny.npz (weights ``w.*``, input ``x``) gives get_last_selfattention(x) and get_intermediate_layers(x, 3) (the
model has 2 blocks, so that is every block: 2 tensors) at the native resolution and at the two non-native inputs of
vit_tiny_interp.npz.  Only
these outputs are stored; the weights stay where they are.  The float64 restatement the tests use (tests/vit_attention_common.py)
must reproduce the reference's fp32 outputs to 5e-6 relative, the bound oracle/gen_golden.py holds every other restatement to.
Fixed zip timestamps: re-running reproduces the archive byte for byte."""
import argparse
import importlib.util
import io
import os
import sys
import zipfile
from functools import partial

import numpy as np
import torch
import torch.nn as nn

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
GOLDEN = os.path.join(ROOT, "tests", "golden")
OUT = os.path.join(GOLDEN, "vit_attention.npz")
sys.path.insert(0, os.path.join(ROOT, "tests"))

import vit_attention_common as VC                      # noqa: E402

PATCH, HEADS = 8, 2                                    # the tiny ViT of oracle/gen_golden.py case_vit


def write_npz(path, arrays):
    with zipfile.ZipFile(path, "w", compression=zipfile.ZIP_DEFLATED) as zf:
        for k in sorted(arrays):
            info = zipfile.ZipInfo(k + ".npy", date_time=(1980, 1, 1, 0, 0, 0))
            info.compress_type = zipfile.ZIP_DEFLATED
            buf = io.BytesIO()
            np.lib.format.write_array(buf, np.ascontiguousarray(arrays[k]), allow_pickle=False)
            zf.writestr(info, buf.getvalue())


def maxrel(a, b):
    a, b = a.double(), b.double()
    return float((a - b).abs().max() / b.abs().max())


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--reference", default=os.environ.get("CVCL_REFERENCE", "/root/reference"))
    a = ap.parse_args()
    spec = importlib.util.spec_from_file_location("ref_vits", os.path.join(a.reference, "multimodal", "vision_transformer_dino_mugs.py"))
    vits = importlib.util.module_from_spec(spec)
    spec.loader.exec_module(vits)
    g = np.load(os.path.join(GOLDEN, "vit_tiny.npz"))
    gi = np.load(os.path.join(GOLDEN, "vit_tiny_interp.npz"))
    sd = {k[2:]: torch.from_numpy(g[k]) for k in g.files if k.startswith("w.")}
    m = vits.VisionTransformer(img_size=[32], patch_size=PATCH, embed_dim=32, depth=2, num_heads=HEADS, mlp_ratio=4, qkv_bias=True,
                               norm_layer=partial(nn.LayerNorm, eps=1e-6)).eval()
    m.load_state_dict(sd)
    n = len(m.blocks)
    sd64 = VC.to_dtype(sd, torch.float64)
    out = {}
    for tag, x in (("", torch.from_numpy(g["x"])), ("_a", torch.from_numpy(gi["x_a"])), ("_b", torch.from_numpy(gi["x_b"]))):
        with torch.no_grad():
            attn = m.get_last_selfattention(x)
            layers = m.get_intermediate_layers(x, 3)           # n beyond the depth: every block (the reference does not refuse it)
            assert len(layers) == n
            assert torch.equal(m.get_intermediate_layers(x, 1)[0], layers[-1])
            assert torch.equal(layers[-1][:, 0], m(x))
        T = attn.shape[-1]
        assert attn.shape == (x.shape[0], HEADS, T, T) and float((attn.sum(-1) - 1).abs().max()) < 1e-5
        e_a = maxrel(VC.last_selfattention(sd64, x.double(), PATCH, HEADS), attn)
        rest = VC.intermediate_layers(sd64, x.double(), PATCH, HEADS, n)
        e_l = max(maxrel(r, w) for r, w in zip(rest, layers))
        print(f"vit_attention{tag or '_native'}: T {T}  restatement-vs-reference rel err: attention {e_a:.2e}, layers {e_l:.2e}")
        assert e_a <= 5e-6 and e_l <= 5e-6
        out["attn" + tag] = attn.numpy()
        out["layers" + tag] = torch.stack(layers).numpy()       # [n, B, T, D], block order
    write_npz(OUT, out)
    print(f"wrote {OUT}: {len(out)} arrays, {os.path.getsize(OUT)} bytes")


if __name__ == "__main__":
    main()
