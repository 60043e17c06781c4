"""CLIP on HIP against eager torch, one process (DESIGN.md section 9 "CLIP evaluation").

    python tools/bench_clip.py [--batches 256 4] [--launches 30] [--tower 24x1024x14x224] [--skip_towers] [--skip_gemm]

* ViT-L/14 image tower (random init), ms per pass and images/s, in ``32`` and ``bf16`` -- and an eager torch composition of the same
  forward on the same weights in fp32 and under ``autocast(bfloat16)``;
* the ``c_fc`` GEMM of that tower at B = 256 (M 65 792, K 1024, N 4096) with ACT_QUICK_GELU, ACT_GELU and ACT_NONE.
Timed by tools/timing.py on single launches (``calls=1``): median [min, max] of ``--launches`` bracketed launches per side, the
activations in turn, each HIP precision in turn with its eager composition.  Prints one JSON line."""
import argparse
import json
import os
import sys

import torch
import torch.nn.functional as F

import timing

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(ROOT, "multimodal-baby_amd"))

from multimodal import _hip as H                          # noqa: E402
from multimodal import clip_model as CM                    # noqa: E402


def torch_image_tower(v, x):
    """Eager torch: conv patches, class token, ln_pre, pre-LN blocks with QuickGELU, ln_post, projection."""
    W = v.embed_dim
    h = F.conv2d(x, v.conv1.weight.to(x.dtype), stride=v.patch_size).flatten(2).transpose(1, 2)
    h = torch.cat([v.class_embedding.to(h.dtype).expand(h.shape[0], 1, W), h], 1) + v.positional_embedding.to(h.dtype)
    h = F.layer_norm(h, (W,), v.ln_pre.weight, v.ln_pre.bias, 1e-5)
    heads = W // 64
    for b in v.transformer.resblocks:
        y = F.layer_norm(h, (W,), b.ln_1.weight, b.ln_1.bias, 1e-5)
        qkv = F.linear(y, b.attn.in_proj_weight, b.attn.in_proj_bias)
        B, T, _ = qkv.shape
        q, k, vv = (qkv.reshape(B, T, 3, heads, 64)[:, :, i].transpose(1, 2) for i in range(3))
        a = F.scaled_dot_product_attention(q, k, vv).transpose(1, 2).reshape(B, T, W)
        h = h + F.linear(a, b.attn.out_proj.weight, b.attn.out_proj.bias)
        y = F.linear(F.layer_norm(h, (W,), b.ln_2.weight, b.ln_2.bias, 1e-5), b.mlp.c_fc.weight, b.mlp.c_fc.bias)
        h = h + F.linear(y * torch.sigmoid(1.702 * y), b.mlp.c_proj.weight, b.mlp.c_proj.bias)
    return F.layer_norm(h[:, 0], (W,), v.ln_post.weight, v.ln_post.bias, 1e-5) @ v.proj.to(h.dtype)


def main(argv=None):
    ap = argparse.ArgumentParser()
    ap.add_argument("--batches", type=int, nargs="+", default=[256, 4])
    ap.add_argument("--launches", type=int, default=30)
    ap.add_argument("--tower", default="24x1024x14x224", help="image tower: layers x width x patch x resolution (default: ViT-L/14)")
    ap.add_argument("--skip_towers", action="store_true")
    ap.add_argument("--skip_gemm", action="store_true")
    args = ap.parse_args(argv)
    dev = torch.device("cuda:0")
    res = {"bench": "clip"}
    if not args.skip_gemm:
        M, K, N = 65792, 1024, 4096
        g = torch.Generator().manual_seed(0)
        A = torch.randn(M, K, generator=g).bfloat16().to(dev)
        W = (torch.randn(N, K, generator=g) / K ** 0.5).bfloat16().to(dev)
        bias, out = torch.randn(N, generator=g).to(dev), torch.empty(M, N, dtype=torch.bfloat16, device=dev)
        acts = {"quick_gelu": H.ACT_QUICK_GELU, "gelu": H.ACT_GELU, "none": H.ACT_NONE}
        launches = max(args.launches, 20)
        t = timing.measure({name: lambda act=act: H.gemm(A, W, out=out, bias=bias, act=act) for name, act in acts.items()},
                           calls=1, repeats=launches, warmup=10)                                  # single launches, the activations in turn
        for name in acts:
            res.update(timing.entry(t[name], f"c_fc_{name}_us", 1e3, 1))
        res["c_fc_launches_per_activation"] = launches
        res["c_fc_quick_gelu_over_gelu"] = round(res["c_fc_quick_gelu_us"] / res["c_fc_gelu_us"], 4)
        del A, W, out
    if not args.skip_towers:
        torch.manual_seed(0)
        layers, width, patch, size = (int(v) for v in args.tower.split("x"))
        model = CM.CLIP(embed_dim=768, image_resolution=size, vision_layers=layers, vision_width=width, vision_patch_size=patch,
                        context_length=77, vocab_size=49408, transformer_width=768, transformer_layers=12).to(dev).eval()
        for B in args.batches:
            x = torch.randn(B, 3, size, size, device=dev)
            n = max(3, min(args.launches, 2560 // B))

            def eager(cast):
                with torch.no_grad(), torch.autocast("cuda", dtype=torch.bfloat16, enabled=cast):
                    return torch_image_tower(model.visual, x)

            # a precision switch re-casts the tower's weights on the next pass, so the precisions are not alternated: each HIP
            # precision alternates with the eager composition in the same arithmetic
            for prec, ref, cast in (("32", "torch_fp32", False), ("bf16", "torch_autocast_bf16", True)):
                model.set_precision(prec)
                t = timing.measure({f"hip_{prec}": lambda: model.encode_image(x), ref: lambda: eager(cast)}, calls=1, repeats=n, warmup=2)
                for side, r in t.items():
                    res.update(timing.entry(r, f"{side}_B{B}_ms", digits=3))
                    res[f"{side}_B{B}_img_s"] = round(B / r["ms"] * 1e3, 1)
    print(json.dumps(res))


if __name__ == "__main__":
    main()
