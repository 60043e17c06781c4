"""CLIP on HIP against eager torch, one process (DESIGN.md section 9 "CLIP evaluation").

    python tools/bench_clip.py [--batches 256 4] [--launches 30] [--skip_towers] [--skip_gemm]

* ViT-L/14 image tower (random init), ms per pass and images/s, in ``32`` and ``bf16`` -- and an eager torch composition of the same
  forward on the same weights in fp32 and under ``autocast(bfloat16)``;
* the ``c_fc`` GEMM of that tower at B = 256 (M 65 792, K 1024, N 4096) with ACT_QUICK_GELU, ACT_GELU and ACT_NONE: event-timed
  launches, the three activations alternating in three rounds (each first once), median over all of an activation's launches
  (>= 20).  Prints one JSON line."""
import argparse
import json
import os
import statistics
import sys

import torch
import torch.nn.functional as F

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(ROOT, "multimodal-baby_amd"))

from multimodal import _hip as H                          # noqa: E402
from multimodal import clip_model as CM                    # noqa: E402


def launch_times(fn, launches, warmup=3):
    """ms of each of ``launches`` event-bracketed calls."""
    for _ in range(warmup):
        fn()
    torch.cuda.synchronize()
    out = []
    for _ in range(launches):
        a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        a.record()
        fn()
        b.record()
        b.synchronize()
        out.append(a.elapsed_time(b))
    return out


def timed(fn, launches, warmup=3):
    """Median ms of ``launches`` event-bracketed calls."""
    return statistics.median(launch_times(fn, launches, warmup))


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


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--batches", type=int, nargs="+", default=[256, 4])
    ap.add_argument("--launches", type=int, default=30)
    ap.add_argument("--skip_towers", action="store_true")
    ap.add_argument("--skip_gemm", action="store_true")
    args = ap.parse_args()
    dev = torch.device("cuda:0")
    res = {"bench": "clip"}
    if not args.skip_gemm:
        M, K, N = 65792, 1024, 4096
        g = torch.Generator().manual_seed(0)
        A = torch.randn(M, K, generator=g).bfloat16().to(dev)
        W = (torch.randn(N, K, generator=g) / K ** 0.5).bfloat16().to(dev)
        bias, out = torch.randn(N, generator=g).to(dev), torch.empty(M, N, dtype=torch.bfloat16, device=dev)
        acts = (("quick_gelu", H.ACT_QUICK_GELU), ("gelu", H.ACT_GELU), ("none", H.ACT_NONE))
        times = {name: [] for name, _ in acts}
        timed(lambda: H.gemm(A, W, out=out, bias=bias, act=H.ACT_NONE), 10, warmup=10)          # clocks up before the first side
        per_round = (max(args.launches, 20) + 2) // 3
        for r in range(3):                                   # the sides alternate, each first in one round
            for name, act in acts[r:] + acts[:r]:
                times[name] += launch_times(lambda: H.gemm(A, W, out=out, bias=bias, act=act), per_round)
        for name, _ in acts:                                 # the median over ALL of an activation's launches (>= 20)
            res[f"c_fc_{name}_us"] = round(1e3 * statistics.median(times[name]), 1)
        res["c_fc_launches_per_activation"] = 3 * per_round
        res["c_fc_quick_gelu_over_gelu"] = round(res["c_fc_quick_gelu_us"] / res["c_fc_gelu_us"], 4)
        del A, W, out
    if not args.skip_towers:
        torch.manual_seed(0)
        model = CM.CLIP(embed_dim=768, image_resolution=224, vision_layers=24, vision_width=1024, vision_patch_size=14, context_length=77,
                        vocab_size=49408, transformer_width=768, transformer_layers=12).to(dev).eval()
        for B in args.batches:
            x = torch.randn(B, 3, 224, 224, device=dev)
            n = max(3, min(args.launches, 2560 // B))
            for prec in ("32", "bf16"):
                model.set_precision(prec)
                ms = timed(lambda: model.encode_image(x), n, warmup=2)
                res[f"hip_{prec}_B{B}_ms"], res[f"hip_{prec}_B{B}_img_s"] = round(ms, 3), round(B / ms * 1e3, 1)
            with torch.no_grad():
                ms = timed(lambda: torch_image_tower(model.visual, x), n, warmup=2)
                res[f"torch_fp32_B{B}_ms"], res[f"torch_fp32_B{B}_img_s"] = round(ms, 3), round(B / ms * 1e3, 1)
                with torch.autocast("cuda", dtype=torch.bfloat16):
                    ms = timed(lambda: torch_image_tower(model.visual, x), n, warmup=2)
                res[f"torch_autocast_bf16_B{B}_ms"], res[f"torch_autocast_bf16_B{B}_img_s"] = round(ms, 3), round(B / ms * 1e3, 1)
    print(json.dumps(res))


if __name__ == "__main__":
    main()
