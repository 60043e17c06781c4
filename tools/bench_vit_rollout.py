"""ViT attention rollout at B = 256, 224 x 224, ViT-B/16 and ViT-B/14, bf16 and fp32 (random-init weights):
  vit_attention_rollout against the eager torch composition on the device (per block softmax(q k^T scale), head mean, + I,
  normalise, and the bmm chain, on torch's ROCm ops with the same weights; under torch.autocast(bfloat16) for the bf16 rows), and
  vit_cls_attention as the cost floor of walking the blocks.  Then the two kernels alone on one block's qkv and a 12-layer slab:
  cvcl_attention_head_fuse (ms, GB/s of the qkv it reads and the F it writes; next to it cvcl_attention_probs at q_rows = T, the
  [B, heads, T, T] write the fusion replaces) and cvcl_attention_rollout at q_rows = 1 and T (ms, GB/s of the slab it reads).
  The discard variant (``--discard_ratio``, default 0.9; 0 leaves these rows out): vit_attention_rollout_discard next to the plain
  call, and on a 12-layer slab cvcl_attention_discard against the eager torch composition with the same semantics (per matrix
  topk(k, largest=False), index 0 put back, zeros scattered).  Both work in place, so every call is preceded by a copy that
  restores the slab and the copy alone is timed as a third side; the kernel's GB/s counts one read of the slab per digit pass (4),
  the final read and the k zeros written per matrix, over the time without the copy.
Timed by tools/timing.py: ms per call, median [min, max], the sides of a comparison alternating.  Prints one JSON line.

    python tools/bench_vit_rollout.py [--batch 256] [--repeats 7] [--window-ms 200] [--model 12x768x12x224] [--patches 16,14] [--dtypes bf16,f32] [--discard_ratio 0.9]
                                       [--kernel-only]"""
import argparse
import json
import os
import sys
from functools import partial

import torch
import torch.nn.functional as F

import timing

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(ROOT, "multimodal-baby_amd"))

from multimodal import vision_transformer_dino_mugs as vits          # noqa: E402
from multimodal import vit_maps                                       # noqa: E402
from multimodal.attention_maps import vit_attention_rollout, vit_attention_rollout_discard, vit_cls_attention   # noqa: E402


def timed(fns, args):
    """fns: {name: callable}, the sides alternating -> {name: {ms (median), min_ms, max_ms}}."""
    return {k: timing.entry(r, digits=3) for k, r in timing.measure(fns, **timing.keywords(args)).items()}


def eager_rollout(model, x):
    """Row 0 of the rollout without its CLS column, [B, T - 1]: the composition on torch ops, the chain carried as the CLS row."""
    B = x.shape[0]
    D, heads = model.embed_dim, model.num_heads
    h = model.patch_embed.proj(x).flatten(2).transpose(1, 2)
    h = torch.cat([model.cls_token.expand(B, -1, -1).to(h.dtype), h], dim=1) + model.pos_embed
    T, depth, mats = h.shape[1], len(model.blocks), []
    eye = torch.eye(T, device=x.device)
    for i, blk in enumerate(model.blocks):
        y = blk.norm1(h)
        qkv = blk.attn.qkv(y).reshape(B, T, 3, heads, D // heads).permute(2, 0, 3, 1, 4)
        attn = ((qkv[0] @ qkv[1].transpose(-2, -1)) * blk.attn.scale).softmax(dim=-1)
        A = attn.float().mean(1) + eye
        mats.append(A / A.sum(-1, keepdim=True))
        if i == depth - 1:
            break
        h = h + blk.attn.proj((attn @ qkv[2]).transpose(1, 2).reshape(B, T, D))
        h = h + blk.mlp.fc2(F.gelu(blk.mlp.fc1(blk.norm2(h))))
    r = mats[-1][:, :1]
    for A in reversed(mats[:-1]):
        r = torch.bmm(r, A)
    return r[:, 0, 1:].float()


def eager_discard(slab, k):
    """cvcl_attention_discard on torch ops, in place: per matrix the k smallest elements zeroed, flat index 0 kept."""
    flat = slab.view(-1, slab.shape[-1] * slab.shape[-1])
    idx = flat.topk(k, dim=-1, largest=False).indices
    first = flat[:, 0].clone()
    flat.scatter_(1, idx, 0.0)
    flat[:, 0] = first
    return slab


def main(argv=None):
    ap = argparse.ArgumentParser()
    ap.add_argument("--batch", type=int, default=256)
    ap.add_argument("--model", type=str, default="12x768x12x224", help="depth x width x heads x image size (default: ViT-B at 224)")
    timing.add_arguments(ap)
    ap.add_argument("--patches", type=str, default="16,14")
    ap.add_argument("--dtypes", type=str, default="bf16,f32")
    ap.add_argument("--discard_ratio", type=float, default=0.9, help="the ratio of the discard rows; 0: leave them out")
    ap.add_argument("--kernel-only", action="store_true", help="time the kernels alone (the run to put under rocprofv3)")
    args = ap.parse_args(argv)
    ratio = vit_maps.check_discard_ratio(args.discard_ratio)
    dev = torch.device("cuda:0")
    B = args.batch
    depth, width, heads, S = (int(v) for v in args.model.split("x"))
    hd, scale = width // heads, (width // heads) ** -0.5
    res = {"batch": B, "model": args.model, "repeats": args.repeats, "window_ms": args.window_ms, "discard_ratio": ratio, "cases": []}
    for patch in (int(p) for p in args.patches.split(",")):
        torch.manual_seed(0)
        model = vits.VisionTransformer(img_size=[S], patch_size=patch, embed_dim=width, depth=depth, num_heads=heads, mlp_ratio=4, qkv_bias=True,
                                       norm_layer=partial(torch.nn.LayerNorm, eps=1e-6), num_classes=0).to(dev).eval()
        for p in model.parameters():
            p.requires_grad_(False)
        x = torch.randn(B, 3, S, S, device=dev)
        T = (S // patch) ** 2 + 1
        for name in args.dtypes.split(","):
            dt = torch.bfloat16 if name == "bf16" else torch.float32
            model.compute_dtype = dt
            case = {"patch": patch, "dtype": name, "T": T}
            cast = torch.autocast("cuda", dtype=torch.bfloat16, enabled=dt == torch.bfloat16)
            if not args.kernel_only:
                def ref():
                    with torch.no_grad(), cast:
                        return eager_rollout(model, x)
                sides = {"vit_attention_rollout": lambda: vit_attention_rollout(model, x), "eager_torch": ref,
                         "vit_cls_attention": lambda: vit_cls_attention(model, x)}
                if ratio:
                    sides["vit_attention_rollout_discard"] = lambda: vit_attention_rollout_discard(model, x, ratio)
                case.update(timed(sides, args))
                case["speedup_vs_eager"] = round(case["eager_torch"]["ms"] / case["vit_attention_rollout"]["ms"], 2)
                case["rollout_over_cls_floor_ms"] = round(case["vit_attention_rollout"]["ms"] - case["vit_cls_attention"]["ms"], 3)
                if ratio:
                    case["discard_over_plain_ms"] = round(case["vit_attention_rollout_discard"]["ms"] - case["vit_attention_rollout"]["ms"], 3)
                torch.cuda.empty_cache()
            # the kernels alone: one block's qkv, then a depth-layer slab of row-stochastic matrices
            qkv = torch.randn(B * T, 3 * model.embed_dim, device=dev).to(dt)
            fused = torch.empty(B, T, T, dtype=torch.float32, device=dev)
            sides = {"head_fuse": lambda: vit_maps.attention_head_fuse(qkv, B, T, heads, hd, scale, "mean", out=fused),
                     "attention_probs_q_rows_T": lambda: vit_maps.attention_probs(qkv, B, T, heads, hd, scale, T)}
            t = timed(sides, args)
            for key, nbytes in (("head_fuse", qkv.numel() * qkv.element_size() * 2 // 3 + B * T * T * 4),
                                ("attention_probs_q_rows_T", qkv.numel() * qkv.element_size() * 2 // 3 + B * heads * T * T * 4)):
                t[key]["bytes"] = nbytes
                t[key]["gbs"] = round(nbytes / (t[key]["ms"] * 1e-3) / 1e9, 1)
                case["kernel_" + key] = t[key]
            del qkv, fused
            torch.cuda.empty_cache()
            slab = torch.randn(depth, B, T, T, device=dev).softmax(-1)
            sides = {"rollout_q_rows_1": lambda: vit_maps.rollout_chain(slab, 0, 1),
                     "rollout_q_rows_T": lambda: vit_maps.rollout_chain(slab, 0, T)}
            t = timed(sides, args)
            for key in sides:
                t[key]["slab_bytes"] = slab.numel() * 4
                t[key]["slab_gbs"] = round(slab.numel() * 4 / (t[key]["ms"] * 1e-3) / 1e9, 1)
                case["kernel_" + key] = t[key]
            k = int(T * T * ratio)
            if k:
                work = torch.empty_like(slab)
                sides = {"copy": lambda: work.copy_(slab),
                         "copy_discard": lambda: vit_maps.attention_discard(work.copy_(slab), k),
                         "copy_eager_discard": lambda: eager_discard(work.copy_(slab), k)}
                t = timed(sides, args)
                nbytes = slab.numel() * 4 * 5 + depth * B * k * 4
                for key in ("copy_discard", "copy_eager_discard"):
                    t[key]["ms_without_copy"] = round(t[key]["ms"] - t["copy"]["ms"], 3)
                t["copy_discard"].update(k=k, bytes=nbytes, gbs=round(nbytes / (t["copy_discard"]["ms_without_copy"] * 1e-3) / 1e9, 1))
                t["speedup_vs_eager"] = round(t["copy_eager_discard"]["ms_without_copy"] / t["copy_discard"]["ms_without_copy"], 2)
                case["kernel_discard"] = t
                del work
            del slab
            torch.cuda.empty_cache()
            res["cases"].append(case)
        del model, x
        torch.cuda.empty_cache()
    print(json.dumps(res))


if __name__ == "__main__":
    main()
