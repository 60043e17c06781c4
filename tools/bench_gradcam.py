"""Grad-CAM throughput on the bf16 C2 encoder (random-init ResNeXt-50, E = 512) at B = 256, 224 x 224:
  (a) the reference's loop: one gradCAM call (forward + backward + act/grad + resize) per image;
  (b) gradCAM_pairs diagonal + bicubic resize to 224 x 224: one trunk pass, one contraction, one resize;
  (c) all pairs, 256 images x 2350 vocabulary words, unresized.
Device-event timing after warm-up; the Grad-CAM kernels' share comes from the library's per-class launch timing (the contraction
is class 'head', the resize and act/grad kernels 'other'; the trunk's classes are everything else).  Prints one JSON line.

    python tools/bench_gradcam.py [--batch 256] [--vocab 2350] [--iters 5] [--loop_images 32]"""
import argparse
import contextlib
import io
import json
import os
import sys

import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(ROOT, "multimodal-baby_amd"))

from multimodal import _hip as H                                      # noqa: E402
from multimodal.attention_maps import gradCAM, gradCAM_pairs          # noqa: E402
from multimodal.multimodal import VisionEncoder                       # noqa: E402

TRUNK_CLASSES = ("gemm", "gconv3x3", "stem7x7", "bn_finalize", "bn_add_relu", "bn_relu_maxpool", "avgpool", "gemm8w", "gemm_pro",
                 "bn_relu_apply")


def timed(fn, iters):
    torch.cuda.synchronize()
    a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    a.record()
    for _ in range(iters):
        fn()
    b.record()
    torch.cuda.synchronize()
    return a.elapsed_time(b) / iters


def profiled(fn):
    """-> {class: ms} of one call (per-launch event brackets: use for shares, not for wall time)."""
    torch.cuda.synchronize()
    H.prof_enable(True)
    fn()
    torch.cuda.synchronize()
    d = H.prof_collect()
    H.prof_enable(False)
    return d


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--batch", type=int, default=256)
    ap.add_argument("--vocab", type=int, default=2350)
    ap.add_argument("--iters", type=int, default=5)
    ap.add_argument("--loop_images", type=int, default=32, help="images timed in the per-image loop (a)")
    args = ap.parse_args()
    dev = torch.device("cuda:0")
    ns = argparse.Namespace(embedding_type="flat", embedding_dim=512, pretrained_cnn=False, cnn_model="resnext50_32x4d",
                            cnn_dino=False, vit_dino=False, finetune_cnn=False)
    torch.manual_seed(0)
    with contextlib.redirect_stdout(io.StringIO()):
        ve = VisionEncoder(ns)
    ve.to(dev).eval()
    ve.set_compute_dtype(torch.bfloat16)
    model = ve.model
    B, V = args.batch, args.vocab
    x = torch.randn(B, 3, 224, 224, device=dev)
    t_diag = torch.nn.functional.normalize(torch.randn(B, 512, device=dev), dim=1)
    t_vocab = torch.nn.functional.normalize(torch.randn(V, 512, device=dev), dim=1)
    hw, C = 49, 2048

    def fwd():
        with torch.no_grad():
            ve(x)

    def loop():
        for i in range(args.loop_images):
            gradCAM(model, x[i:i + 1], t_diag[i:i + 1], model.layer4, normalize_features=True)

    def diag():
        gradCAM_pairs(ve, x, t_diag, True, pairs="diagonal", resize=True)

    def allp():
        gradCAM_pairs(ve, x, t_vocab, True, pairs="all")

    for fn in (fwd, loop, diag, allp):                                 # warm-up: packing, workspaces, allocator
        fn()
    res = {"batch": B, "vocab": V}
    ms_fwd = timed(fwd, args.iters)
    ms_loop = timed(loop, max(1, args.iters // 2))
    ms_diag = timed(diag, args.iters)
    ms_all = timed(allp, args.iters)
    res["eval_forward_ms"] = round(ms_fwd, 3)
    res["a_loop"] = {"ms_per_image": round(ms_loop / args.loop_images, 3), "maps_per_s": round(args.loop_images / ms_loop * 1e3, 1)}
    for key, fn, ms, maps, flop_pairs, resize_bytes in (
            ("b_diagonal_resized", diag, ms_diag, B, B, B * 224 * 224 * 4),
            ("c_all_pairs", allp, ms_all, B * V, B * V, 0)):
        prof = profiled(fn)
        k_ms = prof["head"][0]
        o_ms = prof["other"][0]
        trunk_ms = sum(prof[c][0] for c in TRUNK_CLASSES if c in prof)
        flop = 2.0 * flop_pairs * hw * C                               # the contraction R (U adds N hw C, negligible)
        res[key] = {"ms": round(ms, 3), "maps_per_s": round(maps / ms * 1e3, 1),
                    "contraction_ms": round(k_ms, 3), "contraction_tflops": round(flop / (k_ms * 1e-3) / 1e12, 2) if k_ms else None,
                    "resize_and_other_ms": round(o_ms, 3),
                    "resize_write_gbs": round(resize_bytes / (o_ms * 1e-3) / 1e9, 1) if resize_bytes and o_ms else None,
                    "trunk_ms": round(trunk_ms, 3), "gradcam_share_of_wall": round((k_ms + o_ms) / ms, 3),
                    "contraction_gflop": round(flop / 1e9, 2), "resize_bytes": resize_bytes}
    print(json.dumps(res))


if __name__ == "__main__":
    main()
