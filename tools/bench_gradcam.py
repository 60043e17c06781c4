"""Grad-CAM throughput on the bf16 C2 encoder (random-init ResNeXt-50, E = 512) at B = 256, 224 x 224:
  (a) the reference's loop: one gradCAM call (forward + backward + act/grad + resize) per image;
  (b) gradCAM_pairs diagonal + bicubic resize to 224 x 224: one trunk pass, one contraction, one resize;
  (c) all pairs, 256 images x 2350 vocabulary words, unresized.
Timed by tools/timing.py (ms per call, median [min, max], the three forms in turn); the Grad-CAM kernels' share comes from the
library's per-class launch timing (the contraction
is class 'head', the resize and act/grad kernels 'other'; the trunk's classes are everything else).  Prints one JSON line.

    python tools/bench_gradcam.py [--batch 256] [--vocab 2350] [--repeats 7] [--window-ms 200] [--loop_images 32]"""
import argparse
import contextlib
import io
import json
import os
import sys

import torch

import timing

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(ROOT, "multimodal-baby_amd"))

from multimodal import _hip as H                                      # noqa: E402
from multimodal.attention_maps import gradCAM, gradCAM_pairs          # noqa: E402
from multimodal.multimodal import VisionEncoder                       # noqa: E402

TRUNK_CLASSES = ("gemm", "gconv3x3", "stem7x7", "bn_finalize", "bn_add_relu", "bn_relu_maxpool", "avgpool", "gemm8w", "gemm_pro",
                 "bn_relu_apply")


def profiled(fn):
    """-> {class: ms} of one call (per-launch event brackets: use for shares, not for wall time)."""
    torch.cuda.synchronize()
    H.prof_enable(True)
    fn()
    torch.cuda.synchronize()
    d = H.prof_collect()
    H.prof_enable(False)
    return d


def main(argv=None):
    ap = argparse.ArgumentParser()
    ap.add_argument("--batch", type=int, default=256)
    ap.add_argument("--vocab", type=int, default=2350)
    timing.add_arguments(ap)
    ap.add_argument("--loop_images", type=int, default=32, help="images timed in the per-image loop (a)")
    args = ap.parse_args(argv)
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

    res = {"batch": B, "vocab": V}
    t = timing.measure({"fwd": fwd, "loop": loop, "diag": diag, "all": allp}, **timing.keywords(args))     # (a), (b), (c) in turn
    res.update(timing.entry(t["fwd"], "eval_forward_ms", digits=3))
    res["a_loop"] = {**timing.entry(t["loop"], "ms_per_image", 1.0 / args.loop_images, 3),
                     "maps_per_s": round(args.loop_images / t["loop"]["ms"] * 1e3, 1)}
    for key, fn, side, maps, flop_pairs, resize_bytes in (
            ("b_diagonal_resized", diag, t["diag"], B, B, B * 224 * 224 * 4),
            ("c_all_pairs", allp, t["all"], B * V, B * V, 0)):
        ms = side["ms"]
        prof = profiled(fn)
        k_ms = prof["head"][0]
        o_ms = prof["other"][0]
        trunk_ms = sum(prof[c][0] for c in TRUNK_CLASSES if c in prof)
        flop = 2.0 * flop_pairs * hw * C                               # the contraction R (U adds N hw C, negligible)
        res[key] = {**timing.entry(side, digits=3), "maps_per_s": round(maps / ms * 1e3, 1),
                    "contraction_ms": round(k_ms, 3), "contraction_tflops": round(flop / (k_ms * 1e-3) / 1e12, 2) if k_ms else None,
                    "resize_and_other_ms": round(o_ms, 3),
                    "resize_write_gbs": round(resize_bytes / (o_ms * 1e-3) / 1e9, 1) if resize_bytes and o_ms else None,
                    "trunk_ms": round(trunk_ms, 3), "gradcam_share_of_wall": round((k_ms + o_ms) / ms, 3),
                    "contraction_gflop": round(flop / 1e9, 2), "resize_bytes": resize_bytes}
    print(json.dumps(res))


if __name__ == "__main__":
    main()
