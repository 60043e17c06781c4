"""Per-word Grad-CAM throughput of the captioning LM (random-init ResNeXt-50 + captioning LSTM, E = H = 512, V = 2350) at
B = 256 captions of L = 25 tokens, 224 x 224, fp32 trunk:
  (a) the straight port of the reference's loop (analysis_tools/multimodal_visualization.py:9-49), written here from the public
      operations alone: per image a Hook(layer4) with gradient, lit.calculate_ce_loss(tokenwise=True) at batch 1, then per word
      loss[0, p].backward(retain_graph=True) + gradCAM_with_act_and_grad(act, -grad); timed on --loop_images images, per map;
  (b) gradCAM_captions on the whole batch: one trunk pass, one multi-seed BPTT sweep, one contraction, one copy of the
      [B, L-1, 7, 7] result to the host (both sides end with their maps as numpy arrays).
Also: the kernel-class split of (b) (the library's per-launch event brackets: shares, not wall time), its launch count, and the seed
kernel alone at the sweep's largest step (rows = B (L - 1)) with its streamed bytes per second, on one buffer set (warm
Infinity Cache) and on four rotating sets that together exceed it (HBM).  Timed by tools/timing.py on
single calls: median [min, max] of --launches bracketed calls per side, (a) and (b) in turn.  Prints one JSON line.

    python tools/bench_caption_gradcam.py [--batch 256] [--length 25] [--launches 5] [--loop_images 4]"""
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

from multimodal import _hip as H                                                              # noqa: E402
from multimodal.attention_maps import Hook, gradCAM_captions, gradCAM_with_act_and_grad      # noqa: E402
from multimodal.multimodal import TextEncoder, VisionEncoder                                 # noqa: E402
from multimodal.multimodal_data_module import read_vocab                                     # noqa: E402
from multimodal.multimodal_lit import MultiModalLitModel                                     # noqa: E402


def main(argv=None):
    ap = argparse.ArgumentParser()
    ap.add_argument("--batch", type=int, default=256)
    ap.add_argument("--length", type=int, default=25)
    ap.add_argument("--launches", type=int, default=5, help="bracketed calls per side")
    ap.add_argument("--loop_images", type=int, default=4, help="images timed in the per-word loop (a)")
    args = ap.parse_args(argv)
    dev = torch.device("cuda:0")
    ns = argparse.Namespace(
        embedding_type="flat", embedding_dim=512, pretrained_cnn=False, cnn_model="resnext50_32x4d", cnn_dino=False, vit_dino=False,
        finetune_cnn=False, text_encoder="lstm", captioning=True, attention=False, attention_gate=False, crange=1, dropout_i=0.0,
        dropout_o=0.0, pos_embed_type="no_pos_embed", normalize_features=False, sim="max", temperature=0.07, fix_temperature=False,
        tie=True, bias=True, lr=1e-4, weight_decay=0.1, lambda_mm=0.5, lambda_lm=0.5, lambda_ar=0.0, optimize_unused=True,
        lr_scheduler=False, optimizer=torch.optim.AdamW)
    torch.manual_seed(0)
    with contextlib.redirect_stdout(io.StringIO()):
        ve = VisionEncoder(ns)
        lit = MultiModalLitModel(ve, TextEncoder(read_vocab(), 2048, ns), ns)
    lit.to(dev).eval()
    B, L = args.batch, args.length
    K = L - 1
    V = lit.language_model.text_encoder.vocab_size
    x = torch.randn(B, 3, 224, 224, device=dev)
    y = torch.randint(4, V, (B, L), device=dev)
    y[:, 0], y[:, -1] = 2, 3                                          # full-length captions: B (L - 1) maps
    n = torch.full((B,), L, dtype=torch.int64, device=dev)
    resnet = lit.vision_encoder.model

    def loop():
        saved = {k: p.requires_grad for k, p in lit.named_parameters()}
        for p in lit.parameters():
            p.requires_grad_(False)
        try:
            for i in range(args.loop_images):
                with Hook(resnet.layer4) as hook, torch.enable_grad():
                    loss = lit.calculate_ce_loss(y[i:i + 1], n[i:i + 1], x=x[i:i + 1], tokenwise=True)[0]
                    for p in range(K):
                        hook.data.grad = None
                        loss[0, p].backward(retain_graph=True)
                        gradCAM_with_act_and_grad(hook.activation.detach(), -hook.gradient).squeeze().cpu().numpy()
        finally:
            for k, p in lit.named_parameters():
                p.requires_grad_(saved[k])

    def batched():
        return gradCAM_captions(lit, x, y, n).cpu().numpy()         # on the host, where the loop's maps end as well

    sides = timing.measure({"loop": loop, "batched": batched}, calls=1, repeats=args.launches, warmup=1)      # single calls, in turn
    ms_loop, ms_batched = sides["loop"]["ms"], sides["batched"]["ms"]
    torch.cuda.synchronize()
    H.prof_enable(True)
    batched()
    torch.cuda.synchronize()
    prof = H.prof_collect()
    H.prof_enable(False)
    split = {c: {"ms": round(ms, 3), "launches": int(cnt)} for c, (ms, cnt) in prof.items() if cnt}

    # the seed kernel alone at the largest step of the sweep
    Hd = lit.language_model.text_encoder.hidden_dim
    rows = B * K
    f32 = dict(dtype=torch.float32, device=dev)
    gact, csave, c0 = torch.rand(B * K, 4 * Hd, **f32), torch.randn(B * K, Hd, **f32), torch.randn(B, Hd, **f32)
    d_out, dh, dc = torch.randn(B * K, Hd, **f32), torch.randn(rows, Hd, **f32), torch.randn(rows, Hd, **f32)
    dG, carry = torch.empty(rows, 4 * Hd, **f32), torch.empty(rows, Hd, **f32)
    lib = H.lib()

    def seeds():
        H.check(lib.cvcl_lstm_cell_bwd_seeds(H.ptr(gact), H.ptr(csave), H.ptr(c0), H.ptr(n), 0, H.ptr(d_out), H.ptr(dh), H.ptr(dc),
                                             H.ptr(dG), H.ptr(carry), B, K, Hd, rows, H.stream_ptr()), "cvcl_lstm_cell_bwd_seeds")

    # the same launch over SETS rotating buffer sets, together larger than the 256 MiB Infinity Cache: every launch finds its rows in HBM
    SETS = 4
    rot = [(torch.randn(rows, Hd, **f32), torch.randn(rows, Hd, **f32), torch.empty(rows, 4 * Hd, **f32), torch.empty(rows, Hd, **f32))
           for _ in range(SETS)]

    def seeds_rotating():
        for i in range(12):
            rh, rc, rg, rk = rot[i % SETS]
            H.check(lib.cvcl_lstm_cell_bwd_seeds(H.ptr(gact), H.ptr(csave), H.ptr(c0), H.ptr(n), 0, H.ptr(d_out), H.ptr(rh), H.ptr(rc),
                                                 H.ptr(rg), H.ptr(rk), B, K, Hd, rows, H.stream_ptr()), "cvcl_lstm_cell_bwd_seeds")

    kern = timing.measure({"warm": seeds, "rotating": seeds_rotating}, calls={"warm": 10, "rotating": 1}, repeats=max(5, args.launches), warmup=1)
    us_seed, us_cold = kern["warm"]["ms"] * 1e3, kern["rotating"]["ms"] * 1e3 / 12
    seed_bytes = rows * Hd * 4 * 8 + B * Hd * 4 * 7          # per row: dh, dc in; 4 gate gradients, dc, carry out; the captions' saved rows once
    maps = B * K
    res = {"batch": B, "length": L, "vocab": V, "maps": maps,
           "a_loop": {"images": args.loop_images, **timing.entry(sides["loop"], "ms_per_map", 1.0 / (args.loop_images * K), 4),
                      "maps_per_s": round(args.loop_images * K / ms_loop * 1e3, 1)},
           "b_batched": {**timing.entry(sides["batched"], digits=3), "maps_per_s": round(maps / ms_batched * 1e3, 1), "classes": split,
                         "launches": sum(v["launches"] for v in split.values())},
           "speedup_per_map": round((ms_loop / (args.loop_images * K)) / (ms_batched / maps), 1),
           "seed_kernel": {"rows": rows, "hidden": Hd, **timing.entry(kern["warm"], "us", 1e3, 2), "bytes": seed_bytes,
                           "gb_per_s": round(seed_bytes / (us_seed * 1e-6) / 1e9, 1),
                           "rotating_sets": SETS, "rotating_footprint_mb": round(SETS * rows * Hd * 4 * 7 / 1e6, 1),
                           **timing.entry(kern["rotating"], "rotating_us", 1e3 / 12, 2), "rotating_gb_per_s": round(seed_bytes / (us_cold * 1e-6) / 1e9, 1)}}
    print(json.dumps(res))


if __name__ == "__main__":
    main()
