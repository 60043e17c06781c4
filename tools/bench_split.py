"""The 32-split precision (fp32 storage, split-bf16 products in the ResNeXt trunk's convolutions) against the exact-fp32 and
bf16 modes: C2 at B = 256, 224^2, on bench.py's weights and batch, all three modes timed in one process
(tools/timing.py: ms per step, median [min, max]).  Prints ONE JSON line:
ms/step and pairs/s per mode, logits_rel / cosine / loss_abs of 32-split vs 32 at bench's noise batch and at the conditioned point
(bench.structured_parity's setting), and the per-class kernel times of one 32-split step.

    python tools/bench_split.py [--batch 256 --repeats 7 --window-ms 200]
"""
import argparse
import json
import os
import sys

import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "multimodal-baby_amd"))

import bench                                                          # noqa: E402
import timing                                                         # noqa: E402
from multimodal import _hip as H                                      # noqa: E402


def conditioned(lit, ve, batch_size, dev, gamma3=0.25):
    """32-split vs 32 at bench.structured_parity's well-conditioned point (every bn3.weight = gamma3, smooth structured frames)."""
    evalb = bench.structured_batch_on_device(batch_size, seed=4242, device=dev)
    bn3 = [m.bn3 for m in ve.model.modules() if hasattr(m, "bn3")]
    keep = [b.weight.detach().clone() for b in bn3]
    try:
        with torch.no_grad():
            for b in bn3:
                b.weight.fill_(gamma3)
        return bench.logits_vs_fp32(lit, evalb, "32-split")
    finally:
        with torch.no_grad():
            for b, g in zip(bn3, keep):
                b.weight.copy_(g)


def main(argv=None):
    ap = argparse.ArgumentParser()
    ap.add_argument("--batch", type=int, default=256)
    timing.add_arguments(ap)
    args = ap.parse_args(argv)
    dev = torch.device("cuda:0")
    lit, ve, opt = bench.build_model("c2", dev, "32")
    batch = bench.synthetic_batch_on_device(args.batch, seed=0, device=dev) + (None,)

    rnd = lambda d: {k: float(f"{v:.4g}") for k, v in d.items()}      # noqa: E731
    parity = {"noise": rnd(bench.logits_vs_fp32(lit, batch, "32-split")), "conditioned": rnd(conditioned(lit, ve, args.batch, dev))}

    def step():
        opt.zero_grad(set_to_none=True)
        out = lit.training_step(batch, 0)
        out["loss"].backward()
        opt.step()

    res = {}
    ve.model.enable_trunk_stream(dev, inputs="ready", n_streams=2)    # bench.py's schedule
    for p in ("32-split", "32", "bf16"):
        lit.set_precision(p)
        # (a precision switch re-packs the weights on the next step, so the modes are measured one after the other)
        t = timing.measure({p: step}, **timing.keywords(args))[p]
        res[p] = {**timing.entry(t, "ms_per_step", digits=3), "pairs_per_s": round(args.batch / t["ms"] * 1e3, 1)}
    ve.model.enable_trunk_stream(dev, inputs=None)

    lit.set_precision("32-split")
    step()
    torch.cuda.synchronize()
    H.prof_enable(True)
    step()
    torch.cuda.synchronize()
    kern = {k: round(v[0], 3) for k, v in H.prof_collect().items() if v[1]}
    H.prof_enable(False)
    print(json.dumps({"config": "c2", "batch": args.batch, "repeats": args.repeats, "window_ms": args.window_ms, "modes": res,
                      "split_over_fp32_step": round(res["32-split"]["ms_per_step"] / res["32"]["ms_per_step"], 3),
                      "split_vs_fp32": parity, "split_kernel_ms_by_class": kern}))


if __name__ == "__main__":
    main()
