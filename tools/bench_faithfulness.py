"""Map faithfulness (multimodal/map_faithfulness.py) at 256 frames of 224 x 224, steps = 14: the two kernels against their eager torch
compositions, and the whole deletion_insertion call.

    python tools/bench_faithfulness.py [--frames 256] [--size 224] [--steps 14] [--chunk 256] [--repeats 7] [--window-ms 200]
    python tools/bench_faithfulness.py --quick           # toy sizes: proves that the tool runs, the figures mean nothing
    python tools/bench_faithfulness.py --kernels-only    # no encoder: the run to put under `rocprofv3 --kernel-trace --stats`

- ``cvcl_map_ranks`` (pixel_ranks, ReLU-like maps with 60 % zeros) against ``torch.sort(descending, stable)`` plus the inverse scatter;
- ``cvcl_map_perturb`` (one chunk of deletion items into a reused buffer, zero and tensor baselines) against the ``torch.where``
  composition on gathered frames and ranks, with the bytes each moves at least (ranks + frames [+ baseline] read, frames written);
- ``deletion_insertion`` as a whole on a random-init CVCL model (flat ResNeXt-50, precision 32), the same chunks through
  ``encode_image`` alone, and the share of the call spent outside the encoder.
Timed by tools/timing.py: ms per call, median [min, max], the sides alternating; prints one JSON line."""
import argparse
import json
import os
import sys

import timing

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(ROOT, "multimodal-baby_amd"))


def main(argv=None):
    ap = argparse.ArgumentParser()
    ap.add_argument("--frames", type=int, default=256)
    ap.add_argument("--size", type=int, default=224)
    ap.add_argument("--steps", type=int, default=14)
    ap.add_argument("--chunk", type=int, default=256)
    timing.add_arguments(ap)
    ap.add_argument("--quick", action="store_true", help="4 frames of 64 x 64, 2 steps, short windows")
    ap.add_argument("--kernels-only", action="store_true", help="no model, no torch yardsticks (the profiled run)")
    a = ap.parse_args(argv)
    if a.quick:
        a.frames, a.size, a.steps, a.chunk, a.repeats, a.window_ms = 4, 64, 2, 6, 2, 2.0
    import numpy as np
    import torch
    from multimodal import map_faithfulness as F
    if not torch.cuda.is_available():
        sys.exit("bench_faithfulness: no GPU")
    dev = torch.device("cuda:0")
    g = torch.Generator(device=dev).manual_seed(0)
    N, S, HW = a.frames, a.size, a.size * a.size
    images = torch.randn(N, 3, S, S, device=dev, generator=g)
    maps = (torch.randn(N, S, S, device=dev, generator=g) - 0.25).clamp_(min=0)          # ReLU-like: 60 % exact zeros
    res = {"frames": N, "size": S, "steps": a.steps, "chunk": a.chunk, "repeats": a.repeats, "window_ms": a.window_ms,
           "zero_share_of_maps": float((maps == 0).float().mean())}
    kw = timing.keywords(a)

    # ---- ranks ---------------------------------------------------------------------------------------------------------------------
    flat = maps.view(N, HW)
    position = torch.arange(HW, device=dev).expand(N, HW).contiguous()

    def torch_ranks():
        order = torch.sort(flat, dim=1, descending=True, stable=True).indices
        return torch.empty_like(order).scatter_(1, order, position)

    ranks = F.pixel_ranks(maps)
    sides = {"map_ranks_ms": lambda: F.pixel_ranks(maps)}
    if not a.kernels_only:
        sides["torch_sort_scatter_ms"] = torch_ranks
        res["ranks_equal_torch"] = bool(torch.equal(ranks.view(N, HW).long(), torch_ranks()))
    r = timing.entries(timing.measure(sides, **kw))
    r["map_ranks_us_per_map"] = r["map_ranks_ms"] * 1e3 / N
    if not a.kernels_only:
        r["speedup_vs_torch"] = r["torch_sort_scatter_ms"] / r["map_ranks_ms"]
    res["ranks"] = r

    # ---- perturb: one chunk of deletion items -------------------------------------------------------------------------------------
    n = min(a.chunk, N)
    item_map = np.arange(n, dtype=np.int32)
    item_count = np.full(n, HW // 3, dtype=np.int32)
    item_mode = np.zeros(n, dtype=np.int32)
    baseline = F.gaussian_blur(images)
    buf = torch.empty(n, 3, S, S, device=dev)
    idx = torch.from_numpy(item_map).to(dev).long()
    count = torch.from_numpy(item_count).to(dev).view(n, 1, 1, 1)
    zero = torch.zeros((), device=dev)

    def torch_where(base):
        top = ranks[idx].unsqueeze(1) < count
        return torch.where(top, zero if base is None else base[idx], images[idx])

    sides = {"perturb_zero_ms": lambda: F.perturb(images, None, ranks, None, item_map, item_count, item_mode, out=buf),
             "perturb_tensor_ms": lambda: F.perturb(images, baseline, ranks, None, item_map, item_count, item_mode, out=buf)}
    if not a.kernels_only:
        sides["torch_where_zero_ms"] = lambda: torch_where(None)
        sides["torch_where_tensor_ms"] = lambda: torch_where(baseline)
        res["perturb_equal_torch"] = bool(torch.equal(F.perturb(images, baseline, ranks, None, item_map, item_count, item_mode),
                                                      torch_where(baseline)))
    r = timing.entries(timing.measure(sides, **kw))
    frame_bytes = 3.0 * HW * 4
    r["perturb_zero_GBps"] = n * (HW * 4 + 2 * frame_bytes) / (r["perturb_zero_ms"] * 1e-3) / 1e9
    r["perturb_tensor_GBps"] = n * (HW * 4 + 3 * frame_bytes) / (r["perturb_tensor_ms"] * 1e-3) / 1e9
    if not a.kernels_only:
        r["speedup_vs_torch_zero"] = r["torch_where_zero_ms"] / r["perturb_zero_ms"]
        r["speedup_vs_torch_tensor"] = r["torch_where_tensor_ms"] / r["perturb_tensor_ms"]
    res["perturb"] = r
    res["blur"] = timing.entries(timing.measure({"gaussian_blur_ms": lambda: F.gaussian_blur(images)}, **kw))

    # ---- the whole call -------------------------------------------------------------------------------------------------------------
    if not a.kernels_only:
        from multimodal.alignment import build_model
        lit = build_model(argparse.Namespace(checkpoint=None, random_init=True, precision="32", seed=0), dev)
        mm = lit.model
        targets = torch.randn(N, 512, device=dev, generator=g)
        n_items = 2 * (a.steps + 1) * N
        sizes = [min(a.chunk, n_items - s) for s in range(0, n_items, a.chunk)]
        frames = torch.randn(max(sizes), 3, S, S, device=dev, generator=g)

        def encoder_only():
            with torch.no_grad():
                for c in sizes:
                    mm.encode_image(frames[:c])

        sides = {"deletion_insertion_ms": lambda: F.deletion_insertion(mm, images, targets, maps, steps=a.steps, chunk=a.chunk),
                 "encoder_only_ms": encoder_only}
        r = timing.entries(timing.measure(sides, warmup=1, **kw))
        r["encoder_passes"] = len(sizes)
        r["perturbed_frames"] = n_items
        r["share_outside_encoder"] = 1.0 - r["encoder_only_ms"] / r["deletion_insertion_ms"]
        res["call"] = r
    print(json.dumps(res))


if __name__ == "__main__":
    main()
