"""Nearest-neighbour searches (multimodal/neighbors.py) against the eager torch composition of the reference's own lines on the
same GPU (analysis_cvcl/duplicates.py), at the leakage check's sizes: Nq = 2200 evaluation frames, Nb = 10 000 and 50 000 training
frames, D = 2048 features, frames of 3 x 224 x 224.

    python tools/bench_neighbors.py [--nq 2200] [--nb 10000,50000] [--pixel-nb 10000,50000] [--repeats 7] [--window-ms 200]
    python tools/bench_neighbors.py --kernels-only      # the run to put under `rocprofv3 --kernel-trace --stats`

- feature search: ``nearest_cosine`` over all base rows, and grouped in 22 categories (one launch sequence);
  yardstick: F.cosine_similarity(eval[:, None, :], train[None, :, :], dim=-1) + torch.max / argmax (duplicates.py:805-809), timed on
  one category's 100 queries and scaled to Nq (the broadcast intermediate is 100 x Nb x D fp32: 41 GB at Nb = 50 000), and the
  per-category form of :568-577 (100 queries against Nb / 22 rows, normalised first), scaled by 22.
- pixel search: ``nearest_pixels`` on uint8 frames; yardstick: the per-query loop over base batches of 256 normalised fp32 frames
  resident on the device, torch.sum(torch.abs(eval_img - train_images), dim=(1, 2, 3)) + min / argmin (:988-1002), timed on
  ``--pixel-slice`` queries (default 2) and scaled to Nq.
Timed by tools/timing.py: ms per call, median [min, max], a search and its yardsticks alternating; prints one JSON line.  Also
reported: the fraction of the 155 TF fp32 MFMA rate the feature search reaches (2 Nq Nb D flops over its whole time) and the
v_sad_u8 lane-instructions per second of the pixel search (Nq Nb C HW / 4 over its whole time)."""
import argparse
import json
import os
import sys

import timing

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(ROOT, "multimodal-baby_amd"))

MFMA_F32_PEAK = 155e12


def main(argv=None):
    ap = argparse.ArgumentParser()
    ap.add_argument("--nq", type=int, default=2200)
    ap.add_argument("--nb", default="10000,50000")
    ap.add_argument("--pixel-nb", default="10000,50000")
    ap.add_argument("--dim", type=int, default=2048)
    ap.add_argument("--size", type=int, default=224)
    timing.add_arguments(ap)
    ap.add_argument("--pixel-slice", type=int, default=2)
    ap.add_argument("--kernels-only", action="store_true", help="no torch yardsticks (the profiled run)")
    a = ap.parse_args(argv)
    import torch
    import torch.nn.functional as F
    from multimodal import neighbors as N
    if not torch.cuda.is_available():
        sys.exit("bench_neighbors: no GPU")
    dev = torch.device("cuda:0")
    g = torch.Generator(device=dev).manual_seed(0)
    Nq, D, S = a.nq, a.dim, a.size
    res = {"nq": Nq, "dim": D, "size": S, "repeats": a.repeats, "window_ms": a.window_ms}

    q = torch.randn(Nq, D, device=dev, generator=g)
    qg = (torch.arange(Nq, device=dev) % 22).int()
    for Nb in (int(v) for v in a.nb.split(",") if v):
        b = torch.randn(Nb, D, device=dev, generator=g)
        bg = (torch.arange(Nb, device=dev) % 22).int()
        n = min(100, Nq)

        def eager_all():
            sims = F.cosine_similarity(q[:n, None, :], b[None, :, :], dim=-1)
            return torch.max(sims, dim=-1).values, torch.argmax(sims, dim=-1)

        def eager_category():
            tb, eb = F.normalize(b[:Nb // 22], dim=-1), F.normalize(q[:n], dim=-1)
            sims = F.cosine_similarity(tb[:, None, :], eb[None, :, :], dim=-1)
            return sims.max(dim=0).values, sims.argmax(dim=0)

        r = {}
        sides = {"ms": lambda: N.nearest_cosine(q, b), "grouped22_ms": lambda: N.nearest_cosine(q, b, qg, bg)}       # side = output key
        if not a.kernels_only:
            try:
                eager_all()
                sides["eager_slice_ms"] = eager_all
            except torch.OutOfMemoryError:
                r["eager_scaled_ms"] = "not measured (out of memory)"
            torch.cuda.empty_cache()
            sides["eager_per_category_ms"] = eager_category
        r.update(timing.entries(timing.measure(sides, **timing.keywords(a))))
        ms, msg = r["ms"], r["grouped22_ms"]
        r.update({"queries_per_s": Nq / ms * 1e3, "fraction_of_fp32_mfma_peak": 2.0 * Nq * Nb * D / (ms * 1e-3) / MFMA_F32_PEAK,
                  "grouped22_queries_per_s": Nq / msg * 1e3})
        if "eager_slice_ms" in r:
            r["eager_slice_queries"] = n
            r["eager_scaled_ms"] = r["eager_slice_ms"] * Nq / n
            r["speedup_vs_eager"] = r["eager_scaled_ms"] / ms
        if not a.kernels_only:
            r["eager_22_categories_ms"] = r["eager_per_category_ms"] * 22
            r["grouped22_speedup_vs_eager"] = r["eager_22_categories_ms"] / msg
        res[f"cosine_nb{Nb}"] = r
        del b
        torch.cuda.empty_cache()

    qf = torch.randint(0, 256, (Nq, 3, S, S), device=dev, generator=g, dtype=torch.uint8)
    for Nb in (int(v) for v in a.pixel_nb.split(",") if v):
        bf = torch.randint(0, 256, (Nb, 3, S, S), device=dev, generator=g, dtype=torch.uint8)
        n = min(a.pixel_slice, Nq)
        r, bn = {}, None
        sides = {"ms": lambda: N.nearest_pixels(qf, bf)}
        if not a.kernels_only:
            try:
                bn = torch.empty(Nb, 3, S, S, device=dev)
                for s in range(0, Nb, 1024):
                    bn[s:s + 1024] = N.normalize_u8(bf[s:s + 1024])

                def eager():
                    out = []
                    for i in range(n):
                        eval_img = N.normalize_u8(qf[i:i + 1])[0]
                        best, best_j = float("inf"), -1
                        for s in range(0, Nb, 256):
                            distance = torch.sum(torch.abs(eval_img - bn[s:s + 256]), dim=(1, 2, 3))
                            cur = torch.min(distance)
                            j = torch.argmin(distance)
                            if cur < best:                   # (the reference's host comparison: one sync per batch)
                                best, best_j = cur, s + int(j)
                        out.append(best_j)
                    return out

                eager()
                sides["eager_slice_ms"] = eager
            except torch.OutOfMemoryError:
                r["eager_scaled_ms"] = "not measured (out of memory)"
        r.update(timing.entries(timing.measure(sides, **timing.keywords(a))))
        ms = r["ms"]
        r.update({"queries_per_s": Nq / ms * 1e3, "sad_lane_instructions_per_s": Nq * Nb * 3.0 * S * S / 4 / (ms * 1e-3),
                  "u8_bytes_compared_per_s": Nq * Nb * 3.0 * S * S / (ms * 1e-3)})
        if "eager_slice_ms" in r:
            r["eager_slice_queries"] = n
            r["eager_scaled_ms"] = r["eager_slice_ms"] * Nq / n
            r["speedup_vs_eager"] = r["eager_scaled_ms"] / ms
        res[f"pixels_nb{Nb}"] = r
        del bf, bn
        torch.cuda.empty_cache()
    print(json.dumps(res))


if __name__ == "__main__":
    main()
