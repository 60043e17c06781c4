"""Retrieval ranks (multimodal/retrieval.py retrieval_ranks = nearest_cosine with keys + cvcl_rank_cosine) at N x N, D = 512, single-target
keys (query i's target is base row perm[i]): N = 10 000 and 50 000.

    python tools/bench_retrieval.py [--n 10000,50000] [--dim 512] [--block 2048] [--repeats 7] [--window-ms 200]
    python tools/bench_retrieval.py --kernels-only      # the run to put under `rocprofv3 --kernel-trace --stats`

- ``retrieval_ranks`` (both passes) and ``cvcl_rank_cosine`` alone (the thresholds given), with the rate of each against the fp32 MFMA
  peak for the 2 Nq Nb D products of ONE pass (``retrieval_ranks`` walks the base rows twice);
- against the eager torch composition on the same GPU: F.normalize both sides, ``q @ b.T`` in blocks of ``--block`` queries, the
  comparison against the gathered target column, the sum (it writes block x Nb similarities per block; ties are not resolved by index).
Timed by tools/timing.py: us per call, median [min, max], the sides alternating; prints one JSON line."""
import argparse
import json
import os
import sys

import timing

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(ROOT, "multimodal-baby_amd"))

PEAK_F32_MFMA_TFLOPS = 157.3                          # MI355X, fp32 matrix


def main(argv=None):
    ap = argparse.ArgumentParser()
    ap.add_argument("--n", default="10000,50000")
    ap.add_argument("--dim", type=int, default=512)
    ap.add_argument("--block", type=int, default=2048, help="queries per matmul of the torch composition")
    timing.add_arguments(ap)
    ap.add_argument("--kernels-only", action="store_true", help="no torch yardstick (the profiled run)")
    a = ap.parse_args(argv)
    import torch
    import torch.nn.functional as F
    from multimodal import _hip as H
    from multimodal import retrieval as R
    if not torch.cuda.is_available():
        sys.exit("bench_retrieval: no GPU")
    dev = torch.device("cuda:0")
    g = torch.Generator(device=dev).manual_seed(0)
    D = a.dim
    res = {"dim": D, "block": a.block, "repeats": a.repeats, "window_ms": a.window_ms, "peak_f32_mfma_tflops": PEAK_F32_MFMA_TFLOPS}
    lib = H.lib()
    for N in (int(v) for v in a.n.split(",") if v):
        b = torch.randn(N, D, device=dev, generator=g)
        target = torch.randperm(N, device=dev, generator=g)
        q = b[target] + 0.5 * torch.randn(N, D, device=dev, generator=g)          # a model of some quality: the target is close
        base_keys = torch.arange(N, device=dev, dtype=torch.int32)
        query_keys = target.int()
        rank, thr_cos, thr_idx = R.retrieval_ranks(q, b, query_keys, base_keys)
        ws = torch.empty(lib.cvcl_rank_cosine_workspace_bytes(N, N, D), dtype=torch.uint8, device=dev)
        out = torch.empty_like(rank)

        def rank_only():
            H.check(lib.cvcl_rank_cosine(*H.rows(q), *H.rows(b), N, N, D, 1e-8, H.ptr(query_keys), H.ptr(base_keys), H.ptr(thr_cos),
                                         H.ptr(thr_idx), 0, 0, H.ptr(out), H.ptr(ws), ws.numel(), H.stream_ptr()), "cvcl_rank_cosine")

        def eager():
            qn, bn = F.normalize(q, dim=-1), F.normalize(b, dim=-1)
            out = []
            for s in range(0, N, a.block):
                c = qn[s:s + a.block] @ bn.T
                out.append((c > c.gather(1, target[s:s + a.block, None])).sum(dim=1))
            return torch.cat(out)

        sides = {"retrieval_ranks_us": lambda: R.retrieval_ranks(q, b, query_keys, base_keys), "rank_cosine_us": rank_only}
        if not a.kernels_only:
            sides["eager_torch_us"] = eager
        r = timing.entries(timing.measure(sides, **timing.keywords(a)), scale=1e3)
        flop = 2.0 * N * N * D
        r["rank_cosine_tflops"] = flop / (r["rank_cosine_us"] * 1e-6) / 1e12
        r["rank_cosine_of_peak"] = r["rank_cosine_tflops"] / PEAK_F32_MFMA_TFLOPS
        r["retrieval_ranks_tflops"] = 2.0 * flop / (r["retrieval_ranks_us"] * 1e-6) / 1e12
        r["retrieval_ranks_of_peak"] = r["retrieval_ranks_tflops"] / PEAK_F32_MFMA_TFLOPS
        if not a.kernels_only:
            r["speedup_vs_eager_torch"] = r["eager_torch_us"] / r["retrieval_ranks_us"]
            same = eager() == rank
            r["ranks_equal_eager_share"] = float(same.float().mean())          # (ties and fp32 sum order may move a few)
        r["median_rank"] = float(rank.double().median()) + 1.0
        res[f"n{N}"] = r
        del b, q, ws
        torch.cuda.empty_cache()
    print(json.dumps(res))


if __name__ == "__main__":
    main()
