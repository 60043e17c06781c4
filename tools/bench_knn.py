"""k-nearest-neighbour search and weighted vote (multimodal/neighbors.py knn_cosine / knn_vote) at the leakage check's sizes: Nq = 2200
evaluation frames, Nb = 10 000 and 50 000 training frames, D = 2048 features, k in {1, 20, 200}.

    python tools/bench_knn.py [--nq 2200] [--nb 10000,50000] [--k 1,20,200] [--repeats 7] [--window-ms 200]
    python tools/bench_knn.py --kernels-only      # the run to put under `rocprofv3 --kernel-trace --stats`

- ``knn_cosine`` against ``nearest_cosine`` at the same shape: the price of the lists;
- ``knn_cosine`` against the eager torch composition on the same GPU: F.normalize both sides, matmul in blocks of 256 queries, topk
  (it writes 256 x Nb similarities per block);
- ``knn_vote`` (C = 1000 classes, T = 0.07) against one_hot-and-sum in torch: (one_hot(labels[idx]) * exp(cos / T)[..., None]).sum(1)
  and argmax;
- the worst case for the lists at the test's small shape (130 x 1500 x 64, k = 64): base rows in ascending similarity, where every
  tile's candidates enter, against the same rows shuffled.
Timed by tools/timing.py: ms per call, median [min, max], the sides of a comparison alternating; prints one JSON line."""
import argparse
import json
import os
import sys

import timing

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(ROOT, "multimodal-baby_amd"))


def main(argv=None):
    ap = argparse.ArgumentParser()
    ap.add_argument("--nq", type=int, default=2200)
    ap.add_argument("--nb", default="10000,50000")
    ap.add_argument("--k", default="1,20,200")
    ap.add_argument("--dim", type=int, default=2048)
    ap.add_argument("--classes", type=int, default=1000)
    timing.add_arguments(ap)
    ap.add_argument("--kernels-only", action="store_true", help="no torch yardsticks (the profiled run)")
    a = ap.parse_args(argv)
    import torch
    import torch.nn.functional as F
    from multimodal import neighbors as N
    if not torch.cuda.is_available():
        sys.exit("bench_knn: no GPU")
    dev = torch.device("cuda:0")
    g = torch.Generator(device=dev).manual_seed(0)
    Nq, D, C, T = a.nq, a.dim, a.classes, 0.07
    ks = [int(v) for v in a.k.split(",") if v]
    res = {"nq": Nq, "dim": D, "classes": C, "repeats": a.repeats, "window_ms": a.window_ms}

    def measure(sides):
        """{output key: fn} -> {key, min_key, max_key of every side}, the sides alternating"""
        return timing.entries(timing.measure(sides, **timing.keywords(a)))

    q = torch.randn(Nq, D, device=dev, generator=g)
    for Nb in (int(v) for v in a.nb.split(",") if v):
        b = torch.randn(Nb, D, device=dev, generator=g)
        labels = torch.randint(0, C, (Nb,), device=dev, generator=g)
        r = {}
        for k in ks:
            cos, idx = N.knn_cosine(q, b, k)

            def eager_topk():
                qn, bn = F.normalize(q, dim=-1), F.normalize(b, dim=-1)
                out = [torch.topk(qn[s:s + 256] @ bn.T, k, dim=1) for s in range(0, Nq, 256)]
                return torch.cat([o.values for o in out]), torch.cat([o.indices for o in out])

            def eager_vote():
                w = torch.exp(cos / T)
                scores = (F.one_hot(labels[idx], C) * w[..., None]).sum(dim=1)
                return scores, scores.argmax(dim=1)

            sides = {"nearest_cosine_ms": lambda: N.nearest_cosine(q, b), "knn_cosine_ms": lambda: N.knn_cosine(q, b, k)}
            votes = {"knn_vote_ms": lambda: N.knn_vote(cos, idx, labels, C, T)}
            if not a.kernels_only:
                sides["eager_topk_ms"], votes["eager_vote_ms"] = eager_topk, eager_vote
            rk = {**measure(sides), **measure(votes)}
            rk["over_nearest_cosine"] = rk["knn_cosine_ms"] / rk["nearest_cosine_ms"]
            if not a.kernels_only:
                rk["speedup_vs_eager_topk"] = rk["eager_topk_ms"] / rk["knn_cosine_ms"]
                rk["vote_speedup_vs_eager"] = rk["eager_vote_ms"] / rk["knn_vote_ms"]
            r[f"k{k}"] = rk
        res[f"nb{Nb}"] = r
        del b
        torch.cuda.empty_cache()

    # the worst case: every candidate enters (tests/test_knn_gpu.py::test_order_adversaries)
    nq, nb, d, k = 130, 1500, 64, 64
    q0 = torch.randn(d, device=dev, generator=g)
    qs = q0[None, :] + 0.1 * torch.randn(nq, d, device=dev, generator=g)
    asc = torch.linspace(0.0, 3.0, nb, device=dev)[:, None] * q0[None, :] + torch.randn(nb, d, device=dev, generator=g)
    shuffled = asc[torch.randperm(nb, device=dev, generator=g)]
    res["adversary_130x1500x64_k64"] = measure({"ascending_ms": lambda: N.knn_cosine(qs, asc, k), "shuffled_ms": lambda: N.knn_cosine(qs, shuffled, k),
                                                "nearest_cosine_ms": lambda: N.nearest_cosine(qs, asc)})
    print(json.dumps(res))


if __name__ == "__main__":
    main()
