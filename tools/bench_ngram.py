"""The n-gram baseline (csrc/ngram.hip, ngram.NGramModel) at the product shape: batches of B = 256 utterances of L = 25 positions,
V = 2350, N = 3 and 5, tables counted on a seeded Zipf corpus of 2^20 tokens (the generator of tests/ngram_common.py).

    python tools/bench_ngram.py [--repeats 7] [--window-ms 200] [--loop-batches 8] [--orders 3,5] [--tokens 1048576]

Per order: the three kernels alone (``ops.ngram_keys`` / ``ngram_ce_loss`` / ``ngram_probs``, the probabilities into a buffer
allocated once), ``update`` per batch (launch + the 4-byte read of the bad-id count), the table rebuild from the whole corpus'
pending keys (sort + run-length count per order; host clock, device drained at both ends), ``calculate_ce_loss`` against an eager
torch composition on the same device tensors (the packed keys by shifts, one ``torch.searchsorted`` per table and order, float64
logs; checked against the kernel's values), and ``calculate_ce_loss`` against the Python-loop restatement of
tests/ngram_common.py on ``loop-batches`` batches (host clock).  Device timings by tools/timing.py: us per call, median [min, max],
the sides of a comparison alternating.  Prints one JSON line."""
import argparse
import json
import math
import os
import statistics
import sys
import time

import timing

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(ROOT, "multimodal-baby_amd"))
sys.path.insert(0, os.path.join(ROOT, "tests"))

B, L, V = 256, 25, 2350


def main(argv=None):
    ap = argparse.ArgumentParser()
    timing.add_arguments(ap)
    ap.add_argument("--loop-batches", type=int, default=8)
    ap.add_argument("--orders", default="3,5")
    ap.add_argument("--tokens", type=int, default=1 << 20, help="tokens of the corpus the tables are counted on")
    a = ap.parse_args(argv)
    import numpy as np
    import torch
    import torch.nn.functional as F

    import ngram_common as NC
    from multimodal import ops
    from ngram import NGramModel
    if not torch.cuda.is_available():
        sys.exit("bench_ngram: no GPU")
    dev = torch.device("cuda:0")

    def measure_us(fns):
        """{name: fn} -> {name: {"us", "min_us", "max_us", "calls"}}"""
        return {k: {**timing.entry(r, "us", 1e3), "calls": r["calls"]} for k, r in timing.measure(fns, **timing.keywords(a)).items()}

    def host_clock(fn, prepare=lambda: None):
        out = []
        for _ in range(a.repeats):
            prepare()
            torch.cuda.synchronize()
            t0 = time.perf_counter()
            fn()
            torch.cuda.synchronize()
            out.append(time.perf_counter() - t0)
        return {"s": statistics.median(out), "min_s": min(out), "max_s": max(out)}

    n_batches = math.ceil(a.tokens / (B * (L + 1) / 2))          # lengths are uniform in [1, L]
    ty, tl = NC.corpus(0, V, B * n_batches, L)
    ey, el = NC.corpus(1, V, B * a.loop_batches, L)
    train = [(torch.from_numpy(ty[i * B:(i + 1) * B]).to(dev), torch.from_numpy(tl[i * B:(i + 1) * B]).to(dev)) for i in range(n_batches)]
    evals = [(torch.from_numpy(ey[i * B:(i + 1) * B]).to(dev), torch.from_numpy(el[i * B:(i + 1) * B]).to(dev)) for i in range(a.loop_batches)]
    y, y_len = evals[0]
    res = {"shape": {"B": B, "L": L, "V": V, "train_batches": n_batches, "train_tokens": int(tl.sum()),
                     "scored_tokens_per_batch": NC.n_tokens(el[:B], L)}}
    la, l1a = math.log(0.1), math.log(0.9)
    for N in (int(n) for n in a.orders.split(",")):
        r = {}
        model = NGramModel(N, V, device=dev)

        def fill():
            model._pending, model._gram, model._tables = [], [None] * N, None
            for yy, ll in train:
                model.update(yy, ll)

        r["rebuild"] = host_clock(model._rebuild, fill)
        tables = model._rebuild()
        bits = NC.key_bits(V)
        r["tables"] = {"grams": tables[2], "contexts": tables[5], "bytes": 16 * (tables[0].numel() + tables[3].numel())}
        scratch = NGramModel(N, V, device=dev)

        def update():
            scratch._pending.clear()
            scratch.update(y, y_len)

        probs = torch.empty(B, L - 1, V, device=dev)
        r.update(measure_us({"keys_kernel": lambda: ops.ngram_keys(y, y_len, N, V),
                             "ce_loss_kernel": lambda: ops.ngram_ce_loss(tables, N, V, la, l1a, y, y_len),
                             "probs_kernel": lambda: ops.ngram_probs(tables, N, V, la, l1a, y, y_len, out=probs),
                             "update": update}))
        gram = [(tables[0][tables[2][n]:tables[2][n + 1]], tables[1][tables[2][n]:tables[2][n + 1]]) for n in range(N)]
        ctx = [(tables[3][tables[5][n]:tables[5][n + 1]], tables[4][tables[5][n]:tables[5][n + 1]]) for n in range(N)]
        pos = torch.arange(L, device=dev)[None]

        def torch_loss():
            grams = [y]
            for n in range(1, N):
                grams.append(grams[-1] | (F.pad(y[:, :-n], (n, 0)) << (n * bits)))
            open_ = (pos >= 1) & (pos < y_len[:, None])
            inside = open_
            lp = torch.zeros(B, L, dtype=torch.float64, device=dev)
            for n in range(N - 1, 0, -1):
                (k, c), (ck, ct) = gram[n], ctx[n]
                gi = torch.searchsorted(k, grams[n]).clamp_max(len(k) - 1)
                ci = torch.searchsorted(ck, grams[n] >> bits).clamp_max(len(ck) - 1)
                here = open_ & (pos >= n)
                hit = here & (k[gi] == grams[n])
                lp = torch.where(hit, lp + ((c[gi].double().log() - ct[ci].double().log()) + l1a), lp)
                open_ = open_ & ~hit
                lp = torch.where(here & ~hit, lp + la, lp)
            k, c = gram[0]
            gi = torch.searchsorted(k, y).clamp_max(len(k) - 1)
            seen = torch.where(k[gi] == y, c[gi], torch.zeros_like(c[gi]))
            lp = torch.where(open_, lp + ((seen + 1).double().log() - (ctx[0][1][0] + V).double().log()), lp)
            return torch.where(inside, -lp, torch.zeros_like(lp))[:, 1:].float()

        want = model.calculate_ce_loss(y, y_len)
        r["torch_vs_hip_max_ulp"] = int(NC.ulp_distance(torch_loss().cpu().numpy(), want.cpu().numpy()).max())
        r.update(measure_us({"calculate_ce_loss": lambda: model.calculate_ce_loss(y, y_len), "torch_ce_loss": torch_loss}))
        r["torch_over_hip"] = r["torch_ce_loss"]["us"] / r["calculate_ce_loss"]["us"]
        # the Python loops on the host against the class on the same batches
        rest = NC.Model(N, V, [(k.cpu().numpy(), c.cpu().numpy()) for k, c in gram])
        t0 = time.perf_counter()
        loop = [rest.ce_loss(ey[i * B:(i + 1) * B], el[i * B:(i + 1) * B], 0.1)[0] for i in range(a.loop_batches)]
        t_loop = time.perf_counter() - t0
        torch.cuda.synchronize()
        t0 = time.perf_counter()
        mine = [model.calculate_ce_loss(yy, ll) for yy, ll in evals]
        mine = [m.cpu().numpy() for m in mine]
        t_hip = time.perf_counter() - t0
        r["loop"] = {"batches": a.loop_batches, "python_loop_s": t_loop, "calculate_ce_loss_s": t_hip, "speedup": t_loop / t_hip,
                     "max_ulp": int(max(NC.ulp_distance(p, q).max() for p, q in zip(loop, mine)))}
        res[f"N{N}"] = r
    res.update({"repeats": a.repeats, "window_ms": a.window_ms, "device": torch.cuda.get_device_name(0)})
    print(json.dumps(res))


if __name__ == "__main__":
    main()
