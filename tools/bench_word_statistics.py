"""The two word-statistics kernels (csrc/token_items.hip) against the eager torch compositions on the same device tensors, and the
reference-style per-token Python loop, at the product shape: B = 256 utterances of L = 25 positions, H = 512, V = 2350, K = 3000
(word, tag) keys with a Zipf-like key distribution (every utterance starts with the same <sos> key).

    python tools/bench_word_statistics.py [--repeats 7] [--window-ms 200] [--loop-batches 8]

Yardsticks: ``index_add_`` of the rows / the float64 losses / ones into the tables for the accumulate (not order-preserving: it
uses atomics), ``softmax(-1)`` + ``topk`` + ``gather`` for the top-k.  Timed by tools/timing.py: us per call, median [min, max],
the two sides in alternation.  GB/s over the bytes each kernel has to move (accumulate: n_valid rows of H floats and their losses read, the touched
table rows read and written; top-k: R V floats read, R (2 k + 1) values written).  The per-token loop -- one ``.item()`` and one
SumData ``+=`` per token, as analysis_tools/processing.py:326-331 of the reference -- is timed on ``loop-batches`` batches with the
host clock, next to the CSR build + accumulate launch of this repository on the same batches.  Prints one JSON line."""
import argparse
import json
import os
import sys
import time

import timing

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(ROOT, "multimodal-baby_amd"))

B, L, HD, V, K, TOP_K = 256, 25, 512, 2350, 3000, 5


def main(argv=None):
    ap = argparse.ArgumentParser()
    timing.add_arguments(ap)
    ap.add_argument("--loop-batches", type=int, default=8)
    a = ap.parse_args(argv)
    import numpy as np
    import torch
    from analysis_tools import processing as P
    from multimodal import ops
    if not torch.cuda.is_available():
        sys.exit("bench_word_statistics: no GPU")
    dev = torch.device("cuda:0")

    def measure_us(fns):
        """{name: fn} -> {name: {"us", "min_us", "max_us", "calls"}}"""
        return {k: {**timing.entry(r, "us", 1e3), "calls": r["calls"]} for k, r in timing.measure(fns, **timing.keywords(a)).items()}

    rng = np.random.default_rng(0)
    zipf = 1.0 / np.arange(1, K)
    zipf /= zipf.sum()

    def batch():
        """token ids [B, L] (0 = the <sos> key, the rest Zipf over the other K - 1 keys; the id stands for the whole key), lengths"""
        lens = rng.integers(3, L + 1, B)
        y = rng.choice(np.arange(1, K), size=(B, L), p=zipf)
        y[:, 0] = 0
        return y, lens

    N = B * L
    g = torch.Generator(device=dev).manual_seed(0)
    outputs = torch.randn(N, HD, device=dev, generator=g)
    loss = torch.rand(N, device=dev, generator=g) * 8
    y, lens = batch()
    tags = [["X"] * int(n) for n in lens]
    key_slots = {}
    csr = P.build_batch_csr(y, tags, L, key_slots)
    seg_ptr, rows, slot = (torch.from_numpy(c).to(dev) for c in csr)
    S, n_valid = len(csr[2]), len(csr[1])
    vector = torch.zeros(K, HD, device=dev)
    loss_sum = torch.zeros(K, dtype=torch.float64, device=dev)
    cnt = torch.zeros(K, dtype=torch.int64, device=dev)
    flat_rows = rows.long()
    flat_slot = torch.repeat_interleave(slot.long(), (seg_ptr[1:] - seg_ptr[:-1]).long())
    ones = torch.ones(n_valid, dtype=torch.int64, device=dev)

    def torch_accumulate():
        vector.index_add_(0, flat_slot, outputs[flat_rows])
        loss_sum.index_add_(0, flat_slot, loss[flat_rows].double())
        cnt.index_add_(0, flat_slot, ones)

    res = {"shape": {"B": B, "L": L, "H": HD, "V": V, "K": K, "segments": S, "n_valid": n_valid,
                     "largest_segment": int((seg_ptr[1:] - seg_ptr[:-1]).max())}}
    res.update(measure_us({"hip_accumulate": lambda: ops.token_items_accumulate(outputs, loss, seg_ptr, rows, slot, vector, loss_sum, cnt),
                           "torch_accumulate": torch_accumulate}))
    moved = n_valid * (HD * 4 + 4 + 4) + S * (2 * HD * 4 + 2 * 8 + 2 * 8 + 4) + (S + 1) * 4
    res["accumulate_GBps"] = moved / (res["hip_accumulate"]["us"] * 1e-6) / 1e9
    res["torch_accumulate_GBps"] = moved / (res["torch_accumulate"]["us"] * 1e-6) / 1e9

    logits = torch.randn(N, V, device=dev, generator=g) * 3
    labels = torch.from_numpy(y.reshape(-1) % V).to(dev)

    def torch_topk():
        p = logits.softmax(-1)
        t = p.topk(TOP_K, -1)
        return t, p.gather(1, labels[:, None])

    res.update(measure_us({"hip_topk": lambda: ops.token_topk(logits, labels, TOP_K), "torch_topk": torch_topk}))
    moved = N * V * 4 + N * 8 + N * (TOP_K * 12 + 4)
    res["topk_GBps"] = moved / (res["hip_topk"]["us"] * 1e-6) / 1e9
    res["torch_topk_GBps"] = moved / (res["torch_topk"]["us"] * 1e-6) / 1e9

    # the reference-style loop against CSR build + launch, on the same batches (host clock, device drained at both ends)
    batches = [batch() for _ in range(a.loop_batches)]
    out3, loss2 = outputs.view(B, L, HD), loss.view(B, L)
    torch.cuda.synchronize()
    t0 = time.perf_counter()
    items = {}
    for yb, lb in batches:
        for b in range(B):
            for idx, loss_, outputs_ in zip(yb[b, :lb[b]], loss2[b], out3[b]):
                key = P.Key(int(idx), "X")
                sd = P.SumData(1, loss_.item(), outputs_, None)
                items[key] = items[key] + sd if key in items else P.SumData(np.array(0), np.array(0.), torch.zeros(HD, device=dev), None) + sd
    items = {k: v.to_numpy() for k, v in items.items()}
    torch.cuda.synchronize()
    t_loop = time.perf_counter() - t0
    for t in (vector, loss_sum, cnt):
        t.zero_()
    t0 = time.perf_counter()
    slots = {}
    for yb, lb in batches:
        c = P.build_batch_csr(yb, [["X"] * int(n) for n in lb], L, slots)
        ops.token_items_accumulate(outputs, loss, *(torch.from_numpy(x).to(dev) for x in c), vector, loss_sum, cnt)
    host = (vector.cpu(), loss_sum.cpu(), cnt.cpu())
    t_hip = time.perf_counter() - t0
    same = all(np.array_equal(host[0][s].numpy(), items[k].vector) and float(host[1][s]) == float(items[k].loss) for k, s in slots.items())
    res["loop"] = {"batches": a.loop_batches, "per_token_loop_s": t_loop, "csr_and_launch_s": t_hip, "speedup": t_loop / t_hip,
                   "bitwise_equal": bool(same and len(slots) == len(items))}
    res.update({"repeats": a.repeats, "window_ms": a.window_ms, "device": torch.cuda.get_device_name(0)})
    print(json.dumps(res))


if __name__ == "__main__":
    main()
