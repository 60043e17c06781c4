"""The caption scores (csrc/textgen_scores.hip, multimodal/textgen_eval.py) at the size of a validation epoch: a seeded corpus of
5 000 examples, 5 references each, about 12 tokens per sentence, vocabulary 2 350 (the generator of tests/textgen_scores_common.py:
a reference is a noisy copy of the hypothesis, a slice of another hypothesis, or random words).

    python tools/bench_textgen_scores.py [--repeats 7] [--window-ms 200] [--examples 5000] [--host-repeats 3]

``evaluate`` on the strings (interning on the host, the upload, three launches, four sorts, the read-back) and ``ops.caption_scores``
on tensors that are on the device already, by tools/timing.py: ms per call, median [min, max], the two taking their windows in turn.
The float64 restatement of tests/textgen_scores_common.py on the same strings, one host core, by the host clock.  The largest
relative difference between the two sets of scores is printed beside the times.  Prints one JSON line."""
import argparse
import json
import os
import statistics
import sys
import time

import timing

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(ROOT, "multimodal-baby_amd"))
sys.path.insert(0, os.path.join(ROOT, "tests"))

REFS, TOKENS, V = 5, 12, 2350


def main(argv=None):
    ap = argparse.ArgumentParser()
    timing.add_arguments(ap)
    ap.add_argument("--examples", type=int, default=5000)
    ap.add_argument("--host-repeats", type=int, default=3, help="runs of the host restatement")
    a = ap.parse_args(argv)
    import torch

    import textgen_scores_common as TC
    from multimodal import ops
    from multimodal.textgen_eval import evaluate
    if not torch.cuda.is_available():
        sys.exit("bench_textgen_scores: no GPU")
    dev = torch.device("cuda:0")
    hyps, refs = TC.corpus(0, a.examples, V, max_refs=REFS, ref_tokens=TOKENS)
    text = lambda s: " ".join(f"w{t}" for t in s)                                # noqa: E731
    hyp_text, ref_text = [text(h) for h in hyps], [[text(s) for s in r] for r in refs]
    tensors = TC.tensors(hyps, refs, dev)

    host = []
    for _ in range(a.host_repeats):
        t0 = time.perf_counter()
        want = TC.evaluate(ref_text, hyp_text)
        host.append(time.perf_counter() - t0)
    got = evaluate(ref_text, hyp_text)
    on_ids, arrays = ops.caption_scores(*tensors, V)
    res = {"shape": {"examples": a.examples, "references": sum(map(len, refs)), "tokens": sum(len(s) for r in refs for s in r) + sum(map(len, hyps)),
                     "vocab_size": V, "df_entries": [k.numel() for k, _ in arrays["df"]]},
           "scores": got,
           "max_rel_diff": max(abs(got[k] - want[k]) / abs(want[k]) for k in TC.NAMES),
           "ids_equal_strings_max_rel_diff": max(abs(got[k] - on_ids[k]) / abs(got[k]) for k in TC.NAMES)}
    for k, r in timing.measure({"evaluate": lambda: evaluate(ref_text, hyp_text), "caption_scores": lambda: ops.caption_scores(*tensors, V)},
                               **timing.keywords(a)).items():
        res[k] = {**timing.entry(r), "calls": r["calls"]}
    res["host_restatement"] = {"ms": statistics.median(host) * 1e3, "min_ms": min(host) * 1e3, "max_ms": max(host) * 1e3}
    res["host_over_evaluate"] = res["host_restatement"]["ms"] / res["evaluate"]["ms"]
    res.update({"repeats": a.repeats, "window_ms": a.window_ms, "device": torch.cuda.get_device_name(0)})
    print(json.dumps(res))


if __name__ == "__main__":
    main()
