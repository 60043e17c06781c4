"""GPU: the word-statistics kernels against CPU loops / float64, the analysis end to end against the reference's values of
tests/golden/word_statistics.npz, and the word_statistics.py script.

Bounds: the accumulate is bitwise (the CPU loop adds the same values in the same order in the same formats); probabilities are
held to 10 x the distance of torch's own fp32 CPU softmax from float64 on the same logits (measured 0.9e-7 .. 1.5e-7 of the
largest probability at these shapes), at least 1e-6; token losses to 2e-6 max(1, max|loss|) (test_lm_gpu.py); mean vectors to 1e-5
absolute (the LSTM outputs' bound, test_captioning_gpu.py)."""
import csv
import os
import subprocess
import sys

import numpy as np
import pytest
import torch

import word_statistics_common as WC
from conftest import ROOT
from test_word_statistics_fixture import TOPK_CASES

pytestmark = pytest.mark.gpu


# ----------------------------------------------------------------------------- accumulate
def _accumulate_case(Hd, seed):
    """Two batches of N = 700 rows over K = 50 running keys with non-zero tables; S = 37 segments per batch: one of 300 rows,
    several of one row, ~100 rows unreferenced, 13 slots untouched."""
    N, S, K = 700, 37, 50
    g = np.random.default_rng(seed)
    vector = g.standard_normal((K, Hd)).astype(np.float32)
    loss_sum = g.standard_normal(K) * 10
    cnt = g.integers(0, 1000, K).astype(np.int64)
    batches = []
    for _ in range(2):
        sizes = np.array([300] + [1] * 6 + list(g.integers(2, 12, S - 7)))
        perm = g.permutation(N)[:sizes.sum()]
        seg_ptr = np.concatenate(([0], np.cumsum(sizes))).astype(np.int32)
        rows = np.concatenate([np.sort(perm[a:b]) for a, b in zip(seg_ptr[:-1], seg_ptr[1:])]).astype(np.int32)
        slot = np.sort(g.permutation(K)[:S]).astype(np.int32)
        outputs = (g.standard_normal((N, Hd)) * np.exp(g.standard_normal((N, 1)) * 3)).astype(np.float32)     # magnitudes differ: order matters
        loss = (g.random(N) * 8).astype(np.float32)
        batches.append((outputs, loss, seg_ptr, rows, slot))
    assert sizes.sum() < N - 50
    return vector, loss_sum, cnt, batches


def _accumulate_cpu(vector, loss_sum, cnt, batches):
    vector, loss_sum, cnt = vector.copy(), loss_sum.copy(), cnt.copy()
    for outputs, loss, seg_ptr, rows, slot in batches:
        for s, k in enumerate(slot):
            for r in rows[seg_ptr[s]:seg_ptr[s + 1]]:
                vector[k] = vector[k] + outputs[r]                      # fp32, one row at a time
                loss_sum[k] = loss_sum[k] + np.float64(loss[r])
                cnt[k] += 1
    return vector, loss_sum, cnt


def _accumulate_gpu(dev, vector, loss_sum, cnt, batches):
    from multimodal import ops
    t = [torch.from_numpy(a.copy()).to(dev) for a in (vector, loss_sum, cnt)]
    for batch in batches:
        outputs, loss, seg_ptr, rows, slot = (torch.from_numpy(a).to(dev) for a in batch)
        ops.token_items_accumulate(outputs, loss, seg_ptr, rows, slot, *t)
    torch.cuda.synchronize()
    return [a.cpu().numpy() for a in t]


@pytest.mark.parametrize("Hd", [32, 48, 100])
def test_accumulate_is_the_in_order_sum(dev, Hd):
    vector, loss_sum, cnt, batches = _accumulate_case(Hd, seed=Hd)
    want = _accumulate_cpu(vector, loss_sum, cnt, batches)
    got = _accumulate_gpu(dev, vector, loss_sum, cnt, batches)
    for g_, w_ in zip(got, want):
        assert g_.dtype == w_.dtype and g_.tobytes() == w_.tobytes()
    touched = np.zeros(len(cnt), dtype=bool)
    for b in batches:
        touched[b[4]] = True
    assert 0 < (~touched).sum() and np.array_equal(got[0][~touched], vector[~touched]) and np.array_equal(got[2][~touched], cnt[~touched])
    assert not np.array_equal(got[0][touched], vector[touched])
    again = _accumulate_gpu(dev, vector, loss_sum, cnt, batches)
    assert all(a.tobytes() == b.tobytes() for a, b in zip(got, again))


def test_accumulate_wide_rows_and_malformed_entries(dev):
    """H = 600 spans three column blocks; a row index outside [0, N) and a slot outside [0, K) are left out, nothing else moves."""
    from multimodal import ops
    N, Hd, K = 40, 600, 6
    g = torch.Generator().manual_seed(3)
    outputs, loss = torch.randn(N, Hd, generator=g), torch.rand(N, generator=g)
    seg_ptr = torch.tensor([0, 3, 5, 6], dtype=torch.int32)
    rows = torch.tensor([1, 7, 99, 2, 3, 4], dtype=torch.int32)
    slot = torch.tensor([4, 77, 0], dtype=torch.int32)
    vector, ls, cnt = torch.zeros(K, Hd), torch.zeros(K, dtype=torch.float64), torch.zeros(K, dtype=torch.int64)
    d = [t.to(dev) for t in (outputs, loss, seg_ptr, rows, slot, vector, ls, cnt)]
    ops.token_items_accumulate(*d)
    want = torch.zeros(K, Hd)
    want[4] = (want[4] + outputs[1]) + outputs[7]
    want[0] = want[0] + outputs[4]
    assert torch.equal(d[5].cpu(), want) and d[7].cpu().tolist() == [1, 0, 0, 0, 2, 0]
    assert d[6].cpu().tolist() == [float(loss[4].double()), 0, 0, 0, float(loss[1].double() + loss[7].double()), 0]


# ----------------------------------------------------------------------------- top-k
@pytest.mark.parametrize("R,V,k", TOPK_CASES)
def test_topk(dev, R, V, k):
    from multimodal import ops
    logits, labels = WC.topk_logits(R, V, k, seed=R + V + k)
    want_p, want_i, p64, gap = WC.topk_reference(logits, k)
    assert gap > 1e-4
    bound, measured = WC.softmax_bound(logits)
    top_prob, top_idx, label_prob, probs = ops.token_topk(logits.to(dev), labels.to(dev), k, want_probs=True)
    want_label = torch.where(labels == 0, torch.zeros(R, dtype=torch.float64), p64.gather(1, labels[:, None]).squeeze(1))
    errs = (WC.err(top_prob, want_p), WC.err(label_prob, want_label), WC.err(probs, p64))
    print(f"({R}, {V}, {k}): torch fp32 softmax {measured:.2e}, bound {bound:.2e}; top_prob {errs[0]:.2e} label_prob {errs[1]:.2e} "
          f"probs {errs[2]:.2e}")
    assert top_idx.dtype == torch.int64 and torch.equal(top_idx.cpu(), want_i)
    assert max(errs) <= bound
    own = probs.cpu().gather(1, labels[:, None]).squeeze(1)                # (deep in the tail of V = 2350 a probability underflows to 0)
    assert torch.all(label_prob.cpu()[labels == 0] == 0) and torch.equal(label_prob.cpu()[labels != 0], own[labels != 0])
    assert torch.equal(top_prob, probs.gather(1, top_idx))                 # the listed values are the row's entries
    # a null probs pointer: the same results come back (all that can be observed of it from outside the kernel)
    tp2, ti2, lp2, none = ops.token_topk(logits.to(dev), labels.to(dev), k)
    assert none is None and torch.equal(tp2, top_prob) and torch.equal(ti2, top_idx) and torch.equal(lp2, label_prob)


def test_topk_ties_go_to_the_lower_index(dev):
    from multimodal import ops
    lg = torch.zeros(4, 300)
    lg[1, [250, 7, 130]] = 2.0
    lg[2] = torch.arange(300).remainder(3).float()
    lg[3, 299] = 1.0
    top_prob, top_idx, _lp, _ = ops.token_topk(lg.to(dev), torch.ones(4, dtype=torch.long, device=dev), 6)
    assert top_idx.cpu().tolist() == [[0, 1, 2, 3, 4, 5], [7, 130, 250, 0, 1, 2], [2, 5, 8, 11, 14, 17], [299, 0, 1, 2, 3, 4]]
    assert torch.all(top_prob[:, :-1] >= top_prob[:, 1:])


# ----------------------------------------------------------------------------- end to end on the fixture
@pytest.fixture(scope="module")
def fx():
    return WC.fixture()


@pytest.fixture(scope="module", params=["plain", "captioning"])
def run(request, fx, dev):
    from analysis_tools import processing as P
    z, batches, pos_tags = fx
    model, w = WC.toy_model(dev, request.param == "captioning")
    k = int(z["top_k"])
    return (request.param, w, P.get_model_items(model, batches, pos_tags), P.get_model_probs(model, batches, pos_tags),
            P.get_model_top_predictions(model, batches, pos_tags, top_k=k), P.get_model_losses_on_batches(model, batches))


def test_items_match_the_reference(fx, run):
    z, batches, pos_tags = fx
    name, w, items, _probs, _top, summed = run
    want_losses = z[f"{name}.losses"].double()
    tol = 2e-6 * max(1.0, float(want_losses.abs().max()))
    lens = torch.cat([b[2] for b in batches]).tolist()
    assert items.all_token_items is None and [len(l) for l in items.losses] == lens
    got = np.zeros(tuple(want_losses.shape))
    for r, l in enumerate(items.losses):
        got[r, :len(l)] = l
    d_loss = float((torch.from_numpy(got) - want_losses).abs().max())
    d_sum = float((summed.double().cpu() - want_losses.sum(1)).abs().max())
    print(f"{name}: token losses {d_loss:.2e} (allowed {tol:.2e}), summed {d_sum:.2e}")
    assert d_loss <= tol and d_sum <= 9 * tol                                     # (at most 9 tokens per utterance)
    for table, mine in (("token_pos_items", items.token_pos_items), ("token_items", items.token_items)):
        keys, cnt, loss, vec = WC.stored_items(z, name, table)
        assert [tuple(k) for k in mine] == keys                                   # the keys, sorted, majority tags included
        assert [int(v.cnt) for v in mine.values()] == cnt.tolist()
        mean_loss = np.array([float(v.mean_loss) for v in mine.values()])
        d_mean = float(np.abs(mean_loss - (loss / cnt).numpy()).max())
        mean_vec = np.stack([v.mean_vector for v in mine.values()])
        d_vec = float(np.abs(mean_vec.astype(np.float64) - (vec.double() / cnt[:, None]).numpy()).max())
        print(f"{name}.{table}: loss / cnt {d_mean:.2e} (allowed {tol:.2e}), mean_vector {d_vec:.2e} (allowed 1e-5)")
        assert d_mean <= tol and d_vec <= 1e-5
    assert all(v.loss.dtype == np.float64 and v.vector.dtype == np.float32 for v in items.token_pos_items.values())
    assert all(v.embedding is None for v in items.token_pos_items.values())
    table = w["embedding.weight"].numpy()
    assert all(np.array_equal(v.embedding, table[k.token_id]) for k, v in items.token_items.items())


def test_probs_and_top_predictions_match_the_reference(fx, run):
    z, batches, pos_tags = fx
    name, _w, _items, probs, top, _summed = run
    want = z[f"{name}.probs"].double()
    keys = list(zip(z[f"{name}.probs.token_id"].tolist(), z[f"{name}.probs.pos"].tolist()))
    assert [tuple(k) for k, _p in probs] == keys == [tuple(t[0]) for t in top]
    got = torch.from_numpy(np.stack([p for _k, p in probs]))
    lead = want.sum(1) == 0
    assert int(lead.sum()) == 12 and torch.all(got[lead] == 0)                    # the leading zero row of every utterance
    # the bound: torch's fp32 softmax against float64 on logits that give these probabilities
    bound, measured = WC.softmax_bound(want[~lead].log())
    e = WC.err(got, want)
    print(f"{name}: probs {e:.2e} (torch fp32 softmax {measured:.2e}, allowed {bound:.2e})")
    assert e <= bound
    k, exact = int(z["top_k"]), int(z["exact_k"])
    label_prob = torch.tensor([float(t[1]) for t in top], dtype=torch.float64)
    top_prob = torch.from_numpy(np.stack([t[2] for t in top])).double()
    top_idx = torch.from_numpy(np.stack([t[3] for t in top]))
    want_label = want.gather(1, torch.tensor([kk[0] for kk in keys])[:, None]).squeeze(1)
    assert WC.err(label_prob, want_label) <= bound and torch.all(label_prob[lead] == 0)
    order = want.sort(dim=1, descending=True, stable=True)
    scale = float(want.max())
    assert float((top_prob - order.values[:, :k]).abs().max()) <= bound * scale   # the k best values ...
    assert float((want.gather(1, top_idx) - top_prob).abs().max()) <= bound * scale          # ... at the indices listed with them
    assert all(len(set(r)) == k for r in top_idx.tolist())
    # the toy LMs are flat: ranks 3 .. 6 of a position come as close as 5e-5, so only the best exact + 1 are > 1e-4 apart
    assert exact == 2 and torch.equal(top_idx[:, :exact], order.indices[:, :exact])
    assert top_idx[lead].tolist() == [list(range(k))] * 12


def test_dict_batches_and_positions(fx, dev):
    """Dict batches give the tuples' results; iter_top_predictions names every entry's place, also when a tag list runs past
    its batch's columns and when the tag lists end before the utterances do."""
    from analysis_tools import processing as P
    z, batches, pos_tags = fx
    model, _w = WC.toy_model(dev, False)
    as_dicts = [{"x": x, "y": y, "y_len": n} for x, y, n, _raw in batches]
    a, b = P.get_model_items(model, batches, pos_tags), P.get_model_items(model, as_dicts, pos_tags)
    assert list(a.token_pos_items) == list(b.token_pos_items)
    assert all(np.array_equal(u.vector, v.vector) and u.loss == v.loss and u.cnt == v.cnt
               for u, v in zip(a.token_pos_items.values(), b.token_pos_items.values()))
    tags = [list(t) for t in pos_tags[:9]]                                        # the last three utterances have no tags
    tags[7] = tags[7] + ["X"] * 5                                                 # 11 tags in a batch of 6 columns
    got = list(P.iter_top_predictions(model, as_dicts, tags, top_k=3))
    want = [(u, l) for u, t in enumerate(tags) for l in range(min(len(t), 9 if u < 7 else 6))]
    assert [(u, l) for u, l, *_rest in got] == want and len(P.get_model_top_predictions(model, batches, tags, top_k=3)) == len(want)
    ys = torch.cat([torch.nn.functional.pad(bt[1], (0, 9 - bt[1].shape[1])) for bt in batches])
    assert all(key == P.Key(int(ys[u, l]), tags[u][l]) for u, l, key, *_rest in got)


# ----------------------------------------------------------------------------- the script
def test_word_statistics_script(tmp_path):
    out = tmp_path / "ws"
    r = subprocess.run([sys.executable, os.path.join(ROOT, "word_statistics.py"), "--random_init", "--dataset", "synthetic", "--split",
                        "val", "--batch_size", "8", "--top_k", "3", "--out", str(out)], capture_output=True, text=True, timeout=170)
    assert r.returncode == 0, r.stdout[-2000:] + r.stderr[-2000:]
    with open(out / "token_items.csv") as f:
        rows = list(csv.reader(f))
    assert rows[0] == ["token", "pos", "cnt", "mean_loss", "ppl"]
    vectors, losses = np.load(out / "token_vectors.npy"), np.load(out / "losses.npy")
    assert vectors.shape == (len(rows) - 1, 512) and np.isfinite(vectors).all()
    assert losses.shape == (8, 5) and np.all(losses[:, 0] == 0) and np.all(losses[:, 1:] > 0)      # 8 utterances of <sos> w w w <eos>
    assert sum(int(r_[2]) for r_ in rows[1:]) == 40 and {r_[1] for r_ in rows[1:]} == {"X"}
    assert all(float(r_[4]) == min(np.exp(float(r_[3])), 99999.99) for r_ in rows[1:])
    with open(out / "top_predictions.csv") as f:
        pred = list(csv.reader(f))
    assert pred[0] == ["utterance", "position", "token", "pos", "label_prob", "top1", "top1_prob", "top2", "top2_prob", "top3", "top3_prob"]
    assert len(pred) - 1 == 40 and [p[:2] for p in pred[1:6]] == [["0", str(l)] for l in range(5)]
    assert all(float(p[6]) >= float(p[8]) >= float(p[10]) for p in pred[1:])
