"""CPU: the bookkeeping of multimodal/neighbors.py's weighted k-NN classification (knn_classify, its printed lines and
top_k_matches.csv), fed with precomputed ``neighbours`` and ``votes`` -- the search and the vote themselves are the GPU tests'
subject.  The expected values are a numpy restatement: float64 cosines, a stable sort by (cosine descending, index ascending),
float64 class sums of exp(cos / T), the arg-max with the lowest class on a tie."""
import csv

import numpy as np

from multimodal import neighbors as N

CATS = ["apple", "ball", "cat", "dog", "egg", "fig", "gnu"]


def _sets(seed=0, per_eval=(3, 5, 2, 4, 1, 2, 3), per_train=(7, 0, 9, 4, 6, 3, 5), D=16):
    """shuffled evaluation frames (the bookkeeping must group by itself); "ball" has no training frame"""
    rng = np.random.default_rng(seed)
    el = [c for c, n in zip(CATS, per_eval) for _ in range(n)]
    tl = [c for c, n in zip(CATS, per_train) for _ in range(n)]
    order = rng.permutation(len(el))
    el = [el[i] for i in order]
    en = [f"eval/{c}/{i}.jpg" for i, c in enumerate(el)]
    tn = [f"train/{c}/{i}.jpg" for i, c in enumerate(tl)]
    return rng.standard_normal((len(el), D)).astype(np.float32), el, en, rng.standard_normal((len(tl), D)).astype(np.float32), tl, tn


def _cos(a, b):
    a = a.astype(np.float64) / np.maximum(np.linalg.norm(a.astype(np.float64), axis=1, keepdims=True), 1e-8)
    b = b.astype(np.float64) / np.maximum(np.linalg.norm(b.astype(np.float64), axis=1, keepdims=True), 1e-8)
    return a @ b.T


def _lists(ef, tf, k):
    sims = _cos(ef, tf)
    idx = np.argsort(-sims, axis=1, kind="stable")[:, :k]
    cos = np.take_along_axis(sims, idx, axis=1)
    if k > tf.shape[0]:                                    # slots beyond the base rows: -inf / -1
        pad = k - tf.shape[0]
        cos = np.concatenate([cos, np.full((len(ef), pad), -np.inf)], axis=1)
        idx = np.concatenate([idx, np.full((len(ef), pad), -1)], axis=1)
    return cos.astype(np.float32), idx.astype(np.int64)


def _votes(cos, idx, train_ids, C, T):
    scores = np.zeros((len(cos), C))
    for i in range(len(cos)):
        for c, j in zip(cos[i], idx[i]):
            if j >= 0:
                scores[i, train_ids[j]] += np.exp(float(c) / T) if T > 0 else 1.0
    pred = np.where((idx >= 0).any(axis=1), scores.argmax(axis=1), -1)
    return scores.astype(np.float32), pred.astype(np.int64)


def test_knn_classify_bookkeeping_from_precomputed_lists_and_votes():
    ef, el, en, tf, tl, tn = _sets()
    k, T = 4, 0.07
    names = sorted(set(el) | set(tl))
    _, train_ids = N._label_ids(el, tl)
    cos, idx = _lists(ef, tf, k)
    scores, pred = _votes(cos, idx, train_ids, len(names), T)
    res = N.knn_classify(None, el, None, tl, k=k, temperature=T, eval_filenames=en, train_filenames=tn, neighbours=(cos, idx),
                         votes=(scores, pred))
    assert res["k"] == k and res["temperature"] == T
    # categories in sorted order, frames in their given order, k rows per frame with ranks 1..k in list order
    want_rows = []
    for cat in sorted(set(el)):
        for j in range(len(el)):
            if el[j] == cat:
                want_rows += [[en[j], r + 1, tn[idx[j, r]], float(cos[j, r]), tl[idx[j, r]]] for r in range(k)]
    assert res["rows"] == want_rows and len(res["rows"]) == k * len(el)
    # accuracies divide by the actual counts
    hit = np.array([names[p] == l for p, l in zip(pred, el)])
    assert list(res["per_category"]) == sorted(set(el))
    for cat in set(el):
        mine = hit[np.array(el) == cat]
        assert res["per_category"][cat] == mine.sum() / len(mine)
    assert res["total"] == hit.sum() / len(el) and 0 < hit.sum() < len(el)
    assert res["per_category"]["ball"] == 0.0               # no training frame of that class: it cannot be predicted
    # top-5: the true class is among the five largest scores that are not zero
    top5 = 0
    for j in range(len(el)):
        order = sorted(range(len(names)), key=lambda c: (-float(scores[j, c]), c))[:5]
        top5 += any(names[c] == el[j] and scores[j, c] > 0 for c in order)
    assert res["top5_total"] == top5 / len(el) and res["total"] <= res["top5_total"] < 1.0
    lines = N.knn_summary(res)
    assert lines[0] == f"4-NN accuracy for apple: {res['per_category']['apple']}"
    assert lines[-2] == f"4-NN total accuracy (T = 0.07): {res['total']}" and lines[-1] == f"4-NN top-5 accuracy: {res['top5_total']}"


def test_top5_counts_only_the_five_best_classes_and_short_lists_give_fewer_rows():
    el, tl = ["c6"], [f"c{i}" for i in range(8)]
    cos = np.array([[0.9, 0.8, 0.7, 0.6, 0.5, 0.4, 0.3, -np.inf]], dtype=np.float32)
    idx = np.array([[0, 1, 2, 3, 4, 5, 6, -1]], dtype=np.int64)
    scores = np.array([[8, 7, 6, 5, 4, 3, 2, 0]], dtype=np.float32)
    res = N.knn_classify(None, el, None, tl, k=8, neighbours=(cos, idx), votes=(scores, np.array([0])))
    assert res["top5_total"] == 0.0 and res["total"] == 0.0                 # c6 is the seventh class by score
    assert [r[1] for r in res["rows"]] == [1, 2, 3, 4, 5, 6, 7] and res["rows"][6][2:] == ["6", float(np.float32(0.3)), "c6"]
    res = N.knn_classify(None, ["c4"], None, tl, k=8, neighbours=(cos, idx), votes=(scores, np.array([0])))
    assert res["top5_total"] == 1.0 and res["total"] == 0.0
    # a class without a vote is not a prediction, even among fewer than five classes
    res = N.knn_classify(None, ["b"], None, ["a", "b"], k=1, neighbours=(cos[:, :1], idx[:, :1]),
                         votes=(np.array([[1.0, 0.0]], dtype=np.float32), np.array([0])))
    assert res["top5_total"] == 0.0
    # no neighbour at all: pred -1 is a miss
    res = N.knn_classify(None, ["a"], None, ["a", "b"], k=1, neighbours=(np.array([[-np.inf]], dtype=np.float32), np.array([[-1]])),
                         votes=(np.zeros((1, 2), dtype=np.float32), np.array([-1])))
    assert res["total"] == 0.0 and res["rows"] == []


def test_k1_majority_vote_equals_nn_classify():
    ef, el, en, tf, tl, tn = _sets(seed=3)
    names = sorted(set(el) | set(tl))
    _, train_ids = N._label_ids(el, tl)
    cos, idx = _lists(ef, tf, 1)
    one = N.nn_classify(None, el, None, tl, en, tn, nearest=(cos[:, 0], idx[:, 0]))
    res = N.knn_classify(None, el, None, tl, k=1, temperature=0, eval_filenames=en, train_filenames=tn, neighbours=(cos, idx),
                         votes=_votes(cos, idx, train_ids, len(names), 0))
    assert res["per_category"] == one["per_category"] and list(res["per_category"]) == list(one["per_category"])
    assert res["total"] == one["total"]
    assert [[r[0], r[2], r[3]] for r in res["rows"]] == [r[:3] for r in one["rows"]] and {r[1] for r in res["rows"]} == {1}


def test_top_k_matches_csv(tmp_path):
    rows = [["e/a/0.jpg", 1, "t/a/3.jpg", 0.987654321, "a"], ["e/a/0.jpg", 2, "t/b/1.jpg", 0.5, "b"]]
    N.write_top_k_matches(rows, tmp_path / "top_k_matches.csv")
    with open(tmp_path / "top_k_matches.csv") as f:
        got = list(csv.reader(f))
    assert got[0] == ["eval_filename", "rank", "train_filename", "cosine_sim", "train_label"]
    assert got[1] == ["e/a/0.jpg", "1", "t/a/3.jpg", "0.987654321", "a"] and got[2][1] == "2" and len(got) == 3
