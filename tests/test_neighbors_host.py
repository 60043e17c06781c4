"""CPU: the bookkeeping of multimodal/neighbors.py (nn_classify, same_category_matches, the pixel records, the CSV / JSON schemas and
the printed summaries) against a numpy restatement of the reference's analysis_cvcl/duplicates.py:594-612 and :795-838, fed with
precomputed (value, index) pairs -- the searches themselves are the GPU tests' subject."""
import csv
import json

import numpy as np

from multimodal import neighbors as N

CATS = ["apple", "ball", "cat", "dog", "egg"]


def _data(seed=0, per_eval=(3, 5, 2, 4, 1), per_train=(7, 0, 9, 4, 6), D=16):
    rng = np.random.default_rng(seed)
    eval_feats = {c: rng.standard_normal((n, D)).astype(np.float32) for c, n in zip(CATS, per_eval)}
    train_feats = {c: rng.standard_normal((n, D)).astype(np.float32) for c, n in zip(CATS, per_train) if n}
    eval_files = {c: [f"eval/{c}/{i}.jpg" for i in range(n)] for c, n in zip(CATS, per_eval)}
    train_files = {c: [f"train/{c}/{i}.jpg" for i in range(n)] for c, n in zip(CATS, per_train) if n}
    return eval_feats, train_feats, eval_files, train_files


def _cos(a, b):
    a = a.astype(np.float64) / np.maximum(np.linalg.norm(a.astype(np.float64), axis=1, keepdims=True), 1e-8)
    b = b.astype(np.float64) / np.maximum(np.linalg.norm(b.astype(np.float64), axis=1, keepdims=True), 1e-8)
    return a @ b.T


def _reference_classify(eval_feats, train_feats, eval_files, train_files):
    """duplicates.py:771-838 with numpy in place of torch; accuracies divided by the actual counts"""
    train_labels = np.concatenate([[label] * len(train_feats[label]) for label in train_feats.keys()])
    train_filenames = [f for label in train_feats.keys() for f in train_files[label]]
    train = np.concatenate(list(train_feats.values()), axis=0)
    matched, mismatched, rows, per_cat, pairs = [], [], [], {}, {}
    total = 0
    for cat in sorted(eval_feats):
        sims = _cos(eval_feats[cat], train)
        max_sims, max_idx = sims.max(axis=-1), sims.argmax(axis=-1)
        acc = 0
        for j, i in enumerate(max_idx):
            pairs[eval_files[cat][j]] = (max_sims[j], i)
            if train_labels[i] == cat:
                acc += 1
                matched.append(max_sims[j])
                rows.append([eval_files[cat][j], train_filenames[i], max_sims[j], "match"])
            else:
                mismatched.append(max_sims[j])
                rows.append([eval_files[cat][j], train_filenames[i], max_sims[j], "mismatch"])
        per_cat[cat] = acc / len(max_idx)
        total += acc
    return per_cat, total / sum(len(v) for v in eval_feats.values()), matched, mismatched, rows, pairs


def _flat(eval_feats, train_feats, eval_files, train_files):
    # deliberately NOT grouped by category on the evaluation side: the bookkeeping must group by itself
    order = np.random.default_rng(7).permutation(sum(len(v) for v in eval_feats.values()))
    ef = np.concatenate([eval_feats[c] for c in CATS])[order]
    el = [l for c in CATS for l in [c] * len(eval_feats[c])]
    en = [f for c in CATS for f in eval_files[c]]
    el, en = [el[i] for i in order], [en[i] for i in order]
    tf = np.concatenate(list(train_feats.values()))
    tl = [c for c in train_feats for _ in range(len(train_feats[c]))]
    tn = [f for c in train_feats for f in train_files[c]]
    return ef, el, en, tf, tl, tn


def test_nn_classify_matches_the_reference_bookkeeping():
    data = _data()
    per_cat, total, matched, mismatched, rows, pairs = _reference_classify(*data)
    ef, el, en, tf, tl, tn = _flat(*data)
    # the (value, index) pairs a search over all training frames returns, in the flat order of the evaluation frames
    nearest = (np.array([pairs[f][0] for f in en]), np.array([pairs[f][1] for f in en]))
    res = N.nn_classify(None, el, None, tl, en, tn, nearest=nearest)
    assert res["per_category"] == per_cat and list(res["per_category"]) == sorted(CATS)
    assert res["total"] == total
    # the reference lists frames category by category, in each category's own order; the shuffled input keeps that order per category
    key = lambda r: (r[0].split("/")[1], r[0])
    assert sorted(map(tuple, res["rows"]), key=key) == sorted(map(tuple, rows), key=key)
    assert [r[0].split("/")[1] for r in res["rows"]] == sorted(r[0].split("/")[1] for r in rows)
    assert sorted(res["matched_sims"]) == sorted(matched) and sorted(res["mismatched_sims"]) == sorted(mismatched)
    assert len(res["matched_train_filenames"]) == len(res["matched_eval_filenames"]) == len(matched)
    assert 0 < len(matched) < len(rows)                   # both kinds occur ("ball" has no training frame: always a mismatch)
    assert res["per_category"]["ball"] == 0.0


def test_same_category_matches_restates_the_per_category_argmax():
    eval_feats, train_feats, eval_files, train_files = _data(seed=1)
    want = []
    for cat in sorted(eval_feats):                        # duplicates.py:596-612 (train x eval matrix, argmax over its columns)
        if cat not in train_feats:
            want += [{"train_frame": None, "eval_frame": f, "max_cosine_sim": None} for f in eval_files[cat]]
            continue
        sims = _cos(train_feats[cat], eval_feats[cat])
        for i in range(sims.shape[1]):
            want.append({"train_frame": train_files[cat][int(np.argmax(sims[:, i]))], "eval_frame": eval_files[cat][i],
                         "max_cosine_sim": float(np.max(sims[:, i]))})
    ef = np.concatenate([eval_feats[c] for c in CATS])
    el = [c for c in CATS for _ in range(len(eval_feats[c]))]
    en = [f for c in CATS for f in eval_files[c]]
    tf = np.concatenate(list(train_feats.values()))
    tl = [c for c in train_feats for _ in range(len(train_feats[c]))]
    tn = [f for c in train_feats for f in train_files[c]]
    sims = _cos(ef, tf)
    sims[np.array(el)[:, None] != np.array(tl)[None, :]] = -np.inf
    idx = np.where(np.isfinite(sims.max(axis=1)), sims.argmax(axis=1), -1)
    got = N.same_category_matches(None, el, None, tl, en, tn, nearest=(sims.max(axis=1), idx))
    assert got == want
    lines = N.matches_summary(got)
    s = np.array([m["max_cosine_sim"] for m in want if m["max_cosine_sim"] is not None])
    assert lines[0] == f"Proportion of max cosine sims between 0.7 and 0.8: {np.sum((s >= 0.7) & (s < 0.8)) / len(s)}"
    assert lines[2] == f"Proportion of max cosine sims between 0.9 and 1: {np.sum(s >= 0.9) / len(s)}"


def test_label_ids_are_shared_between_the_two_sides():
    q, b = N._label_ids(["b", "a", "zz"], ["zz", "zz", "a", "c"])
    assert q.dtype == np.int32 and q.tolist() == [1, 0, 3] and b.tolist() == [3, 3, 0, 2]


def test_outputs_have_the_reference_schemas(tmp_path):
    rows = [["e/a/0.jpg", "t/a/3.jpg", 0.987654321, "match"], ["e/b/0.jpg", "t/a/1.jpg", 0.5, "mismatch"]]
    N.write_matched_results(rows, tmp_path / "matched_results.csv")
    with open(tmp_path / "matched_results.csv") as f:
        got = list(csv.reader(f))
    assert got[0] == ["eval_filename", "train_filename", "cosine_sim", "matched"]
    assert got[1] == ["e/a/0.jpg", "t/a/3.jpg", "0.987654321", "match"] and got[2][3] == "mismatch" and len(got) == 3
    recs = N.pixel_records(["e0", "e1"], ["a", "b"], ["t0", "t1", "t2"], ["a", "a", "c"], np.array([0.0, 12.5]), np.array([1, 2]))
    assert [set(r) for r in recs] == [{"eval_frame", "eval_label", "min_label", "min_frame", "min_distance", "correct"}] * 2
    assert recs[0] == {"eval_frame": "e0", "eval_label": "a", "min_label": "a", "min_frame": "t1", "min_distance": 0.0, "correct": True}
    assert recs[1]["correct"] is False and recs[1]["min_frame"] == "t2"
    json.dumps(recs)
    res = {"per_category": {"a": 1.0, "b": 0.0}, "total": 0.5, "matched_sims": [0.987654321], "mismatched_sims": [0.5]}
    lines = N.classify_summary(res)
    assert lines[:3] == ["Accuracy for a: 1.0", "Accuracy for b: 0.0", "Total accuracy: 0.5"]
    assert lines[-2] == "Proportion of matched cosine sims > 0.95: 0.5" and lines[-1] == "Proportion of matched cosine sims > 0.9: 0.5"


def test_pixel_weights_and_synthetic_sets():
    assert N.pixel_weights((0.229, 0.224, 0.225)) == [1.0 / (255.0 * 0.229), 1.0 / (255.0 * 0.224), 1.0 / (255.0 * 0.225)]
    a, b = N.synthetic_sets(3), N.synthetic_sets(3)
    assert a["planted"] == b["planted"] and bool((a["eval"] == b["eval"]).all()) and a["train"].dtype == b["eval"].dtype
    kinds = [k for _, _, k in a["planted"]]
    assert kinds.count("duplicate") == kinds.count("near") == 4
    for e, t, kind in a["planted"]:
        assert a["eval_labels"][e] == a["train_labels"][t]
        diff = (a["eval"][e].int() - a["train"][t].int()).abs()
        assert (int(diff.sum()) == 0) if kind == "duplicate" else (0 < int(diff.sum()) <= 6 and int(diff.max()) == 1)
