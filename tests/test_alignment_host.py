"""CPU: the float64 restatement of tests/alignment_common.py against the reference's own values (tests/golden/alignment.npz, written
by tools/gen_golden_alignment.py) at 5e-6 relative, and the host side of multimodal/alignment.py: the interleave order of
combined_sims, the CSV layouts (x outer, y inner), the kitty mapping, the seeded frame sampling and the p value."""
import csv
import json

import numpy as np
import pytest
import torch

import alignment_common as AC
from conftest import load_golden

REL = 5e-6


def _rel(a, b):
    a, b = np.asarray(a, dtype=np.float64), np.asarray(b, dtype=np.float64)
    return float(np.abs(a - b).max() / np.abs(b).max())


def _g():
    return {k: (v.numpy() if torch.is_tensor(v) else v) for k, v in load_golden("alignment").items()}


def test_golden_inputs_are_the_seeded_ones():
    g = _g()
    feats, labels, text = AC.golden_inputs()
    assert np.array_equal(g["features"], feats) and np.array_equal(g["labels"], labels) and np.array_equal(g["text_features"], text)
    assert feats.shape == (157, 64) and text.shape == (7, 64) and feats.dtype == np.float32
    sizes = np.bincount(labels, minlength=7)
    assert sizes.min() == 1 and len(set(sizes.tolist())) == 7                # unequal classes, one singleton


def test_restatement_matches_the_reference_values():
    g = _g()
    feats, labels, text = g["features"], g["labels"], g["text_features"]
    means = g["mean_image_features"]
    assert _rel(AC.class_means64(feats, labels, 7), means) <= REL
    assert _rel(AC.cosine64(means), g["image_sims"]) <= REL
    assert _rel(AC.cosine64(text), g["text_sims"]) <= REL
    assert _rel(AC.cosine64(means, text), g["image_text_sims"]) <= REL
    assert _rel(AC.cosine64(AC.interleave(means, text)), g["combined_sims"]) <= REL
    assert _rel(AC.cosine64(means), g["rs_cosine_matrix"]) <= REL
    assert _rel(AC.dissim64(means), g["rs_cosine_dissim_matrix"]) <= REL
    assert _rel(AC.triu_items(AC.cosine64(means)), g["rs_strict_upper_tri_items"]) <= REL
    assert _rel(AC.paired_l2_64(means, text), g["paired_distances"]) <= REL
    r, p, n = g["pearson"]
    assert n == 21 and abs(AC.rsa64(AC.cosine64(means), AC.cosine64(text)) - r) <= REL * abs(r)
    assert abs(AC.rsa64(AC.dissim64(means), AC.dissim64(text)) - g["rs_rsa"][0]) <= REL * abs(g["rs_rsa"][0])
    # a dissimilarity is an affine map of the similarity: the same correlation
    assert abs(g["rs_rsa"][0] - r) <= 1e-5


def test_pearson_condition_of_the_gpu_tests_holds_on_the_fixture():
    """sigma_min >= 0.05 and the reference's own fp32 loop is inside 4 delta / sigma_min"""
    g = _g()
    m64 = AC.class_means64(g["features"], g["labels"], 7)
    ti, tt = AC.triu_items(AC.cosine64(m64)), AC.triu_items(AC.cosine64(g["text_features"]))
    bound, sigma = AC.pearson_bound(64, ti, tt)
    assert sigma >= 0.05
    assert abs(g["pearson"][0] - AC.pearson64(ti, tt)[0]) <= bound


def test_pearson64_constant_side_is_nan_and_moments():
    x, y = np.array([1.0, 2.0, 4.0, 8.0]), np.array([3.0, 3.0, 3.0, 3.0])
    assert np.isnan(AC.pearson64(x, y)[0]) and np.isnan(AC.pearson64(y, x)[0])
    r, n, mx, my, vx, vy = AC.pearson64(x, 2 * x + 1)
    assert n == 4 and abs(r - 1.0) < 1e-15 and mx == 3.75 and abs(vx - np.var(x)) < 1e-15 and abs(vy - 4 * np.var(x)) < 1e-12


def test_interleave_order():
    from multimodal import alignment as A
    img = torch.arange(12, dtype=torch.float32).view(4, 3)
    txt = 100 + torch.arange(12, dtype=torch.float32).view(4, 3)
    c = A.interleave(img, txt)
    assert c.shape == (8, 3) and c.is_contiguous()
    for i in range(4):                                   # image_0, text_0, image_1, text_1, ... for any C, not 22
        assert torch.equal(c[2 * i], img[i]) and torch.equal(c[2 * i + 1], txt[i])
    assert np.array_equal(c.numpy(), AC.interleave(img.numpy(), txt.numpy()))
    with pytest.raises(ValueError):
        A.interleave(img, txt[:3])


def _fake_result(n, D=5, seed=3):
    rng = np.random.default_rng(seed)
    return {"mean_image_features": rng.standard_normal((n, D)).astype(np.float32),
            "image_sims": rng.standard_normal((n, n)).astype(np.float32), "text_sims": rng.standard_normal((n, n)).astype(np.float32),
            "image_text_sims": rng.standard_normal((n, n)).astype(np.float32),
            "combined_sims": rng.standard_normal((2 * n, 2 * n)).astype(np.float32), "pearson_r": 0.25, "pearson_p": 0.5, "n_pairs": 3}


def test_written_files_headers_and_row_order(tmp_path):
    from multimodal import alignment as A
    words = ["ball", "car", "kitty"]
    res = _fake_result(3)
    feats, text = np.zeros((9, 5), dtype=np.float32), np.ones((3, 5), dtype=np.float32)
    dist = np.array([1.5, 2.5, 3.5], dtype=np.float32)
    summary = A.write_results(str(tmp_path), "cvc", 0, words, feats, text, res, dist, accuracies={"ball": 90.0, "car": 50.0, "kitty": 20.0})
    assert np.load(tmp_path / "cvc_all_image_features_seed_0.npy").shape == (9, 5)
    assert np.array_equal(np.load(tmp_path / "cvc_mean_image_features_seed_0.npy"), res["mean_image_features"])
    assert np.load(tmp_path / "cvc_all_text_features_seed_0.npy").shape == (3, 5)
    with open(tmp_path / "cvc_joint_embeddings_sims_seed_0.csv") as f:
        assert f.readline() == "image_sims,text_sims,eval_category_x,eval_category_y\n"
        rows = list(csv.reader(f))
    assert len(rows) == 9
    for k, row in enumerate(rows):                       # x outer, y inner
        i, j = divmod(k, 3)
        assert row[2:] == [words[i], words[j]]
        assert float(row[0]) == float(res["image_sims"][i, j]) and float(row[1]) == float(res["text_sims"][i, j])
        assert row[0] == repr(float(res["image_sims"][i, j]))            # pandas' shortest round-trip repr
    with open(tmp_path / "cvc_image_text_embeddings_sims_seed_0.csv") as f:
        assert f.readline() == "image_text_sims,eval_category_x,eval_category_y\n"
        rows = list(csv.reader(f))
    assert [r[1:] for r in rows] == [[words[i], words[j]] for i in range(3) for j in range(3)]
    assert float(rows[5][0]) == float(res["image_text_sims"][1, 2])
    assert not (tmp_path / "cvc_joint_embeddings_tsne_seed_0.csv").exists()
    on_disk = json.load(open(tmp_path / "alignment.json"))
    assert on_disk == summary and on_disk["r"] == 0.25 and on_disk["p"] == 0.5 and on_disk["n_pairs"] == 3
    assert on_disk["paired_distances"] == {"ball": 1.5, "car": 2.5, "kitty": 3.5}
    assert abs(on_disk["distance_accuracy"]["r"] - np.corrcoef([1.5, 2.5, 3.5], [90.0, 50.0, 20.0])[0, 1]) < 1e-12
    with pytest.raises(KeyError, match="kitty"):
        A.write_results(str(tmp_path), "cvc", 0, words, feats, text, res, dist, accuracies={"ball": 1.0, "car": 2.0})


def test_tsne_file_when_sklearn_is_present(tmp_path):
    pytest.importorskip("sklearn")
    from multimodal import alignment as A
    n = 12
    feats, _labels, text = AC.prototype_case(5, n, 16)
    res = _fake_result(n)
    res["combined_sims"] = AC.cosine64(AC.interleave(text, text[::-1].copy())).astype(np.float32)
    words = [f"w{i}" for i in range(n)]
    A.write_results(str(tmp_path), "cvc", 1, words, feats, text, res, np.zeros(n), tsne=True)
    with open(tmp_path / "cvc_joint_embeddings_tsne_seed_1.csv") as f:
        assert f.readline() == "x,y,eval_category,modality\n"
        rows = list(csv.reader(f))
    assert len(rows) == 2 * n
    assert [r[2] for r in rows] == [w for w in words for _ in range(2)] and [r[3] for r in rows] == ["image", "text"] * n
    assert all(np.isfinite(float(r[0])) and np.isfinite(float(r[1])) for r in rows)


def test_kitty_mapping():
    from multimodal import alignment as A
    cats = ["ball", "car", "cat", "dog"]
    assert A.category_words(cats) == cats
    assert A.category_words(cats, use_kitty_label=True) == ["ball", "car", "kitty", "dog"]
    from multimodal.multimodal_data_module import read_vocab
    vocab = read_vocab()
    assert all(w in vocab for w in A.SYNTHETIC_WORDS) and "kitty" in vocab
    assert list(A.SYNTHETIC_WORDS) == sorted(A.SYNTHETIC_WORDS)


def test_seeded_sampling():
    from multimodal import alignment as A
    labels = ["b"] * 5 + ["a"] * 300 + ["c"] * 40
    idx, picked = A.sample_indices(labels, per_class=200, replace=True, seed=0)
    idx2, picked2 = A.sample_indices(labels, per_class=200, replace=True, seed=0)
    assert np.array_equal(idx, idx2) and picked == picked2                           # reproducible
    assert picked == ["a"] * 200 + ["b"] * 5 + ["c"] * 40                            # sorted categories, min(len, per_class) each
    assert all(labels[i] == p for i, p in zip(idx, picked))
    assert len(set(idx[:200].tolist())) < 200                                        # with replacement (alignment.py:86)
    # the stream is the one np.random.seed(0) + np.random.choice give, category after category
    st = np.random.get_state()
    np.random.seed(0)
    want = [np.random.choice(np.arange(5, 305), size=200), np.random.choice(np.arange(0, 5), size=5),
            np.random.choice(np.arange(305, 345), size=40)]
    np.random.set_state(st)
    assert np.array_equal(idx, np.concatenate(want))
    idx3, _ = A.sample_indices(labels, per_class=100, replace=False, seed=0)          # embeddings.py:72
    assert len(set(idx3[:100].tolist())) == 100 and sorted(idx3[100:105].tolist()) == [0, 1, 2, 3, 4]


def test_p_value_agrees_with_scipy():
    from multimodal import alignment as A
    try:
        import scipy.stats
    except ImportError:
        assert A.pearson_p_value(0.3, 21) is None
        return
    rng = np.random.default_rng(0)
    for n in (3, 21, 231, 2000):
        x = rng.standard_normal(n)
        y = 0.4 * x + rng.standard_normal(n)
        res = scipy.stats.pearsonr(x, y)
        p = A.pearson_p_value(res[0], n)
        assert abs(p - res[1]) <= 1e-9 * max(res[1], 1e-300) + 1e-300, (n, p, res[1])
    assert np.isnan(A.pearson_p_value(float("nan"), 21))
    g = _g()
    assert abs(A.pearson_p_value(g["pearson"][0], int(g["pearson"][2])) - g["pearson"][1]) <= 1e-9 * g["pearson"][1]
