"""The alignment kernels on the MI355X (csrc/alignment.hip, multimodal/alignment.py) against the float64 restatement of
tests/alignment_common.py.  Bounds (u = 2^-24):
  class means       |mean - mean64| <= 16 u mean_i |x_i| per element (a fixed tree over <= 2^16 members has depth 16; the kernel sums in double)
  cosine entries    |out - out64| <= 2 D u (worst-case fp32 dot product of unit vectors plus the two normalisations)
  paired distances  16 u relative
  Pearson           |r - r64| <= 4 delta / sigma_min, delta = 2 D u, sigma_min = the smaller standard deviation of the two triangles in
                    float64, computed from the data; the inputs (class prototypes plus noise) must give sigma_min >= 0.05, which every
                    case asserts, and the reference's own fp32 arithmetic (normalise, then cosine, entry by entry) is checked on the
                    CPU against the same bound on the same inputs.
Every case prints its figures before it asserts."""
import csv
import json
import os
import subprocess
import sys

import numpy as np
import pytest
import torch

import alignment_common as AC
from conftest import ROOT, load_golden

pytestmark = pytest.mark.gpu

DEV = "cuda:0"
U = AC.U

# (C, D, sizes or None = 1 .. 37 at random with a singleton): D in {37, 64, 512, 2048}, C in {3, 7, 22, 257}, no N a multiple of a tile
CASES = [
    (3, 37, [1, 4099, 333]),
    (7, 64, [1, 3001, 2, 65, 130, 511, 17]),
    (22, 512, [1] + [150 + 3 * i for i in range(21)]),
    (257, 2048, None),
    (257, 37, None),
    (3, 2048, [5, 1, 1031]),
    (22, 64, None),
    (7, 512, [63, 64, 65, 1, 255, 257, 129]),
]
IDS = [f"C{c}-D{d}" for c, d, _ in CASES]


def _A():
    from multimodal import alignment
    return alignment


def _case(i):
    Cn, D, sizes = CASES[i]
    return AC.prototype_case(100 + i, Cn, D, sizes)


def _dev(a):
    return torch.from_numpy(np.ascontiguousarray(a)).to(DEV)


def _fp32_reference_cosines(a):
    """F.cosine_similarity(F.normalize(a_i), F.normalize(a_j)) in fp32 on the CPU, all entries at once (alignment.py:182-195)"""
    n = torch.nn.functional.normalize(torch.from_numpy(a), p=2, dim=1)
    nn_ = n.norm(dim=1).clamp_min(1e-8)
    return ((n @ n.T) / (nn_[:, None] * nn_[None, :])).numpy()


@pytest.mark.parametrize("i", range(len(CASES)), ids=IDS)
def test_class_means(i):
    A = _A()
    feats, labels, _ = _case(i)
    Cn = CASES[i][0]
    means, counts = A.class_means(_dev(feats), labels, Cn)
    want = AC.class_means64(feats, labels, Cn)
    bound = AC.mean_bound(feats, labels, Cn)
    err = np.abs(means.cpu().numpy().astype(np.float64) - want)
    print(f"[class_means {IDS[i]}] N {len(labels)} sizes {np.bincount(labels).min()}..{np.bincount(labels).max()}: "
          f"worst error / bound {float((err / bound).max()):.3f}")
    assert np.array_equal(counts.cpu().numpy(), np.bincount(labels, minlength=Cn))
    assert bool((err <= bound).all())
    # labels as a device tensor, and as int64: the same bits
    m2, _ = A.class_means(_dev(feats), torch.from_numpy(labels.astype(np.int64)).to(DEV), Cn)
    assert torch.equal(m2, means)


def test_class_means_empty_class_and_bad_labels():
    A = _A()
    feats, labels, _ = _case(1)
    x = _dev(feats)
    with pytest.raises(ValueError, match=r"without a member: \[7, 8\]"):
        A.class_means(x, labels, 9)
    means, counts = A._class_means(x, labels, 9)
    assert counts.cpu().tolist()[7:] == [0, 0] and float(means[7:].abs().max()) == 0.0
    with pytest.raises(ValueError, match="outside"):
        A.class_means(x, labels, 6)
    with pytest.raises(ValueError, match="outside"):
        A.class_means(x, torch.from_numpy(labels).to(DEV) - 1, 7)


@pytest.mark.parametrize("i", range(len(CASES)), ids=IDS)
def test_cosine_matrices(i):
    A = _A()
    feats, labels, text = _case(i)
    Cn, D, _ = CASES[i]
    bound = AC.cosine_bound(D)
    t = _dev(text)
    b = _dev(feats[:301])
    got_self = A.cosine_matrix(t).cpu().numpy()
    got_pair = A.cosine_matrix(t, b).cpu().numpy()
    got_pair_t = A.cosine_matrix(b, t).cpu().numpy()
    e_self = float(np.abs(got_self - AC.cosine64(text)).max())
    e_pair = float(np.abs(got_pair - AC.cosine64(text, feats[:301])).max())
    e_diag = float(np.abs(np.diag(got_self).astype(np.float64) - 1.0).max())
    print(f"[cosine {IDS[i]}] bound {bound:.3e}: self {e_self:.3e}, [C, 301] {e_pair:.3e}, diagonal - 1 {e_diag:.3e}")
    assert got_self.shape == (Cn, Cn) and got_pair.shape == (Cn, min(301, len(labels)))
    assert e_self <= bound and e_pair <= bound and e_diag <= bound
    assert np.array_equal(got_self, got_self.T)                          # bit-symmetric
    assert float(np.abs(got_pair_t.T.astype(np.float64) - AC.cosine64(text, feats[:301])).max()) <= bound
    # a copy of the operand is a second pointer: the general path, the same values within the bound and the same diagonal claim
    got_copy = A.cosine_matrix(t, t.clone()).cpu().numpy()
    assert float(np.abs(got_copy - AC.cosine64(text)).max()) <= bound


@pytest.mark.parametrize("M,K,D", [(700, 900, 512), (1000, 1000, 2048), (333, 1025, 37)])
def test_cosine_matrix_32_tiles_and_zero_rows(M, K, D):
    A = _A()
    rng = np.random.default_rng(M + K + D)
    a = rng.standard_normal((M, D)).astype(np.float32)
    b = rng.standard_normal((K, D)).astype(np.float32)
    a[5] = 0.0
    b[K - 1] = 0.0
    bound = AC.cosine_bound(D)
    got = A.cosine_matrix(_dev(a), _dev(b)).cpu().numpy()
    err = float(np.abs(got - AC.cosine64(a, b)).max())
    print(f"[cosine {M}x{K} D {D}] bound {bound:.3e}: error {err:.3e}")
    assert err <= bound
    assert not got[5].any() and not got[:, K - 1].any()                  # zero rows give 0
    s = A.cosine_matrix(_dev(a)).cpu().numpy()
    assert np.array_equal(s, s.T) and float(np.abs(s - AC.cosine64(a)).max()) <= bound
    d = np.diag(s).astype(np.float64)
    assert d[5] == 0.0 and float(np.abs(np.delete(d, 5) - 1.0).max()) <= bound


@pytest.mark.parametrize("i", range(len(CASES)), ids=IDS)
def test_paired_distances(i):
    A = _A()
    feats, labels, text = _case(i)
    Cn = CASES[i][0]
    means = AC.class_means64(feats, labels, Cn).astype(np.float32)
    got = A.paired_distances(_dev(means), _dev(text)).cpu().numpy().astype(np.float64)
    want = AC.paired_l2_64(means, text)
    rel = float((np.abs(got - want) / want).max())
    print(f"[paired_distances {IDS[i]}] worst relative error {rel:.3e} (bound {16 * U:.3e})")
    assert rel <= 16 * U
    same = A.paired_distances(_dev(text), _dev(text)).cpu().numpy().astype(np.float64)      # x == y: the eps term alone
    assert float(np.abs(same / (1e-6 * np.sqrt(text.shape[1])) - 1.0).max()) <= 1e-6


@pytest.mark.parametrize("i", range(len(CASES)), ids=IDS)
def test_pearson_chain(i):
    A = _A()
    feats, labels, text = _case(i)
    Cn, D, _ = CASES[i]
    m64 = AC.class_means64(feats, labels, Cn)
    c_img, c_txt = AC.cosine64(m64), AC.cosine64(text)
    tri_i, tri_t = AC.triu_items(c_img), AC.triu_items(c_txt)
    r64 = AC.pearson64(tri_i, tri_t)[0]
    bound, sigma = AC.pearson_bound(D, tri_i, tri_t)
    # the reference's own fp32 arithmetic on these inputs (CPU)
    ref_i = _fp32_reference_cosines(m64.astype(np.float32))
    ref_t = _fp32_reference_cosines(text)
    r_ref = AC.pearson64(AC.triu_items(ref_i), AC.triu_items(ref_t))[0]
    means, _ = A.class_means(_dev(feats), labels, Cn)
    s_img, s_txt = A.cosine_matrix(means), A.cosine_matrix(_dev(text))
    r, p = A.rsa_of_dissim_matrices(s_img, s_txt)
    r_dis, _ = A.rsa_of_dissim_matrices(A.cosine_dissim_matrix(means), A.cosine_dissim_matrix(_dev(text)))
    r64_dis = AC.rsa64(AC.dissim64(m64), AC.dissim64(text))
    print(f"[pearson {IDS[i]}] n {len(tri_i)} sigma_min {sigma:.4f} bound {bound:.3e}: r64 {r64:.9f}, kernel chain error {abs(r - r64):.3e}, "
          f"dissimilarity chain error {abs(r_dis - r64_dis):.3e}, reference fp32 error {abs(r_ref - r64):.3e}")
    assert sigma >= 0.05
    assert abs(r_ref - r64) <= bound
    assert abs(r - r64) <= bound
    assert abs(r_dis - r64_dis) <= bound
    # the kernel alone, on the fp32 matrices it was given: moments in double
    m = A.triu_moments(s_img, s_txt)
    a_tri, b_tri = AC.triu_items(s_img.cpu().numpy()), AC.triu_items(s_txt.cpu().numpy())
    w = AC.pearson64(a_tri, b_tri)
    assert m["n"] == Cn * (Cn - 1) // 2 == w[1]
    assert abs(m["r"] - w[0]) <= 1e-12 and m["r"] == r
    assert abs(m["mean_a"] - w[2]) <= 1e-14 and abs(m["mean_b"] - w[3]) <= 1e-14
    assert abs(m["var_a"] - w[4]) <= 1e-13 * max(1.0, w[4]) and abs(m["var_b"] - w[5]) <= 1e-13 * max(1.0, w[5])
    try:
        import scipy.stats
        ps = scipy.stats.pearsonr(a_tri.astype(np.float64), b_tri.astype(np.float64))[1]
        assert abs(p - ps) <= 1e-6 * ps + 1e-300
    except ImportError:
        assert p is None
    assert torch.equal(A.strict_upper_tri_items(s_img).cpu(), torch.from_numpy(a_tri))


def test_pearson_large_and_zero_variance():
    A = _A()
    rng = np.random.default_rng(9)
    Cn = 2350
    a = rng.standard_normal((Cn, Cn)).astype(np.float32)
    b = (0.3 * a + rng.standard_normal((Cn, Cn))).astype(np.float32)
    m = A.triu_moments(_dev(a), _dev(b))
    w = AC.pearson64(AC.triu_items(a), AC.triu_items(b))
    print(f"[pearson C {Cn}] r {m['r']:.12f} against {w[0]:.12f}")
    assert m["n"] == w[1] and abs(m["r"] - w[0]) <= 1e-12 and abs(m["var_a"] - w[4]) <= 1e-12 and abs(m["mean_b"] - w[3]) <= 1e-14
    const = np.full((22, 22), 0.1, dtype=np.float32)                  # 0.1 is not exact in binary: a naive sum / n would not see it
    lower = np.tril(rng.standard_normal((22, 22))).astype(np.float32)
    for A_, B_ in ((const, a[:22, :22].copy()), (a[:22, :22].copy(), const), (const + lower, a[:22, :22].copy())):
        r, p = A.rsa_of_dissim_matrices(_dev(A_), _dev(B_))               # only the strict upper triangle counts
        assert np.isnan(r) and (p is None or np.isnan(p))
    r, _ = A.rsa_of_dissim_matrices(_dev(a[:3, :3].copy()), _dev((2 * a[:3, :3] + 1).copy()))
    assert abs(r - 1.0) <= 1e-12                                          # C = 3, the smallest


def test_every_kernel_is_deterministic_and_class_means_ignore_addresses():
    A = _A()
    feats, labels, text = _case(3)
    Cn = CASES[3][0]
    x, t = _dev(feats), _dev(text)
    m1, c1 = A.class_means(x, labels, Cn)
    s1, q1 = A.cosine_matrix(m1), A.cosine_matrix(m1, t)
    p1 = A._triu_pearson(s1, A.cosine_matrix(t)).clone()
    d1 = A.paired_distances(m1, t)
    m2, c2 = A.class_means(x, labels, Cn)
    assert torch.equal(m1, m2) and torch.equal(c1, c2)
    assert torch.equal(s1, A.cosine_matrix(m1)) and torch.equal(q1, A.cosine_matrix(m1, t))
    assert torch.equal(p1, A._triu_pearson(s1, A.cosine_matrix(t)))
    assert torch.equal(d1, A.paired_distances(m1, t))
    # free and reallocate everything else, move the operand: the same bits
    keep = m1.cpu()
    del m1, m2, s1, q1, p1, d1, c1, c2, t
    junk = [torch.empty(n, device=DEV) for n in (1 << 20, 12345, 1 << 22)]
    x2 = x.clone()
    del x, junk
    torch.cuda.empty_cache()
    pad = torch.empty(777, device=DEV)
    x3 = x2.clone()
    assert x3.data_ptr() != x2.data_ptr()
    m3, _ = A.class_means(x3, labels, Cn)
    m4, _ = A.class_means(x2, labels, Cn)
    assert torch.equal(m3.cpu(), keep) and torch.equal(m4.cpu(), keep)
    del pad


def test_alignment_on_the_golden_fixture():
    A = _A()
    g = {k: (v.numpy() if torch.is_tensor(v) else v) for k, v in load_golden("alignment").items()}
    feats, labels, text = g["features"], g["labels"], g["text_features"]
    res = A.alignment(_dev(feats), labels, _dev(text))
    D = feats.shape[1]
    cb = AC.cosine_bound(D)
    assert bool((np.abs(res["mean_image_features"].astype(np.float64) - g["mean_image_features"]) <= AC.mean_bound(feats, labels, 7)).all())
    for k in ("image_sims", "text_sims", "image_text_sims", "combined_sims"):
        err = float(np.abs(res[k].astype(np.float64) - g[k]).max())
        print(f"[golden {k}] error {err:.3e} (bound {cb:.3e})")
        assert res[k].shape == g[k].shape and err <= cb
    # image_0, text_0, image_1, ...: the blocks of combined_sims are the three small matrices
    assert np.array_equal(res["combined_sims"][0::2, 0::2], res["image_sims"])
    assert np.array_equal(res["combined_sims"][1::2, 1::2], res["text_sims"])
    assert float(np.abs(res["combined_sims"][0::2, 1::2] - res["image_text_sims"]).max()) <= cb
    assert float(np.abs(A.cosine_matrix(_dev(res["mean_image_features"])).cpu().numpy() - g["rs_cosine_matrix"]).max()) <= cb
    assert float(np.abs(A.cosine_dissim_matrix(_dev(res["mean_image_features"])).cpu().numpy() - g["rs_cosine_dissim_matrix"]).max()) <= cb
    m64 = AC.class_means64(feats, labels, 7)
    bound, sigma = AC.pearson_bound(D, AC.triu_items(AC.cosine64(m64)), AC.triu_items(AC.cosine64(text)))
    r_ref, p_ref, n_ref = g["pearson"]
    print(f"[golden pearson] r {res['pearson_r']:.9f} against the reference's {r_ref:.9f} (bound {bound:.3e}, sigma_min {sigma:.4f})")
    assert sigma >= 0.05 and res["n_pairs"] == n_ref == 21 and abs(res["pearson_r"] - r_ref) <= bound
    assert res["pearson_p"] == A.pearson_p_value(res["pearson_r"], 21)
    d = A.paired_distances(_dev(res["mean_image_features"]), _dev(text)).cpu().numpy().astype(np.float64)
    assert float((np.abs(d - g["paired_distances"]) / g["paired_distances"]).max()) <= 16 * U + 2 * U   # (+ the stored fp32 value's own rounding)


def test_script_end_to_end(tmp_path):
    A = _A()
    out = tmp_path / "alignment"
    cmd = [sys.executable, os.path.join(ROOT, "alignment.py"), "--dataset", "synthetic", "--random_init", "--out", str(out)]
    try:
        import sklearn  # noqa: F401
        cmd.append("--tsne")
        tsne = True
    except ImportError:
        tsne = False
    r = subprocess.run(cmd, cwd=tmp_path, capture_output=True, text=True, timeout=600)
    assert r.returncode == 0, r.stdout[-3000:] + r.stderr[-3000:]
    words = list(A.SYNTHETIC_WORDS)
    Cn = len(words)
    feats = np.load(out / "cvc_all_image_features_seed_0.npy")
    means = np.load(out / "cvc_mean_image_features_seed_0.npy")
    text = np.load(out / "cvc_all_text_features_seed_0.npy")
    assert feats.shape == (Cn * 12, 512) and means.shape == (Cn, 512) and text.shape == (Cn, 512) and feats.dtype == np.float32
    labels = np.repeat(np.arange(Cn), 12)
    m64 = AC.class_means64(feats, labels, Cn)
    assert bool((np.abs(means - m64) <= AC.mean_bound(feats, labels, Cn)).all())
    with open(out / "cvc_joint_embeddings_sims_seed_0.csv") as f:
        assert f.readline() == "image_sims,text_sims,eval_category_x,eval_category_y\n"
        rows = list(csv.reader(f))
    assert [row[2:] for row in rows] == [[words[i], words[j]] for i in range(Cn) for j in range(Cn)]
    img = np.array([float(row[0]) for row in rows]).reshape(Cn, Cn)
    txt = np.array([float(row[1]) for row in rows]).reshape(Cn, Cn)
    cb = AC.cosine_bound(512)
    assert float(np.abs(img - AC.cosine64(m64)).max()) <= cb and float(np.abs(txt - AC.cosine64(text)).max()) <= cb
    with open(out / "cvc_image_text_embeddings_sims_seed_0.csv") as f:
        assert f.readline() == "image_text_sims,eval_category_x,eval_category_y\n"
        rows = list(csv.reader(f))
    assert len(rows) == Cn * Cn
    assert float(np.abs(np.array([float(row[0]) for row in rows]).reshape(Cn, Cn) - AC.cosine64(m64, text)).max()) <= cb
    summary = json.load(open(out / "alignment.json"))
    tri_i, tri_t = AC.triu_items(AC.cosine64(m64)), AC.triu_items(AC.cosine64(text))
    r64 = AC.pearson64(tri_i, tri_t)[0]
    bound, sigma = AC.pearson_bound(512, tri_i, tri_t)
    print(f"[script] r {summary['r']:.9f} against {r64:.9f} (bound {bound:.3e}, sigma_min {sigma:.3e})")
    assert summary["n_pairs"] == Cn * (Cn - 1) // 2 and abs(summary["r"] - r64) <= bound
    assert list(summary["paired_distances"]) == words
    want_d = AC.paired_l2_64(means, text)
    assert all(abs(summary["paired_distances"][w] - want_d[k]) <= 18 * U * want_d[k] for k, w in enumerate(words))
    assert f"PearsonRResult(statistic={summary['r']}" in r.stdout
    tsne_file = out / "cvc_joint_embeddings_tsne_seed_0.csv"
    assert tsne_file.exists() == tsne
    if tsne:
        with open(tsne_file) as f:
            assert f.readline() == "x,y,eval_category,modality\n"
            assert len(list(csv.reader(f))) == 2 * Cn
