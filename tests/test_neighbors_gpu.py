"""The nearest-neighbour searches on the MI355X (csrc/neighbors.hip, multimodal/neighbors.py).

Cosine: the reference value is float64 F.cosine_similarity + max on the CPU, evaluated as a product of rows normalised in float64
(the same function without the Nb x Nq x D intermediate), in row blocks.  Over ALL queries the returned index j must satisfy
cos64[i, j] >= max_j cos64[i, .] - tau and |best_cos - max64| <= tau, with tau = 4 x the worst error of torch's own fp32
cosine similarity against float64 on the same inputs (evaluated the same way in fp32 on the CPU): a tiled MFMA sum and torch's
sum order differ and both are legitimate fp32 evaluations.  Every case prints its tau and the kernel's own error before asserting.
Measured on one MI355X (Gaussian rows, Nq = 2200, Nb = 50 000, D = 2048): see DESIGN.md section 9 "Nearest-neighbour searches".

Pixels: the reference value is integer numpy -- exact channel sums, the same double expression bit for bit, numpy's first arg-min.
One case restates the reference's fp32 lines (duplicates.py:993-1002) on the CPU and checks that the reference picks the same frame
wherever the exact top-2 margin exceeds the reference's own rounding error; the inputs (planted neighbours on a random
background) leave no case out, which the test asserts (0 of 24 left out)."""
import csv
import json
import os
import subprocess
import sys

import numpy as np
import pytest
import torch

from conftest import ROOT

pytestmark = pytest.mark.gpu

DEV = "cuda:0"


def _N():
    from multimodal import neighbors
    return neighbors


# ---- cosine -----------------------------------------------------------------------------------------------------------------------
def _check_cosine(name, q, b, got_cos, got_idx, eligible=None, block=256):
    """both checks over all queries; returns (tau, kernel error)"""
    qn64 = q.double() / q.double().norm(dim=1, keepdim=True).clamp_min(1e-8)
    bn64 = b.double() / b.double().norm(dim=1, keepdim=True).clamp_min(1e-8)
    qn32 = q / q.norm(dim=1, keepdim=True).clamp_min(1e-8)
    bn32 = b / b.norm(dim=1, keepdim=True).clamp_min(1e-8)
    torch_err, max64, at_got = 0.0, [], []
    for s in range(0, q.shape[0], block):
        c64 = qn64[s:s + block] @ bn64.T
        c32 = qn32[s:s + block] @ bn32.T
        torch_err = max(torch_err, float((c32.double() - c64).abs().max()))
        if eligible is not None:
            c64 = c64.masked_fill(~eligible[s:s + block], float("-inf"))
        max64.append(c64.max(dim=1).values)
        gi = got_idx[s:s + block].clamp_min(0)
        at_got.append(c64.gather(1, gi[:, None])[:, 0])
    max64, at_got = torch.cat(max64), torch.cat(at_got)
    tau = 4.0 * torch_err
    has = torch.isfinite(max64)
    assert bool((got_idx[~has] == -1).all()) and bool((got_cos[~has] == float("-inf")).all())
    assert bool((got_idx[has] >= 0).all())
    idx_gap = float((max64[has] - at_got[has]).max()) if bool(has.any()) else 0.0
    val_err = float((got_cos[has].double() - max64[has]).abs().max()) if bool(has.any()) else 0.0
    print(f"[cosine {name}] Nq {q.shape[0]} Nb {b.shape[0]} D {q.shape[1]}: torch fp32 worst error {torch_err:.3e} -> tau {tau:.3e}; "
          f"kernel |best_cos - max64| {val_err:.3e}; cos64 gap of the returned index {idx_gap:.3e}")
    assert idx_gap <= tau, (name, idx_gap, tau)
    assert val_err <= tau, (name, val_err, tau)
    return tau, val_err


def _search(q, b, **kw):
    cos, idx = _N().nearest_cosine(q.to(DEV), b.to(DEV), **kw)
    torch.cuda.synchronize()
    return cos.cpu(), idx.cpu()


def test_cosine_gaussian_full_size():
    g = torch.Generator().manual_seed(0)
    q, b = torch.randn(2200, 2048, generator=g), torch.randn(50000, 2048, generator=g)
    cos, idx = _search(q, b)
    _check_cosine("gaussian", q, b, cos, idx)
    # a chunked search equals the one-shot search bit for bit
    cos_c, idx_c = _search(q, b, chunk=12345)
    assert torch.equal(cos_c, cos) and torch.equal(idx_c, idx)


def test_cosine_nonnegative_rows_with_planted_copies():
    g = torch.Generator().manual_seed(1)
    q = torch.randn(600, 2048, generator=g).relu_()          # as a ReLU-pooled feature is
    b = torch.randn(5003, 2048, generator=g).relu_()
    for k in range(100):                                     # exact copies, and copies perturbed by 1e-3
        b[37 * k + 5] = q[k]
        b[37 * k + 9] = q[100 + k] * (1.0 + 1e-3 * torch.randn(2048, generator=g))
    cos, idx = _search(q, b)
    _check_cosine("relu+planted", q, b, cos, idx)
    assert idx[:100].tolist() == [37 * k + 5 for k in range(100)]
    assert idx[100:200].tolist() == [37 * k + 9 for k in range(100)]


def test_cosine_strides_ragged_sizes_and_zero_rows():
    g = torch.Generator().manual_seed(2)
    N = _N()
    qs, bs = torch.randn(130, 520, generator=g).to(DEV), torch.randn(777, 640, generator=g).to(DEV)      # D = 512, strides above D
    q, b = qs[:, :512], bs[:, 64:576]
    assert q.stride(0) == 520 and b.stride(0) == 640
    cos, idx = N.nearest_cosine(q, b)
    cos_p, idx_p = N.nearest_cosine(q.contiguous(), b.contiguous())
    assert torch.equal(cos, cos_p) and torch.equal(idx, idx_p)
    _check_cosine("D512 strided", q.cpu().contiguous(), b.cpu().contiguous(), cos.cpu(), idx.cpu())
    for Nq, Nb, D in ((1, 1, 7), (3, 2, 33), (129, 127, 130), (257, 129, 2048), (64, 1000, 100)):          # no multiple of any tile
        q, b = torch.randn(Nq, D, generator=g), torch.randn(Nb, D, generator=g)
        cos, idx = _search(q, b)
        _check_cosine(f"ragged {Nq}x{Nb}x{D}", q, b, cos, idx)
    q, b = torch.randn(5, 64, generator=g), torch.randn(9, 64, generator=g)
    q[2] = 0
    b[4] = 0
    cos, idx = _search(q, b)
    assert float(cos[2]) == 0.0 and int(idx[2]) == 0         # a zero query: every cosine is 0, the tie goes to row 0
    cos0, _ = _search(q, b[4:5])
    assert bool((cos0 == 0).all())                           # a zero base row gives cosine 0


def test_cosine_groups_ties_and_chunks():
    g = torch.Generator().manual_seed(3)
    N = _N()
    D, G = 256, 22
    sizes_b = [0 if c == 7 else 40 + 13 * c for c in range(G)]                 # unequal, group 7 empty on the base side
    sizes_q = [3 + (c % 5) for c in range(G)]
    bg = torch.cat([torch.full((n,), c, dtype=torch.int32) for c, n in enumerate(sizes_b)])
    qg = torch.cat([torch.full((n,), c, dtype=torch.int32) for c, n in enumerate(sizes_q)])
    bg, qg = bg[torch.randperm(len(bg), generator=g)], qg[torch.randperm(len(qg), generator=g)]
    q, b = torch.randn(len(qg), D, generator=g), torch.randn(len(bg), D, generator=g)
    cos, idx = _search(q, b, query_groups=qg, base_groups=bg)
    _check_cosine("22 groups", q, b, cos, idx, eligible=qg[:, None] == bg[None, :])
    assert bool((idx[qg == 7] == -1).all()) and bool((cos[qg == 7] == float("-inf")).all())
    for c in range(G):                                       # equals the ungrouped kernel run per group
        qi, bi = (qg == c).nonzero()[:, 0], (bg == c).nonzero()[:, 0]
        if len(bi) == 0:
            continue
        cc, ii = _search(q[qi], b[bi])
        assert torch.equal(cc, cos[qi]) and torch.equal(bi[ii], idx[qi]), c
    cos_c, idx_c = _search(q, b, query_groups=qg, base_groups=bg, chunk=101)
    assert torch.equal(cos_c, cos) and torch.equal(idx_c, idx)
    # exact ties from duplicated base rows: the lower index, in one shot and across chunk and tile boundaries
    b2 = torch.randn(900, D, generator=g)
    for k, (lo, hi) in enumerate(((3, 4), (100, 700), (127, 128), (5, 899))):
        b2[lo] = q[k]
        b2[hi] = q[k]
    cos_t, idx_t = _search(q[:4], b2)
    assert idx_t.tolist() == [3, 100, 127, 5]
    for chunk in (1, 128, 500):
        cc, ii = _search(q[:4], b2, chunk=chunk)
        assert torch.equal(cc, cos_t) and torch.equal(ii, idx_t), chunk
    with pytest.raises(Exception):
        N.nearest_cosine(q.to(DEV), b.to(DEV), query_groups=qg)


# ---- pixels -----------------------------------------------------------------------------------------------------------------------
def _pixel_reference(q, b, std, eligible=None):
    """integer numpy: (dist [Nq] float64, first arg-min [Nq], the winner's channel sums [Nq, C] int64)"""
    Nq, Cn = q.shape[0], q.shape[1]
    qi = q.reshape(Nq, Cn, -1).astype(np.int16)
    bi = b.reshape(b.shape[0], Cn, -1).astype(np.int16)
    w = [1.0 / (255.0 * float(s)) for s in std]
    S = np.stack([np.abs(qi[i][None] - bi).sum(axis=2, dtype=np.int64) for i in range(Nq)])       # [Nq, Nb, C]
    d = S[..., 0].astype(np.float64) * w[0]
    for c in range(1, Cn):
        d = d + S[..., c].astype(np.float64) * w[c]
    if eligible is not None:
        d = np.where(eligible, d, np.inf)
    idx = d.argmin(axis=1)
    none = ~np.isfinite(d.min(axis=1))
    sums = S[np.arange(Nq), idx]
    sums[none] = 0
    return d.min(axis=1), np.where(none, -1, idx), sums


def _check_pixels(name, q, b, std=(0.229, 0.224, 0.225), groups=None, **kw):
    N = _N()
    eligible = None if groups is None else groups[0][:, None] == groups[1][None, :]
    want_d, want_i, want_s = _pixel_reference(q, b, std, eligible)
    gk = {} if groups is None else dict(query_groups=torch.from_numpy(groups[0]), base_groups=torch.from_numpy(groups[1]))
    dist, idx, sums = N.nearest_pixels(torch.from_numpy(q).to(DEV), torch.from_numpy(b).to(DEV), std=std, **gk, **kw)
    torch.cuda.synchronize()
    dist, idx, sums = dist.cpu().numpy(), idx.cpu().numpy(), sums.cpu().numpy()
    print(f"[pixels {name}] {q.shape} x {b.shape}: sums equal {np.array_equal(sums, want_s)}, dist bits equal "
          f"{np.array_equal(dist.view(np.int64), want_d.view(np.int64))}, idx equal {np.array_equal(idx, want_i)}")
    assert np.array_equal(sums, want_s), name
    assert np.array_equal(dist.view(np.int64), want_d.view(np.int64)), name
    assert np.array_equal(idx, want_i), name
    return dist, idx, sums


def test_pixels_224_frames():
    rng = np.random.default_rng(0)
    q = rng.integers(0, 256, (32, 3, 224, 224), dtype=np.uint8)
    b = rng.integers(0, 256, (512, 3, 224, 224), dtype=np.uint8)
    for k in range(8):                                       # near-duplicates: +-1 on a few pixels
        b[50 * k + 7] = q[k]
        for _ in range(5):
            c, y, x = rng.integers(3), rng.integers(224), rng.integers(224)
            v = int(b[50 * k + 7, c, y, x])
            b[50 * k + 7, c, y, x] = v + 1 if v < 128 else v - 1
    dist, idx, sums = _check_pixels("32x512 at 3x224x224", q, b)
    assert idx[:8].tolist() == [50 * k + 7 for k in range(8)] and int(sums[:8].sum(axis=1).max()) <= 5
    d2, i2, s2 = _check_pixels("chunked", q, b, chunk=100)
    assert np.array_equal(d2, dist) and np.array_equal(i2, idx) and np.array_equal(s2, sums)


def test_pixels_many_small_frames_with_duplicates_and_ties():
    rng = np.random.default_rng(1)
    q = rng.integers(0, 256, (16, 3, 64, 64), dtype=np.uint8)
    b = rng.integers(0, 256, (20000, 3, 64, 64), dtype=np.uint8)
    for k in range(8):                                       # exact duplicates, each planted twice: distance 0, the lower index
        b[1000 + 2000 * k] = q[k]
        b[19999 - 7 * k] = q[k]
    dist, idx, _ = _check_pixels("16x20000 at 3x64x64", q, b)
    assert idx[:8].tolist() == [1000 + 2000 * k for k in range(8)] and bool((dist[:8] == 0).all())
    _check_pixels("16x20000 chunked", q, b, chunk=3001)


def test_pixels_extremes_ragged_tails_one_channel_and_groups():
    rng = np.random.default_rng(2)
    N = _N()
    q = np.zeros((3, 3, 224, 224), dtype=np.uint8)
    b = np.full((5, 3, 224, 224), 255, dtype=np.uint8)        # all-0 against all-255: the largest sums
    b[3, :, 0, 0] = 254
    _, idx, sums = _check_pixels("0 vs 255", q, b)
    assert idx.tolist() == [3, 3, 3] and sums[0].tolist() == [224 * 224 * 255 - 1] * 3
    for hw in ((1, 4), (3, 4), (5, 52), (31, 36), (17, 100), (40, 68)):           # HW % 4 == 0, ragged lane and vector tails
        q = rng.integers(0, 256, (9, 3) + hw, dtype=np.uint8)
        b = rng.integers(0, 256, (41, 3) + hw, dtype=np.uint8)
        _check_pixels(f"HW {hw}", q, b)
    q = rng.integers(0, 256, (10, 1, 32, 32), dtype=np.uint8)
    b = rng.integers(0, 256, (70, 1, 32, 32), dtype=np.uint8)
    _check_pixels("C = 1", q, b, std=(0.5,))
    q = rng.integers(0, 256, (30, 3, 16, 16), dtype=np.uint8)
    b = rng.integers(0, 256, (300, 3, 16, 16), dtype=np.uint8)
    qg = rng.integers(0, 6, 30).astype(np.int32)
    bg = rng.integers(0, 5, 300).astype(np.int32)             # group 5 is empty on the base side
    _, idx, _ = _check_pixels("groups", q, b, groups=(qg, bg))
    assert bool((idx[qg == 5] == -1).all()) and bool((qg == 5).any())
    _check_pixels("groups chunked", q, b, groups=(qg, bg), chunk=64)
    # chunks handed over one at a time (the base set need not be resident at once)
    qd, bd = torch.from_numpy(q).to(DEV), torch.from_numpy(b).to(DEV)
    one = N.nearest_pixels(qd, bd)
    it = N.nearest_pixels(qd, (bd[s:s + 77] for s in range(0, 300, 77)))
    assert all(torch.equal(a, c) for a, c in zip(one, it))


def test_pixels_against_the_reference_fp32_lines():
    """duplicates.py:993-1002 on the CPU in fp32 (ToTensor + Normalize frames, torch.sum(torch.abs(eval_img - train_images)), batches
    of 256 with a strict '<' between batches) picks the kernel's frame wherever the exact top-2 margin exceeds twice the
    reference's own worst rounding error on these pairs."""
    rng = np.random.default_rng(3)
    N = _N()
    q = rng.integers(0, 256, (24, 3, 224, 224), dtype=np.uint8)
    b = rng.integers(0, 256, (600, 3, 224, 224), dtype=np.uint8)
    for k in range(24):                                      # planted neighbours on a random background
        b[23 * k + 11] = q[k]
        for _ in range(3 + k):
            c, y, x = rng.integers(3), rng.integers(224), rng.integers(224)
            b[23 * k + 11, c, y, x] ^= 1
    mean, std = torch.tensor(N.IMAGENET_MEAN).view(1, 3, 1, 1), torch.tensor(N.IMAGENET_STD).view(1, 3, 1, 1)
    norm = lambda a: (torch.from_numpy(a).float().div(255.0) - mean) / std
    bn = norm(b)
    ref_idx, ref_d = [], []
    for i in range(len(q)):
        e = norm(q[i:i + 1])[0]
        best, best_j, row = float("inf"), -1, []
        for s in range(0, len(b), 256):
            distance = torch.sum(torch.abs(e - bn[s:s + 256]), dim=(1, 2, 3))
            row.append(distance)
            if float(torch.min(distance)) < best:
                best, best_j = float(torch.min(distance)), s + int(torch.argmin(distance))
        ref_idx.append(best_j)
        ref_d.append(torch.cat(row).double().numpy())
    ref_d = np.stack(ref_d)
    dist, idx, _ = N.nearest_pixels(torch.from_numpy(q).to(DEV), torch.from_numpy(b).to(DEV))
    dist, idx = dist.cpu().numpy(), idx.cpu().numpy()
    qi, bi = q.reshape(24, 3, -1).astype(np.int16), b.reshape(600, 3, -1).astype(np.int16)
    w = N.pixel_weights(N.IMAGENET_STD)
    exact = np.stack([sum(np.abs(qi[i][None] - bi).sum(axis=2, dtype=np.int64)[:, c] * w[c] for c in range(3)) for i in range(24)])
    ref_err = float(np.abs(ref_d - exact).max())
    top2 = np.sort(exact, axis=1)[:, :2]
    decided = (top2[:, 1] - top2[:, 0]) > 2 * ref_err
    print(f"[pixels vs fp32 reference] reference worst rounding error {ref_err:.3e} on distances up to {exact.max():.3e}; "
          f"{int((~decided).sum())} of {len(q)} cases left out")
    assert int((~decided).sum()) == 0
    assert np.array_equal(idx[decided], np.array(ref_idx)[decided])
    assert idx.tolist() == [23 * k + 11 for k in range(24)]
    assert float(np.abs(dist - exact[np.arange(24), idx]).max()) == 0.0


# ---- end to end -------------------------------------------------------------------------------------------------------------------
def test_script_end_to_end(tmp_path):
    N = _N()
    out = tmp_path / "dup"
    r = subprocess.run([sys.executable, os.path.join(ROOT, "nearest_neighbors.py"), "--dataset", "synthetic", "--space", "both",
                        "--random_init", "--out_dir", str(out)], cwd=tmp_path, capture_output=True, text=True, timeout=600)
    assert r.returncode == 0, r.stdout[-3000:] + r.stderr[-3000:]
    d = N.synthetic_sets(0)
    rows = list(csv.reader(open(out / "matched_results.csv")))
    assert rows[0] == ["eval_filename", "train_filename", "cosine_sim", "matched"] and len(rows) == 1 + len(d["eval_names"])
    matches = json.load(open(out / "max_cosine_sims.json"))
    assert set(matches[0]) == {"train_frame", "eval_frame", "max_cosine_sim"} and len(matches) == len(d["eval_names"])
    recs = json.load(open(out / "nn_pixel_space_results.json"))
    assert set(recs[0]) == {"eval_frame", "eval_label", "min_label", "min_frame", "min_distance", "correct"}
    by_eval_feat = {row[0]: row[1] for row in rows[1:]}
    by_eval_same = {m["eval_frame"]: m["train_frame"] for m in matches}
    by_eval_pix = {rec["eval_frame"]: rec for rec in recs}
    for e, t, kind in d["planted"]:                          # every planted duplicate is found in both spaces
        en, tn = d["eval_names"][e], d["train_names"][t]
        assert by_eval_feat[en] == tn and by_eval_same[en] == tn and by_eval_pix[en]["min_frame"] == tn, (kind, en)
        assert by_eval_pix[en]["correct"] and (by_eval_pix[en]["min_distance"] == 0.0) == (kind == "duplicate")
    # the 1-NN accuracy equals the host restatement (float64 cosine + argmax, duplicates.py:805-816) on the features the call extracted
    f = np.load(out / "features.npz")
    ef, tf = f["eval_features"].astype(np.float64), f["train_features"].astype(np.float64)
    assert ef.shape == (len(d["eval_names"]), 2048) and tf.shape == (len(d["train_names"]), 2048)
    sims = (ef / np.maximum(np.linalg.norm(ef, axis=1, keepdims=True), 1e-8)) @ (tf / np.maximum(np.linalg.norm(tf, axis=1, keepdims=True), 1e-8)).T
    pred = [d["train_labels"][j] for j in sims.argmax(axis=1)]
    summary = json.load(open(out / "nn_features_summary.json"))
    hits = [p == l for p, l in zip(pred, d["eval_labels"])]
    assert summary["total"] == sum(hits) / len(hits)
    for cat in sorted(set(d["eval_labels"])):
        mine = [h for h, l in zip(hits, d["eval_labels"]) if l == cat]
        assert summary["per_category"][cat] == sum(mine) / len(mine)
        assert f"Accuracy for {cat}: {sum(mine) / len(mine)}" in r.stdout
    assert f"Total accuracy: {sum(hits) / len(hits)}" in r.stdout and "Proportion of max cosine sims between 0.9 and 1:" in r.stdout
