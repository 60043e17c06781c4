"""The k-nearest-neighbour search and the weighted vote on the MI355X (csrc/neighbors.hip cvcl_knn_cosine / cvcl_knn_vote,
multimodal/neighbors.py knn_cosine / knn_vote / knn_classify).

Search.  The reference value is the float64 cosine on the CPU, evaluated as a product of rows normalised in float64, in row blocks,
as tests/test_neighbors_gpu.py::_check_cosine does.  tau = 4 x the worst error of torch's own fp32 cosine against float64 on the same
inputs (evaluated the same way in fp32 on the CPU): a tiled MFMA sum and torch's sum order differ and both are legitimate fp32
evaluations; tau is measured against the reference arithmetic, not against the kernel, and every case prints it with the kernel's own
figures before asserting.  Per query: the list is sorted by (cos desc, idx asc) and holds no index twice; every value is within tau
of cos64 at its index; the set is right -- (the k-th largest cos64 of the row) - (the smallest cos64 among the returned indices) <=
tau; slots beyond the eligible count hold -inf / -1.  Beside that, bit-exact anchors: k = 1 and the first column at k = 20 against
nearest_cosine (and at k = 5 on the scalar-load path, with ragged tiles and groups), strided against contiguous inputs, chunked against one-shot, grouped against the ungrouped search per group.

Vote.  scores are compared against numpy float64 sums of exp(cos / T) over the same lists, T being the fp32 value the entry
receives.  Bound on the relative error, 2^-22: the kernel forms the weights and the sum in double and rounds ONCE to fp32.  One
rounding to fp32 moves a value by at most one unit in the last place, 2^-23 relative (half of that in round-to-nearest); the double
exp of the device library may differ from libm's in its last place, 2^-52 relative per weight, and the double sums of at most 256
positive terms add at most 256 x 2^-53 -- both vanish beside 2^-23.  Doubled for slack that does not depend on the code under test:
2^-22.  pred must equal the float64 arg-max wherever the float64 top-2 margin exceeds that bound times the top score; the seeded
inputs leave 0 queries out, which the test asserts."""
import csv
import functools
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
NEG_INF = float("-inf")
VOTE_BOUND = 2.0 ** -22


def _N():
    from multimodal import neighbors
    return neighbors


def _knn(q, b, k, **kw):
    cos, idx = _N().knn_cosine(q.to(DEV), b.to(DEV), k, **kw)
    torch.cuda.synchronize()
    return cos.cpu(), idx.cpu()


def _nearest(q, b, **kw):
    cos, idx = _N().nearest_cosine(q.to(DEV), b.to(DEV), **kw)
    torch.cuda.synchronize()
    return cos.cpu(), idx.cpu()


def _check_knn(name, q, b, k, got_cos, got_idx, eligible=None, block=256):
    """all per-query checks over all queries; returns tau"""
    Nq, Nb = q.shape[0], b.shape[0]
    assert tuple(got_cos.shape) == (Nq, k) == tuple(got_idx.shape) and got_cos.dtype == torch.float32 and got_idx.dtype == torch.int64
    qn64 = q.double() / q.double().norm(dim=1, keepdim=True).clamp_min(1e-8)
    bn64 = b.double() / b.double().norm(dim=1, keepdim=True).clamp_min(1e-8)
    qn32 = q / q.norm(dim=1, keepdim=True).clamp_min(1e-8)
    bn32 = b / b.norm(dim=1, keepdim=True).clamp_min(1e-8)
    torch_err, val_err, set_gap = 0.0, 0.0, 0.0
    order_ok = unique_ok = tail_ok = True
    for s in range(0, Nq, block):
        c64 = qn64[s:s + block] @ bn64.T
        c32 = qn32[s:s + block] @ bn32.T
        torch_err = max(torch_err, float((c32.double() - c64).abs().max()))
        if eligible is not None:
            c64 = c64.masked_fill(~eligible[s:s + block], NEG_INF)
        gc, gi = got_cos[s:s + block], got_idx[s:s + block]
        n_elig = torch.isfinite(c64).sum(dim=1)
        keff = n_elig.clamp_max(k)                                    # entries each list must hold
        slot = torch.arange(k)[None, :]
        held = slot < keff[:, None]
        tail_ok &= bool(((gi >= 0) == held).all()) and bool((gi[~held] == -1).all()) and bool((gc[~held] == NEG_INF).all())
        tail_ok &= bool((gi < Nb).all())
        at = c64.gather(1, gi.clamp(0, Nb - 1))                       # cos64 at the returned indices
        if bool(held.any()):
            val_err = max(val_err, float((gc.double() - at)[held].abs().max()))
        # sorted by (cos desc, idx asc) over the held prefix
        both = held[:, 1:]
        a_c, b_c, a_i, b_i = gc[:, :-1], gc[:, 1:], gi[:, :-1], gi[:, 1:]
        order_ok &= bool((((a_c > b_c) | ((a_c == b_c) & (a_i < b_i))) | ~both).all())
        # no index twice: the held indices of a row, sorted, strictly increase
        srt = torch.where(held, gi, torch.arange(Nb, Nb + k)[None, :]).sort(dim=1).values
        unique_ok &= bool((srt[:, 1:] > srt[:, :-1]).all())
        # the set: the keff-th largest cos64 of the row against the smallest cos64 among the returned
        top = c64.topk(min(k, Nb), dim=1).values
        has = keff > 0
        if bool(has.any()):
            kth = top.gather(1, (keff - 1).clamp_min(0)[:, None])[:, 0]
            worst = at.masked_fill(~held, float("inf")).min(dim=1).values
            set_gap = max(set_gap, float((kth - worst)[has].max()))
    tau = 4.0 * torch_err
    print(f"[knn {name}] Nq {Nq} Nb {Nb} D {q.shape[1]} k {k}: torch fp32 worst error {torch_err:.3e} -> tau {tau:.3e}; kernel "
          f"|cos - cos64 at its index| {val_err:.3e}; cos64 gap of the returned set {set_gap:.3e}; sorted {order_ok}, "
          f"unique {unique_ok}, tails {tail_ok}")
    assert tail_ok, name
    assert order_ok, name
    assert unique_ok, name
    assert val_err <= tau, (name, val_err, tau)
    assert set_gap <= tau, (name, set_gap, tau)
    return tau


@functools.lru_cache(maxsize=None)
def _gaussian_case(Nq, Nb, D, k):
    """seeded Gaussian rows and the lists the search returns for them (computed once, shared, never modified)"""
    g = torch.Generator().manual_seed(1000 * Nq + Nb + D + k)
    q, b = torch.randn(Nq, D, generator=g), torch.randn(Nb, D, generator=g)
    cos, idx = _knn(q, b, k)
    return q, b, cos, idx


# ---- shapes ---------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("Nq,Nb,D,k", [
    (1, 1, 7, 1),
    (3, 2, 33, 2),
    (3, 2, 33, 5),                                            # k above Nb
    (129, 127, 130, 64),
    (257, 300, 2048, 20),
    (64, 1000, 100, 256),                                     # several base splits at the maximum k
    (300, 20000, 2048, 20),                                   # one mid-size case on Gaussian rows
])
def test_lists_against_float64(Nq, Nb, D, k):
    q, b, cos, idx = _gaussian_case(Nq, Nb, D, k)
    _check_knn("gaussian", q, b, k, cos, idx)


# ---- bit-exact anchors ----------------------------------------------------------------------------------------------------------------
def test_k1_and_first_column_equal_the_argmax_search():
    g = torch.Generator().manual_seed(11)
    q, b = torch.randn(257, 512, generator=g), torch.randn(1000, 512, generator=g)
    want_cos, want_idx = _nearest(q, b)
    cos1, idx1 = _knn(q, b, 1)
    assert torch.equal(cos1[:, 0], want_cos) and torch.equal(idx1[:, 0], want_idx)
    cos20, idx20 = _knn(q, b, 20)
    assert torch.equal(cos20[:, 0], want_cos) and torch.equal(idx20[:, 0], want_idx)
    _check_knn("anchor k 20", q, b, 20, cos20, idx20)


def test_k1_and_first_column_equal_the_argmax_search_on_the_scalar_path():
    """the anchor above on the kernels' scalar-load instantiation, with ragged tiles and groups: 130 and 257 rows are a full tile and
    a ragged one on both sides, D = 33 is two k steps (the second nearly empty) and rules out 16-byte loads; then the same rows
    through a row stride that is no multiple of 4"""
    g = torch.Generator().manual_seed(18)
    Nq, Nb, D = 130, 257, 33
    q, b = torch.randn(Nq, D, generator=g), torch.randn(Nb, D, generator=g)
    qg, bg = (torch.arange(Nq) % 3).int(), ((torch.arange(Nb) * 7) % 3).int()
    qg, bg = qg[torch.randperm(Nq, generator=g)], bg[torch.randperm(Nb, generator=g)]
    assert sorted(set(qg.tolist())) == sorted(set(bg.tolist())) == [0, 1, 2]
    kw = dict(query_groups=qg, base_groups=bg)
    want_cos, want_idx = _nearest(q, b, **kw)
    assert bool((want_idx >= 0).all())
    cos1, idx1 = _knn(q, b, 1, **kw)
    assert torch.equal(cos1[:, 0], want_cos) and torch.equal(idx1[:, 0], want_idx)
    cos5, idx5 = _knn(q, b, 5, **kw)
    assert torch.equal(cos5[:, 0], want_cos) and torch.equal(idx5[:, 0], want_idx)
    _check_knn("scalar path k 5", q, b, 5, cos5, idx5, eligible=qg[:, None] == bg[None, :])
    qs, bs = torch.zeros(Nq, 35), torch.zeros(Nb, 35)                      # 35-wide storage, the first 33 columns are the rows
    qs[:, :D], bs[:, :D] = q, b
    qv, bv = qs.to(DEV)[:, :D], bs.to(DEV)[:, :D]
    assert qv.stride(0) == 35 and bv.stride(0) == 35
    N = _N()
    got = [N.nearest_cosine(qv, bv, **kw), N.knn_cosine(qv, bv, 1, **kw), N.knn_cosine(qv, bv, 5, **kw)]
    torch.cuda.synchronize()
    for (gc, gi), (wc, wi) in zip(got, [(want_cos, want_idx), (cos1, idx1), (cos5, idx5)]):
        assert torch.equal(gc.cpu(), wc) and torch.equal(gi.cpu(), wi)


def test_strided_inputs_equal_contiguous_inputs():
    g = torch.Generator().manual_seed(12)
    N = _N()
    qs, bs = torch.randn(130, 520, generator=g).to(DEV), torch.randn(777, 640, generator=g).to(DEV)      # D = 512, strides above D
    q, b = qs[:, :512], bs[:, 64:576]
    assert q.stride(0) == 520 and b.stride(0) == 640
    cos, idx = N.knn_cosine(q, b, 20)
    cos_p, idx_p = N.knn_cosine(q.contiguous(), b.contiguous(), 20)
    assert torch.equal(cos, cos_p) and torch.equal(idx, idx_p)
    _check_knn("D512 strided", q.cpu().contiguous(), b.cpu().contiguous(), 20, cos.cpu(), idx.cpu())


def _tie_rows(g, D=256):
    q, b = torch.randn(5, D, generator=g), torch.randn(900, D, generator=g)
    pairs = ((3, 4), (100, 700), (127, 128), (5, 899))
    for j, (lo, hi) in enumerate(pairs):
        b[lo] = q[j]
        b[hi] = q[j]
    five = (120, 126, 130, 200, 250)                          # one row five times, across the tiles 0..127 and 128..255
    for r in five:
        b[r] = q[4]
    return q, b, pairs, five


def test_chunks_equal_one_shot_and_ties_come_out_in_index_order():
    g = torch.Generator().manual_seed(13)
    q, b, pairs, five = _tie_rows(g)
    cos, idx = _knn(q, b, 20)
    _check_knn("ties", q, b, 20, cos, idx)
    for j, (lo, hi) in enumerate(pairs):
        assert idx[j, :2].tolist() == [lo, hi] and float(cos[j, 0]) == float(cos[j, 1]), (j, idx[j, :3], cos[j, :3])
    assert idx[4, :5].tolist() == list(five) and bool((cos[4, :5] == cos[4, 0]).all())
    for chunk in (1, 128, 500):                               # equal cosines meet across chunk boundaries too
        cc, ii = _knn(q, b, 20, chunk=chunk)
        assert torch.equal(cc, cos) and torch.equal(ii, idx), chunk
    # Gaussian rows, k beyond a chunk's rows
    g = torch.Generator().manual_seed(14)
    q, b = torch.randn(70, 96, generator=g), torch.randn(900, 96, generator=g)
    cos, idx = _knn(q, b, 150)
    for chunk in (1, 128, 500):
        cc, ii = _knn(q, b, 150, chunk=chunk)
        assert torch.equal(cc, cos) and torch.equal(ii, idx), chunk


def test_order_adversaries():
    """base rows in ascending similarity to the queries: every tile beats the threshold; and the same rows in descending order"""
    g = torch.Generator().manual_seed(15)
    Nq, Nb, D, k = 130, 1500, 64, 64
    q0 = torch.randn(D, generator=g)
    q = q0[None, :] + 0.1 * torch.randn(Nq, D, generator=g)
    q[0] = q0
    alpha = torch.linspace(0.0, 3.0, Nb)
    b = alpha[:, None] * q0[None, :] + torch.randn(Nb, D, generator=g)
    c0 = (b.double() @ q0.double()) / b.double().norm(dim=1)
    assert float(c0[-200:].min()) > float(c0[:200].max())    # (the trend is there)
    cos, idx = _knn(q, b, k)
    _check_knn("ascending", q, b, k, cos, idx)
    bd = b.flip(0).contiguous()
    cos_d, idx_d = _knn(q, bd, k)
    _check_knn("descending", q, bd, k, cos_d, idx_d)
    # the same rows either way: equal values, and equal rows wherever a list holds no two equal fp32 cosines (a tie's order flips)
    distinct = (cos[:, 1:] != cos[:, :-1]).all(dim=1)
    assert torch.equal(cos_d, cos) and torch.equal((Nb - 1 - idx_d)[distinct], idx[distinct]) and int(distinct.sum()) > Nq // 2


def test_groups():
    g = torch.Generator().manual_seed(16)
    D, G, k = 256, 22, 20
    sizes_b = [0 if c == 7 else (5 if c == 3 else 40 + 13 * c) for c in range(G)]      # group 7 empty, group 3 below k
    sizes_q = [3 + (c % 5) for c in range(G)]
    bg = torch.cat([torch.full((n,), c, dtype=torch.int32) for c, n in enumerate(sizes_b)])
    qg = torch.cat([torch.full((n,), c, dtype=torch.int32) for c, n in enumerate(sizes_q)])
    bg, qg = bg[torch.randperm(len(bg), generator=g)], qg[torch.randperm(len(qg), generator=g)]
    q, b = torch.randn(len(qg), D, generator=g), torch.randn(len(bg), D, generator=g)
    cos, idx = _knn(q, b, k, query_groups=qg, base_groups=bg)
    _check_knn("22 groups", q, b, k, cos, idx, eligible=qg[:, None] == bg[None, :])
    assert bool((idx[qg == 7] == -1).all()) and bool((cos[qg == 7] == NEG_INF).all()) and bool((qg == 7).any())
    assert bool((idx[qg == 3][:, :5] >= 0).all()) and bool((idx[qg == 3][:, 5:] == -1).all()) and bool((cos[qg == 3][:, 5:] == NEG_INF).all())
    for c in range(G):                                       # equals the ungrouped kernel run per group, bit for bit
        qi, bi = (qg == c).nonzero()[:, 0], (bg == c).nonzero()[:, 0]
        if len(bi) == 0:
            continue
        cc, ii = _knn(q[qi], b[bi], k)
        mapped = torch.where(ii >= 0, bi[ii.clamp_min(0)], torch.full_like(ii, -1))
        assert torch.equal(cc, cos[qi]) and torch.equal(mapped, idx[qi]), c
    cos_c, idx_c = _knn(q, b, k, query_groups=qg, base_groups=bg, chunk=101)
    assert torch.equal(cos_c, cos) and torch.equal(idx_c, idx)
    with pytest.raises(Exception):
        _N().knn_cosine(q.to(DEV), b.to(DEV), k, query_groups=qg)


# ---- vote -----------------------------------------------------------------------------------------------------------------------------
def _vote(cos, idx, labels, C, T):
    scores, pred = _N().knn_vote(cos.to(DEV), idx.to(DEV), labels.to(DEV), C, T)
    torch.cuda.synchronize()
    return scores.cpu().numpy(), pred.cpu().numpy()


def test_vote_scores_and_predictions_against_float64():
    _, _, cos, idx = _gaussian_case(257, 300, 2048, 20)
    C, T = 10, 0.07
    labels = torch.from_numpy(np.random.default_rng(17).integers(0, C, 300).astype(np.int32))
    scores, pred = _vote(cos, idx, labels, C, T)
    t32 = float(np.float32(T))                               # the entry takes the temperature in fp32
    w = np.exp(cos.numpy().astype(np.float64) / t32)
    lab = labels.numpy()[idx.numpy()]
    want = np.zeros((257, C))
    for j in range(20):                                      # in list order
        np.add.at(want, (np.arange(257), lab[:, j]), w[:, j])
    voted = want > 0
    rel = float((np.abs(scores.astype(np.float64) - want)[voted] / want[voted]).max())
    srt = np.sort(want, axis=1)
    decided = (srt[:, -1] - srt[:, -2]) > VOTE_BOUND * srt[:, -1]
    print(f"[vote] 257 lists of 20, C {C}, T {T}: worst relative score error {rel:.3e} (bound {VOTE_BOUND:.3e}); "
          f"{int((~decided).sum())} of 257 queries left out of the prediction check")
    assert bool((scores[~voted] == 0).all())
    assert rel <= VOTE_BOUND
    assert int((~decided).sum()) == 0
    assert np.array_equal(pred[decided], want.argmax(axis=1)[decided])


def test_vote_special_cases():
    C, Nb = 6, 40
    labels = torch.tensor([j % C for j in range(Nb)], dtype=torch.int32)
    labels[30] = -1                                          # labels outside [0, C)
    labels[31] = C
    cos = torch.tensor([[0.9, 0.8, 0.7, 0.6, 0.5, 0.4]] * 6, dtype=torch.float32)
    idx = torch.tensor([
        [2, 8, 1, 7, 0, 14],                                 # classes 2 2 1 1 0 2: counts 1 2 3
        [4, 10, 3, 9, 5, 12],                                # classes 4 4 3 3 5 0: 3 and 4 tie at 2 -> 3
        [5, 1, 2, 3, 4, 0],                                  # one each: class 0
        [4, 10, Nb, Nb + 1000, 2 ** 40, 3],                  # indices >= Nb are skipped: class 4 twice, class 3 once
        [30, 31, 30, 31, 9, -1],                             # labels outside the classes are skipped: class 3 once
        [-1, -1, -1, -1, -1, -1],                            # nothing counts
    ], dtype=torch.int64)
    scores, pred = _vote(cos, idx, labels, C, 0.0)           # T = 0: weight 1, integer counts
    want = np.array([[1, 2, 3, 0, 0, 0], [1, 0, 0, 2, 2, 1], [1, 1, 1, 1, 1, 1], [0, 0, 0, 1, 2, 0], [0, 0, 0, 1, 0, 0],
                     [0, 0, 0, 0, 0, 0]], dtype=np.float32)
    assert np.array_equal(scores, want), scores
    assert pred.tolist() == [2, 3, 0, 4, 3, -1]
    # the same lists weighted: skipped entries stay out, the empty list stays -1 with zero scores
    t32 = float(np.float32(0.07))
    scores, pred = _vote(cos, idx, labels, C, 0.07)
    w = np.exp(cos[0].numpy().astype(np.float64) / t32)
    assert abs(scores[3, 4] - (w[0] + w[1])) <= VOTE_BOUND * (w[0] + w[1]) and abs(scores[3, 3] - w[5]) <= VOTE_BOUND * w[5]
    assert abs(scores[4, 3] - w[4]) <= VOTE_BOUND * w[4] and float(np.abs(scores[4]).sum()) == float(scores[4, 3])
    assert bool((scores[5] == 0).all()) and pred.tolist()[3:] == [4, 3, -1]
    # more classes than threads of a workgroup, k = 1
    big = torch.arange(3000, dtype=torch.int32)
    scores, pred = _vote(torch.ones(3, 1), torch.tensor([[2999], [256], [0]]), big, 3000, 0.0)
    assert pred.tolist() == [2999, 256, 0] and scores.sum(axis=1).tolist() == [1.0, 1.0, 1.0] and scores[0, 2999] == 1.0


# ---- end to end -----------------------------------------------------------------------------------------------------------------------
def test_script_end_to_end_top_k(tmp_path):
    N = _N()
    out = tmp_path / "dup"
    r = subprocess.run([sys.executable, os.path.join(ROOT, "nearest_neighbors.py"), "--dataset", "synthetic", "--space", "features",
                        "--random_init", "--top_k", "5", "--out_dir", str(out)], cwd=tmp_path, capture_output=True, text=True, timeout=600)
    assert r.returncode == 0, r.stdout[-3000:] + r.stderr[-3000:]
    d = N.synthetic_sets(0)
    rows = list(csv.reader(open(out / "top_k_matches.csv")))
    assert rows[0] == ["eval_filename", "rank", "train_filename", "cosine_sim", "train_label"]
    assert len(rows) == 1 + 5 * len(d["eval_names"])
    by_eval = {}
    for e, rank, t, sim, label in rows[1:]:
        by_eval.setdefault(e, []).append((int(rank), t, float(sim), label))
    label_of = dict(zip(d["train_names"], d["train_labels"]))
    for e in d["eval_names"]:
        assert [x[0] for x in by_eval[e]] == [1, 2, 3, 4, 5] and len({x[1] for x in by_eval[e]}) == 5
        assert all(a[2] >= b[2] for a, b in zip(by_eval[e], by_eval[e][1:])) and all(label_of[x[1]] == x[3] for x in by_eval[e])
    matched = list(csv.reader(open(out / "matched_results.csv")))[1:]
    assert len(matched) == len(d["eval_names"])
    for e, t, sim, _ in matched:                             # the rank-1 rows are the arg-max search's rows
        assert by_eval[e][0][1] == t and by_eval[e][0][2] == float(sim)
    res = json.load(open(out / "knn_results.json"))
    assert set(res) == {"k", "temperature", "per_category", "total", "top5_total"} and res["k"] == 5 and res["temperature"] == 0.07
    assert sorted(res["per_category"]) == sorted(set(d["eval_labels"])) and 0.0 <= res["total"] <= res["top5_total"] <= 1.0
    for cat, acc in res["per_category"].items():
        assert f"5-NN accuracy for {cat}: {acc}" in r.stdout
    assert f"5-NN total accuracy (T = 0.07): {res['total']}" in r.stdout and f"5-NN top-5 accuracy: {res['top5_total']}" in r.stdout
    # the planted duplicates lead their lists
    for e, t, _ in d["planted"]:
        assert by_eval[d["eval_names"][e]][0][1] == d["train_names"][t]
