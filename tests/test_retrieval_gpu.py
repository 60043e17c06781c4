"""Retrieval ranks on the MI355X (csrc/neighbors.hip cvcl_rank_cosine, multimodal/retrieval.py, retrieval.py) against the float64
numpy restatement of tests/retrieval_common.py -- never against the library.

Exact cases: features from {-1, +1}, where the integer dots order the rows exactly and every tie is a true tie, so the ranks must
equal the reference for every query.  Float cases: Gaussian features, every rank inside the bracket that delta = (D + 2) 2^-24 leaves
open, exactly where the bracket is tight; that at most 10 % of the brackets are loose is asserted from the float64 reference alone.
Beside that the anchors that need no tolerance: the single-target form against cvcl_knn_cosine's lists, chunks in both orders, strided
and misaligned operands, the threshold outputs against nearest_cosine bit for bit."""
import functools
import json
import os
import subprocess
import sys

import numpy as np
import pytest
import torch

from conftest import ROOT
from retrieval_common import bracket, check_bracket, exact_ranks, pair_keys, sign_features

pytestmark = pytest.mark.gpu

DEV = "cuda:0"
SHAPES = [(1, 1, 1), (127, 65, 5), (129, 129, 127), (33, 300, 129), (129, 513, 512), (2049, 4097, 64)]
FLOAT_CASES = [(129, 4097, 32, 1000), (257, 1025, 130, 300)]


def _R():
    from multimodal import retrieval
    return retrieval


def _N():
    from multimodal import neighbors
    return neighbors


def _ranks(q, b, qk, bk, **kw):
    rank, cos, idx = _R().retrieval_ranks(torch.from_numpy(q).to(DEV), torch.from_numpy(b).to(DEV), qk, bk, **kw)
    torch.cuda.synchronize()
    return rank.cpu().numpy(), cos.cpu(), idx.cpu()


@functools.lru_cache(maxsize=None)
def _sign_case(Nq, Nb, D):
    """seeded +-1 rows (computed once, shared, never modified)"""
    rng = np.random.default_rng(1000 * Nq + Nb + D)
    return sign_features(rng, Nq, D), sign_features(rng, Nb, D)


@functools.lru_cache(maxsize=None)
def _float_case(Nq, Nb, D, n_keys, seed):
    """seeded Gaussian rows and random keys with their float64 bracket (computed once, shared, never modified)"""
    rng = np.random.default_rng(seed)
    q, b = rng.standard_normal((Nq, D)).astype(np.float32), rng.standard_normal((Nb, D)).astype(np.float32)
    qk, bk = rng.integers(0, n_keys, Nq).astype(np.int64), rng.integers(0, n_keys, Nb).astype(np.int64)
    return q, b, qk, bk, bracket(q, b, qk, bk)


# ---- 1. exact ranks, ties included ---------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("Nq,Nb,D", SHAPES)
def test_exact_ranks_with_ties(Nq, Nb, D):
    q, b = _sign_case(Nq, Nb, D)
    rng = np.random.default_rng(7 * Nq + Nb)
    for G in sorted({Nb, max(1, Nb // 4), max(1, Nb // 8)}):          # 1, 4..5 and 8..9 positives per key (Nb < 8: fewer keys)
        bk = np.arange(Nb, dtype=np.int64) % G
        qk = rng.integers(0, G + max(1, G // 8), Nq).astype(np.int64)      # keys >= G match no row
        want, want_idx = exact_ranks(q, b, qk, bk)
        got, _, got_idx = _ranks(q, b, qk, bk)
        n_none = int((want < 0).sum())
        # (small D) the ranks that the tie rule decides: those that change when the rows come in the opposite order
        n_tied = int(((want >= 0) & (want != exact_ranks(q, b[::-1], qk, bk[::-1])[0])).sum()) if D <= 5 else -1
        print(f"[exact] Nq {Nq} Nb {Nb} D {D} G {G}: {n_none} queries without a positive, {n_tied} ranks that depend on the tie rule "
              f"(-1: not counted), {int((got != want).sum())} mismatches")
        assert np.array_equal(got_idx.numpy(), want_idx)
        assert np.array_equal(got, want), np.nonzero(got != want)[0][:10]
        if Nq >= 33:
            assert n_none > 0 and n_none < Nq
        if D <= 5 and Nq > 1:
            assert n_tied > 0                                         # the lower-index rule decides on both sides of thr_idx


# ---- 2. single-target form against the merged top-k search -------------------------------------------------------------------------
@pytest.mark.parametrize("Nq,Nb,D", SHAPES)
def test_single_target_form_agrees_with_the_top_k_lists(Nq, Nb, D):
    q, b = _sign_case(Nq, Nb, D)
    target = np.random.default_rng(3 * Nq + Nb).integers(0, Nb, Nq).astype(np.int64)
    got, _, got_idx = _ranks(q, b, target, np.arange(Nb, dtype=np.int64))
    assert np.array_equal(got_idx.numpy(), target)
    assert np.array_equal(got, exact_ranks(q, b, target, np.arange(Nb, dtype=np.int64))[0])
    for k in (1, 5, 64):
        _, idx = _N().knn_cosine(torch.from_numpy(q).to(DEV), torch.from_numpy(b).to(DEV), k)
        in_list = (idx.cpu().numpy() == target[:, None]).any(axis=1)
        assert np.array_equal(got < k, in_list), (k, np.nonzero((got < k) != in_list)[0][:10])


# ---- 3. float inputs, bracketed --------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("seed", [0, 1, 2])
@pytest.mark.parametrize("Nq,Nb,D,n_keys", FLOAT_CASES)
def test_float_ranks_inside_the_float64_bracket(Nq, Nb, D, n_keys, seed):
    q, b, qk, bk, (lo, hi, has) = _float_case(Nq, Nb, D, n_keys, seed)
    n_ranked, n_loose = int(has.sum()), int((has & (lo != hi)).sum())
    print(f"[float] Nq {Nq} Nb {Nb} D {D} keys {n_keys} seed {seed}: {n_ranked} ranked, {Nq - n_ranked} without a positive, "
          f"{n_loose} loose brackets ({100.0 * n_loose / max(n_ranked, 1):.1f} %)")
    assert n_ranked > Nq // 2 and n_loose <= 0.10 * n_ranked           # from the reference alone
    got, _, _ = _ranks(q, b, qk, bk)
    assert check_bracket(got, lo, hi, has) == n_loose


# ---- 4. chunking, strides, alignment -----------------------------------------------------------------------------------------------------
def _entry(q, ldq, b, ldb, Nq, n, D, qk, bk, thr_cos, thr_idx, offset, accumulate, rank):
    from multimodal import _hip as H
    lib = H.lib()
    ws = torch.empty(lib.cvcl_rank_cosine_workspace_bytes(Nq, n, D), dtype=torch.uint8, device=DEV)
    H.check(lib.cvcl_rank_cosine(q.data_ptr(), ldq, b.data_ptr(), ldb, Nq, n, D, 1e-8, qk.data_ptr(), bk.data_ptr(), thr_cos.data_ptr(),
                                 thr_idx.data_ptr(), offset, accumulate, rank.data_ptr(), ws.data_ptr(), ws.numel(), H.stream_ptr()),
            "cvcl_rank_cosine")
    torch.cuda.synchronize()


def test_chunks_in_either_order_strides_and_alignment():
    Nq, Nb, D = 129, 4097, 32
    q, b, qk, bk, (lo, hi, has) = _float_case(Nq, Nb, D, 1000, 0)
    one_shot, thr_cos, thr_idx = _ranks(q, b, qk, bk)
    check_bracket(one_shot, lo, hi, has)
    assert np.array_equal(_ranks(q, b, qk, bk, chunk=1000)[0], one_shot)               # the library's own chunk loop
    qd, bd = torch.from_numpy(q).to(DEV), torch.from_numpy(b).to(DEV)
    qkd, bkd = torch.from_numpy(qk).to(DEV).int(), torch.from_numpy(bk).to(DEV).int()
    tc, ti = thr_cos.to(DEV), thr_idx.to(DEV)
    chunks = [(0, 1000), (1000, 1000), (2000, 2097)]
    for order in (chunks, chunks[::-1]):
        rank = torch.full((Nq,), 12345, dtype=torch.int64, device=DEV)              # (the first call overwrites)
        for n_call, (s, n) in enumerate(order):
            _entry(qd, D, bd[s:], D, Nq, n, D, qkd, bkd[s:], tc, ti, s, int(n_call > 0), rank)
        assert np.array_equal(rank.cpu().numpy(), one_shot), order
    # row strides above D
    qs, bs = torch.zeros(Nq, D + 8, device=DEV), torch.zeros(Nb, D + 4, device=DEV)
    qs[:, :D], bs[:, 4:] = qd, bd
    rank = torch.zeros(Nq, dtype=torch.int64, device=DEV)
    _entry(qs, D + 8, bs[:, 4:], D + 4, Nq, Nb, D, qkd, bkd, tc, ti, 0, 0, rank)
    assert np.array_equal(rank.cpu().numpy(), one_shot)
    assert np.array_equal(_ranks_views(qs[:, :D], bs[:, 4:], qk, bk), one_shot)
    # a base pointer that is not 16-byte aligned, with a stride that is no multiple of 4: the scalar-load path
    flat = torch.zeros(Nb * (D + 1) + 1, device=DEV)
    bm = flat[1:].view(Nb, D + 1)
    bm[:, :D] = bd
    assert bm.data_ptr() % 16 == 4
    rank = torch.zeros(Nq, dtype=torch.int64, device=DEV)
    _entry(qd, D, bm, D + 1, Nq, Nb, D, qkd, bkd, tc, ti, 0, 0, rank)
    assert np.array_equal(rank.cpu().numpy(), one_shot)


def _ranks_views(qv, bv, qk, bk):
    rank = _R().retrieval_ranks(qv, bv, qk, bk)[0]
    torch.cuda.synchronize()
    return rank.cpu().numpy()


# ---- 5. the threshold outputs ------------------------------------------------------------------------------------------------------------
def test_best_positive_is_the_grouped_nearest_search_and_calls_repeat():
    q, b, qk, bk, _ = _float_case(257, 1025, 130, 300, 1)
    qd, bd = torch.from_numpy(q).to(DEV), torch.from_numpy(b).to(DEV)
    R = _R()
    rank, cos, idx = R.retrieval_ranks(qd, bd, qk, bk)
    want_cos, want_idx = _N().nearest_cosine(qd, bd, qk, bk)
    assert cos.dtype == torch.float32 and idx.dtype == torch.int64 and rank.dtype == torch.int64 and rank.is_cuda
    assert torch.equal(cos, want_cos) and torch.equal(idx, want_idx)
    assert torch.equal((idx < 0), (rank < 0)) and bool((cos[idx < 0] == float("-inf")).all())
    rank2, cos2, idx2 = R.retrieval_ranks(qd, bd, qk, bk)
    assert torch.equal(rank, rank2) and torch.equal(cos, cos2) and torch.equal(idx, idx2)
    rank3, cos3, idx3 = R.retrieval_ranks(qd, bd, qk, bk, chunk=300)
    assert torch.equal(rank, rank3) and torch.equal(cos, cos3) and torch.equal(idx, idx3)


# ---- 6. end to end -------------------------------------------------------------------------------------------------------------------------
SUMMARY_KEYS = {"n_queries", "n_without_positive", "recall@1", "recall@5", "recall@10", "median_rank", "mean_rank", "mrr",
                "chance_recall@1", "chance_recall@5", "chance_recall@10"}


def test_script_end_to_end(tmp_path):
    out = tmp_path / "ret"
    r = subprocess.run([sys.executable, os.path.join(ROOT, "retrieval.py"), "--dataset", "synthetic", "--random_init", "--split", "val",
                        "--save_features", "--out", str(out)], cwd=tmp_path, capture_output=True, text=True, timeout=600)
    assert r.returncode == 0, r.stdout[-3000:] + r.stderr[-3000:]
    rec = json.load(open(out / "retrieval.json"))
    assert set(rec) == {"image_to_text", "text_to_image", "split", "N", "n_texts", "precision", "checkpoint"}
    assert rec["split"] == "val" and rec["precision"] == "32" and rec["checkpoint"] is None
    image, text, ids = np.load(out / "features_image.npy"), np.load(out / "features_text.npy"), np.load(out / "text_ids.npy")
    N = rec["N"]
    assert image.shape == text.shape == (N, 512) and ids.shape == (N,) and N == 64          # the synthetic split: one batch of pairs
    dense, first = pair_keys(ids)
    T = len(first)
    assert rec["n_texts"] == T
    sides = {"image_to_text": (image, text[first], dense, np.arange(T)), "text_to_image": (text[first], image, np.arange(T), dense)}
    for name, (q, b, qk, bk) in sides.items():
        s = rec[name]
        assert set(s) == SUMMARY_KEYS, name
        assert s["n_queries"] + s["n_without_positive"] == len(q) and s["n_without_positive"] == 0
        assert 0.0 <= s["recall@1"] <= s["recall@5"] <= s["recall@10"] <= 1.0
        ranks = np.load(out / f"ranks_{name}.npy")
        assert ranks.shape == (len(q),) and ranks.dtype == np.int64
        check_bracket(ranks, *bracket(q, b, qk, bk))
        assert s["recall@5"] == float(np.mean(ranks < 5)) and s["median_rank"] == float(np.median(ranks + 1.0))
        assert f"{name}: R@1 {s['recall@1']:.4f}" in r.stdout


def test_text_features_that_are_the_image_features_retrieve_perfectly(tmp_path, monkeypatch):
    """encode_text patched (here, not in the product) to hand back the features encode_image gave for the same pairs, their
    columns moved by one fixed permutation on both sides: every pair's cosine is 1, so recall@1 is 1.0 both ways"""
    from multimodal.multimodal import MultiModalModel
    R = _R()
    perm = torch.randperm(512, generator=torch.Generator().manual_seed(5)).to(DEV)
    seen = []
    encode_image = MultiModalModel.encode_image

    def image_side(self, image):
        f, fmap = encode_image(self, image)
        seen.append(f[:, perm].contiguous())
        return seen[-1], fmap

    def text_side(self, text, text_length):
        assert seen[-1].shape[0] == text.shape[0]
        return seen[-1].clone(), None

    monkeypatch.setattr(MultiModalModel, "encode_image", image_side)
    monkeypatch.setattr(MultiModalModel, "encode_text", text_side)
    rec = R.main(R.parser().parse_args(["--dataset", "synthetic", "--random_init", "--split", "test", "--out", str(tmp_path / "perm")]))
    for name in ("image_to_text", "text_to_image"):
        assert rec[name]["recall@1"] == 1.0 and rec[name]["median_rank"] == 1.0 and rec[name]["n_without_positive"] == 0, rec[name]
