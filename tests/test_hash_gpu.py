"""The perceptual-hash kernels on the MI355X (csrc/phash.hip, multimodal/neighbors.py) against the numpy integer oracle of
tests/hash_common.py.  Everything is integer arithmetic, so every comparison is bit-exact and over all outputs: the rounded cells
and the hash words of ``average_hash``, the (distance, index) pairs of ``nearest_hamming`` and the (ratio, index) pairs of the
digit-string search, with the first arg-min / arg-max of numpy as the tie rule.

The end-to-end case runs ``synthetic_sets(0)``: its 8 planted frames (exact copies, and copies with +-1 on six pixels) must come back
at Hamming 0 and ratio 100 with their planted training frame; the oracle's values for the other 8 evaluation frames on this seed
are a smallest Hamming distance of 86 and a largest ratio of 51 (computed on the CPU), which the kernels must reproduce."""
import json
import os
import subprocess
import sys

import numpy as np
import pytest
import torch

import hash_common as HC
from conftest import ROOT

pytestmark = pytest.mark.gpu

DEV = "cuda:0"


def _N():
    from multimodal import neighbors
    return neighbors


def _hash(frames, layout="NCHW"):
    """numpy or torch frames -> (words int64 [N, 4], cells int64 [N, 256]) from the device"""
    t = frames if torch.is_tensor(frames) else torch.from_numpy(frames).to(DEV)
    words, cells = _N().average_hash(t, layout, return_cells=True)
    torch.cuda.synchronize()
    assert words.dtype == torch.int64 and cells.dtype == torch.int32 and words.is_cuda
    return words.cpu().numpy(), cells.cpu().numpy().astype(np.int64)


def _check_hash(frames_np, got):
    want_words, want_cells = HC.ahash(frames_np)
    assert np.array_equal(got[1], want_cells), "cells (the resize)"
    assert np.array_equal(got[0], want_words), "words (the threshold)"


# ---- average hash -----------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("n", [1, 3, 257])
@pytest.mark.parametrize("h,w", [(16, 16), (17, 31), (37, 50), (64, 64), (224, 224)])
def test_hash_random_frames(n, h, w):
    x = HC.random_frames(1000 * n + h + w, n, h, w)
    got = _hash(x)
    _check_hash(x, got)
    # two calls give the same bits
    again = _hash(x)
    assert np.array_equal(again[0], got[0]) and np.array_equal(again[1], got[1])


def test_hash_480_by_640():
    x = HC.random_frames(7, 2, 480, 640)
    _check_hash(x, _hash(x))


def test_hash_layouts_give_the_same_bits():
    x = HC.random_frames(8, 3, 37, 50)
    planar = _hash(x)
    rows = torch.from_numpy(np.ascontiguousarray(x.transpose(0, 2, 3, 1))).to(DEV)           # [N, H, W, 3], as the frame store keeps it
    assert rows.is_contiguous() and rows.shape == (3, 37, 50, 3)
    interleaved = _hash(rows, "NHWC")
    _check_hash(x, interleaved)
    assert np.array_equal(planar[0], interleaved[0]) and np.array_equal(planar[1], interleaved[1])
    # without the cells the words are the same
    assert np.array_equal(_N().average_hash(rows, "NHWC").cpu().numpy(), planar[0])


def test_hash_reads_a_crop_in_place():
    big = HC.random_frames(9, 3, 80, 90)
    t = torch.from_numpy(big).to(DEV)
    crop = t[:, :, 5:55, 7:71]
    assert not crop.is_contiguous()
    _check_hash(big[:, :, 5:55, 7:71], _hash(crop))
    every_other = t[::2, :, ::2, ::3]                                                         # strides above 1 in every place
    _check_hash(big[::2, :, ::2, ::3], _hash(every_other))


def test_hash_constant_and_saturated_frames():
    const = np.empty((2, 3, 40, 33), dtype=np.uint8)
    const[0, 0], const[0, 1], const[0, 2] = 12, 200, 77
    const[1] = 0
    words, cells = _hash(const)
    _check_hash(const, (words, cells))
    assert bool((words == -1).all())                                                          # every cell equals the mean: all 256 bits
    assert len(set(cells[0].tolist())) == 1 and bool((cells[1] == 0).all())
    white = np.full((3, 3, 224, 224), 255, dtype=np.uint8)
    words, cells = _hash(white)
    assert bool((cells == 255).all()) and bool((words == -1).all())


def test_hash_cells_equal_to_the_mean_are_set():
    frame, _ = HC.tie_frame()
    words, cells = _hash(frame)
    _check_hash(frame, (words, cells))
    assert int(cells.sum()) == 256 * 15
    bits = HC.bits_of_words(words)[0]
    assert np.array_equal(bits, cells[0] >= 15) and int(bits[cells[0] == 15].sum()) == 32 and int(bits.sum()) == 144


# ---- Hamming ----------------------------------------------------------------------------------------------------------------------
def _hamming(q, b, qg=None, bg=None):
    dist, idx = _N().nearest_hamming(torch.from_numpy(q).to(DEV), torch.from_numpy(b).to(DEV), qg, bg)
    torch.cuda.synchronize()
    assert dist.dtype == torch.int32 and idx.dtype == torch.int64
    return dist.cpu().numpy().astype(np.int64), idx.cpu().numpy()


def _check_hamming(q, b, qg=None, bg=None):
    eligible = np.ones((len(q), len(b)), dtype=bool) if qg is None else np.asarray(qg)[:, None] == np.asarray(bg)[None, :]
    want = HC.nearest(HC.hamming_matrix(q, b), eligible, True, HC.NO_MATCH)
    got = _hamming(q, b, qg, bg)
    assert np.array_equal(got[0], want[0]) and np.array_equal(got[1], want[1])
    return got


def test_hamming_one_by_one_and_the_sign_bits():
    q = np.array([[-1, -1, -1, -1]], dtype=np.int64)
    b = np.array([[0, 0, 0, np.iinfo(np.int64).min]], dtype=np.int64)
    dist, idx = _check_hamming(q, b)
    assert dist.tolist() == [255] and idx.tolist() == [0]
    dist, _ = _check_hamming(q, np.zeros((1, 4), dtype=np.int64))
    assert dist.tolist() == [256]
    # bit 63 of every word set on one side only
    top = np.full((2, 4), np.iinfo(np.int64).min, dtype=np.int64)
    top[1, 2] = 0
    dist, idx = _check_hamming(np.zeros((1, 4), dtype=np.int64), top)
    assert dist.tolist() == [3] and idx.tolist() == [1]


def test_hamming_ties_go_to_the_lower_index():
    b = HC.random_hashes(11, 1000)
    b[500:510] = b[20:30]                                       # duplicated base rows
    b[990] = b[3]
    q = HC.random_hashes(12, 33)
    q[:10] = b[20:30]
    q[10] = b[990]
    q[11] = HC.flip_bits(b[25], [0, 63, 64, 255])               # equally far from rows 25 and 505
    dist, idx = _check_hamming(q, b)
    assert idx[:12].tolist() == list(range(20, 30)) + [3, 25] and dist[:12].tolist() == [0] * 11 + [4]
    again = _hamming(q, b)
    assert np.array_equal(again[0], dist) and np.array_equal(again[1], idx)


def test_hamming_planted_copies_over_several_base_splits():
    b = HC.random_hashes(13, 70001)
    q = HC.random_hashes(14, 64)
    rng = np.random.default_rng(15)
    where = rng.choice(70001, 48, replace=False)
    where[:3] = [0, 70000, 35000]
    for i, j in enumerate(where):                               # copies at 0 to 3 flipped bits
        q[i] = HC.flip_bits(b[j], rng.choice(256, i % 4, replace=False))
    dist, idx = _check_hamming(q, b)
    assert idx[:48].tolist() == where.tolist() and dist[:48].tolist() == [i % 4 for i in range(48)]
    assert int(dist[48:].min()) > 3                             # (random 256-bit hashes: about 128 apart)


def test_hamming_groups():
    b = HC.random_hashes(16, 700)
    q = HC.random_hashes(17, 90)
    sizes = [1, 250, 0, 37, 412]                                # group 2 has no base row
    bg = np.repeat(np.arange(5), sizes).astype(np.int32)
    bg = bg[np.random.default_rng(18).permutation(700)]
    qg = (np.arange(90) % 5).astype(np.int32)
    dist, idx = _check_hamming(q, b, qg, bg)
    assert bool((idx[qg == 2] == -1).all()) and bool((dist[qg == 2] == 257).all()) and bool((idx[qg != 2] >= 0).all())
    # the grouped search is the ungrouped kernel run per group
    for g in (0, 1, 3, 4):
        rows = np.flatnonzero(bg == g)
        d, i = _hamming(q[qg == g], b[rows])
        assert np.array_equal(d, dist[qg == g]) and np.array_equal(rows[i], idx[qg == g])


# ---- ratio ------------------------------------------------------------------------------------------------------------------------
def _ratio(qs, bs, qg=None, bg=None, ld=HC.DIGITS_MAX):
    (qd, ql), (bd, bl) = HC.digit_rows(qs, ld), HC.digit_rows(bs, ld)
    t = lambda a: torch.from_numpy(a).to(DEV)
    ratio, idx = _N().nearest_digit_strings(t(qd), t(ql), t(bd), t(bl), qg, bg)
    torch.cuda.synchronize()
    assert ratio.dtype == torch.int32 and idx.dtype == torch.int64
    return ratio.cpu().numpy().astype(np.int64), idx.cpu().numpy()


def _check_ratio(qs, bs, qg=None, bg=None, ld=HC.DIGITS_MAX):
    (qd, ql), (bd, bl) = HC.digit_rows(qs, ld), HC.digit_rows(bs, ld)
    eligible = np.ones((len(qs), len(bs)), dtype=bool) if qg is None else np.asarray(qg)[:, None] == np.asarray(bg)[None, :]
    want = HC.nearest(HC.ratio_matrix(qd, ql, bd, bl), eligible, False, 0)
    got = _ratio(qs, bs, qg, bg, ld)
    assert np.array_equal(got[0], want[0]) and np.array_equal(got[1], want[1])
    return got


def _digit_strings(seed, lengths):
    rng = np.random.default_rng(seed)
    return ["".join(map(str, rng.integers(0, 10, n))) for n in lengths]


EDGE_LENGTHS = [1, 63, 64, 65, 127, 128]


def test_ratio_random_strings_of_every_length():
    rng = np.random.default_rng(20)
    qs = _digit_strings(21, EDGE_LENGTHS + list(rng.integers(1, 129, 10)))
    bs = _digit_strings(22, EDGE_LENGTHS + list(rng.integers(1, 129, 294)))
    assert len(qs) == 16 and len(bs) == 300
    ratio, idx = _check_ratio(qs, bs)
    assert bool((idx >= 0).all())
    again = _ratio(qs, bs)
    assert np.array_equal(again[0], ratio) and np.array_equal(again[1], idx)
    # a row width that is no multiple of 4 (the byte path), and one that is, below 128
    for ld in (101, 100):
        rng = np.random.default_rng(30 + ld)
        _check_ratio(_digit_strings(31, [1, 63, 64, 65, ld] + list(rng.integers(1, ld + 1, 11))),
                     _digit_strings(32, [1, 63, 64, 65, ld] + list(rng.integers(1, ld + 1, 295))), ld=ld)
    # short alphabets: long common subsequences, many equal ratios
    rng = np.random.default_rng(23)
    two = lambda n: "".join(map(str, rng.integers(3, 5, n)))
    _check_ratio([two(n) for n in EDGE_LENGTHS + [78] * 10], [two(n) for n in EDGE_LENGTHS + list(rng.integers(60, 129, 294))])


def test_ratio_identical_strings_and_ties():
    qs = _digit_strings(24, [78, 77, 128, 1, 64, 65] + [70] * 10)
    bs = _digit_strings(25, [76] * 300)
    for i, j in enumerate([290, 7, 150, 33, 64, 299]):
        bs[j] = qs[i]
    bs[295] = qs[0]                                             # a later copy of row 290, and of row 7 at 8
    bs[8] = qs[1]
    ratio, idx = _check_ratio(qs, bs)
    assert ratio[:6].tolist() == [100] * 6 and idx[:6].tolist() == [290, 7, 150, 33, 64, 299]
    # equal base rows throughout: every query's winner is the first of them
    ratio, idx = _check_ratio(qs, [bs[0]] * 40)
    assert idx.tolist() == [0] * 16


def test_ratio_half_cases_round_to_even():
    ratio, idx = _check_ratio(["1" + "0" * 7, "111" + "0" * 5], ["1" + "2" * 7, "111" + "2" * 5])
    # 200 * 1 / 16 = 12.5 -> 12 and 200 * 3 / 16 = 37.5 -> 38; the second query's best is 37.5 against row 1
    assert ratio.tolist() == [12, 38] and idx.tolist() == [0, 1]
    ratio, _ = _check_ratio(["1" + "0" * 7], ["1" + "2" * 7], ld=8)
    assert ratio.tolist() == [12]
    ratio, _ = _check_ratio(["111" + "0" * 5], ["111" + "2" * 5], ld=9)
    assert ratio.tolist() == [38]


def test_ratio_disjoint_alphabets_have_no_winner():
    ratio, idx = _check_ratio(["1111", "5", "13" * 64], ["222", "0", "2" * 128, "04" * 39])
    assert ratio.tolist() == [0, 0, 0] and idx.tolist() == [-1, -1, -1]


def test_ratio_groups():
    qs = _digit_strings(26, [78] * 16)
    bs = _digit_strings(27, list(np.random.default_rng(28).integers(70, 79, 300)))
    sizes = [3, 120, 0, 177]                                    # group 2 has no base row
    bg = np.repeat(np.arange(4), sizes).astype(np.int32)
    bg = bg[np.random.default_rng(29).permutation(300)]
    qg = (np.arange(16) % 4).astype(np.int32)
    ratio, idx = _check_ratio(qs, bs, qg, bg)
    assert bool((idx[qg == 2] == -1).all()) and bool((ratio[qg == 2] == 0).all()) and bool((idx[qg != 2] >= 0).all())
    for g in (0, 1, 3):
        rows = np.flatnonzero(bg == g)
        r, i = _ratio([qs[k] for k in np.flatnonzero(qg == g)], [bs[k] for k in rows])
        assert np.array_equal(r, ratio[qg == g]) and np.array_equal(rows[i], idx[qg == g])


# ---- end to end -------------------------------------------------------------------------------------------------------------------
def test_synthetic_sets_end_to_end():
    N = _N()
    d = N.synthetic_sets(0)
    train, evalf = d["train"].to(DEV), d["eval"].to(DEV)
    th, eh = N.average_hash(train), N.average_hash(evalf)
    want_t, want_e = HC.ahash(d["train"].numpy())[0], HC.ahash(d["eval"].numpy())[0]
    assert np.array_equal(th.cpu().numpy(), want_t) and np.array_equal(eh.cpu().numpy(), want_e)
    dist, didx = (t.cpu().numpy() for t in N.nearest_hamming(eh, th))
    ratio, ridx = (t.cpu().numpy() for t in N.nearest_digit_ratio(eh, th))
    every = np.ones((len(want_e), len(want_t)), dtype=bool)
    want = HC.nearest(HC.hamming_matrix(want_e, want_t), every, True, HC.NO_MATCH)
    assert np.array_equal(dist, want[0]) and np.array_equal(didx, want[1])
    (qd, ql), (bd, bl) = N.hash_digits(want_e), N.hash_digits(want_t)
    want = HC.nearest(HC.ratio_matrix(qd, ql, bd, bl), every, False, 0)
    assert np.array_equal(ratio, want[0]) and np.array_equal(ridx, want[1])
    planted = {e: t for e, t, _ in d["planted"]}
    assert len(planted) == 8
    for e, t in planted.items():
        assert (int(dist[e]), int(didx[e]), int(ratio[e]), int(ridx[e])) == (0, t, 100, t)
    others = [e for e in range(len(want_e)) if e not in planted]
    assert len(others) == 8 and min(int(dist[e]) for e in others) >= 86 and max(int(ratio[e]) for e in others) <= 51
    # the bookkeeping around the grouped searches
    res = N.hash_duplicates(evalf, d["eval_labels"], train, d["train_labels"], d["eval_names"], d["train_names"])
    assert res["n_exact_duplicates"] == 8 == res["n_category_duplicates"]
    by_eval = {r["eval_frame"]: r for r in res["indirect_duplicates"]}
    by_eval_h = {r["eval_frame"]: r for r in res["hamming_duplicates"]}
    for e, t in planted.items():
        assert by_eval[d["eval_names"][e]] == {"eval_frame": d["eval_names"][e], "train_frame": d["train_names"][t], "distance": 100}
        assert by_eval_h[d["eval_names"][e]] == {"eval_frame": d["eval_names"][e], "train_frame": d["train_names"][t], "distance": 0}
    assert all(by_eval[d["eval_names"][e]]["distance"] <= 51 and by_eval_h[d["eval_names"][e]]["distance"] >= 86 for e in others)


def test_cli_hash_space(tmp_path):
    N = _N()
    out = tmp_path / "dup"
    r = subprocess.run([sys.executable, os.path.join(ROOT, "nearest_neighbors.py"), "--dataset", "synthetic", "--space", "hash",
                        "--out_dir", str(out)], cwd=tmp_path, capture_output=True, text=True, timeout=600)
    assert r.returncode == 0, r.stdout[-3000:] + r.stderr[-3000:]
    assert "total number of duplicates (using perceptual hash): 8" in r.stdout and "Total number of duplicates: 8" in r.stdout
    d = N.synthetic_sets(0)
    hashed_eval, hashed_train = json.load(open(out / "hashed_eval_frames.json")), json.load(open(out / "hashed_train_frames.json"))
    assert len(set(hashed_eval) & set(hashed_train)) == 8
    assert set(hashed_eval.values()) == set(d["eval_names"]) and set(hashed_train.values()) == set(d["train_names"])
    want = {str(v): n for v, n in zip(HC.ints_of_words(HC.ahash(d["eval"].numpy())[0]), d["eval_names"])}
    assert hashed_eval == want
    indirect, hamming = json.load(open(out / "indirect_duplicates.json")), json.load(open(out / "hash_duplicates.json"))
    assert len(indirect) == len(hamming) == len(d["eval_names"])
    assert all(set(rec) == {"eval_frame", "train_frame", "distance"} for rec in indirect + hamming)
    assert sum(rec["distance"] == 100 for rec in indirect) == 8 == sum(rec["distance"] == 0 for rec in hamming)
    assert sorted(os.listdir(out)) == ["hash_duplicates.json", "hashed_eval_frames.json", "hashed_train_frames.json",
                                       "indirect_duplicates.json"]
