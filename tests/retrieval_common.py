"""The yardstick of the retrieval tests: ranks restated in float64 numpy, independent of the library.

A query's positives are the base rows of its key; s = the largest cosine among them, at the lowest such row t.  Its rank is the number
of negatives j with c_j > s, or c_j == s and j < t: the position of the best positive in a stable descending sort with the other
positives removed; -1 without a positive.

``exact_ranks``: for features drawn from {-1, +1} all norms are sqrt(D), the dots are exact integers in fp32 and float64 alike, and
equal dots give equal cosines in any arithmetic that scales them the same way, so the integer dots order the rows exactly, ties
included.  ``bracket``: for real-valued features an fp32 cosine differs from the float64 one; with delta the bound on that difference
every correct rank lies in #{neg: c64 > s64 + delta} <= rank <= #{neg: c64 >= s64 - delta}."""
import numpy as np


def sign_features(rng, n, d):
    return (rng.integers(0, 2, (n, d)) * 2 - 1).astype(np.float32)


def exact_ranks(q, b, qk, bk):
    """q [Nq, D], b [Nb, D] with entries +-1, integer keys -> (rank [Nq] int64, best row [Nq] int64; both -1 without a positive)"""
    dots = np.rint(q.astype(np.float64) @ b.astype(np.float64).T).astype(np.int64)      # |dot| <= D: exact in float64
    pos = qk[:, None] == bk[None, :]
    rows = np.arange(b.shape[0])[None, :]
    low = np.iinfo(np.int64).min
    s = np.where(pos, dots, low).max(axis=1)
    has = pos.any(axis=1)
    t = np.where(pos & (dots == s[:, None]), rows, b.shape[0]).min(axis=1)
    beats = ~pos & ((dots > s[:, None]) | ((dots == s[:, None]) & (rows < t[:, None])))
    return np.where(has, beats.sum(axis=1), -1).astype(np.int64), np.where(has, t, -1).astype(np.int64)


def cosines64(q, b, eps=1e-8):
    q64, b64 = q.astype(np.float64), b.astype(np.float64)
    qn = q64 / np.maximum(np.linalg.norm(q64, axis=1, keepdims=True), eps)
    bn = b64 / np.maximum(np.linalg.norm(b64, axis=1, keepdims=True), eps)
    return qn @ bn.T


def delta_of(d):
    """(D + 2) 2^-24: the fp32 summation bound for the dot of two unit vectors of D terms, plus the two roundings around it"""
    return (d + 2) * 2.0 ** -24


def bracket(q, b, qk, bk):
    """-> (lo [Nq], hi [Nq], has [Nq] bool): the bounds on the rank of every query with a positive"""
    c = cosines64(q, b)
    pos = qk[:, None] == bk[None, :]
    has = pos.any(axis=1)
    s = np.where(pos, c, -np.inf).max(axis=1)
    d = delta_of(q.shape[1])
    lo = (~pos & (c > (s + d)[:, None])).sum(axis=1)
    hi = (~pos & (c >= (s - d)[:, None])).sum(axis=1)
    return lo.astype(np.int64), hi.astype(np.int64), has


def check_bracket(rank, lo, hi, has):
    """every ranked query inside its bracket, tight brackets exactly, queries without a positive at -1 -> the number of loose ones"""
    rank = np.asarray(rank)
    assert np.array_equal(rank[~has], np.full(int((~has).sum()), -1))
    assert bool((lo[has] <= rank[has]).all()) and bool((rank[has] <= hi[has]).all()), \
        (np.nonzero(has & ((rank < lo) | (rank > hi)))[0][:10], rank[has][:10], lo[has][:10], hi[has][:10])
    tight = has & (lo == hi)
    assert np.array_equal(rank[tight], lo[tight])
    return int((has & (lo != hi)).sum())


def pair_keys(text_ids):
    """text ids [N] -> (key of each pair's text, numbered in order of first appearance [N]; first pair of each distinct text [T])"""
    seen, dense, first = {}, [], []
    for i, t in enumerate(int(x) for x in text_ids):
        if t not in seen:
            seen[t] = len(first)
            first.append(i)
        dense.append(seen[t])
    return np.array(dense, dtype=np.int64), np.array(first, dtype=np.int64)
