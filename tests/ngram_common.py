"""Shared by the n-gram tests and tools/gen_golden_ngram.py: the seeded corpus generator, the case table, and a pure-Python / numpy
restatement of the reference's n-gram model (top-level ngram.py) in the form the device uses -- every (n + 1)-gram packed into one
non-negative int64, a sorted unique table per order, two lower-bound searches per back-off step, log and sum in float64.
tests/test_ngram_fixture.py pins this restatement to the reference's own results (tests/golden/ngram.npz), bit for bit; the GPU
tests may then use it on inputs that are not in the archive."""
import functools
import math

import numpy as np

# (N, vocab_size, B, L); the training corpus has seed N, the evaluation corpus seed 100 + N
CASES = ((1, 7, 6, 5), (3, 7, 12, 6), (4, 30, 40, 9), (5, 4096, 64, 12), (3, 2350, 64, 25))
ALPHAS = (0.1, 0.4)
UNSEEN_UNIGRAM_EXEMPT = ((1, 7, 6, 5), (3, 7, 12, 6))         # every word of these vocabularies occurs in training
SOS, EOS = 1, 2


def case_name(case):
    return "n{}_v{}_b{}_l{}".format(*case)


def corpus(seed, V, B, L):
    """-> (y [B, L] int64, y_len [B] int64): lengths uniform in [1, L]; <sos> = 1 first, <eos> = 2 last when the length is > 1,
    Zipf(1.5) word ids 3 + min(z - 1, V - 4) between them, zero padding."""
    rng = np.random.default_rng(seed)
    y_len = rng.integers(1, L + 1, B).astype(np.int64)
    words = 3 + np.minimum(rng.zipf(1.5, (B, L)) - 1, V - 4)
    y = np.zeros((B, L), dtype=np.int64)
    for b, n in enumerate(y_len):
        y[b, :n] = words[b, :n]
        y[b, 0] = SOS
        if n > 1:
            y[b, n - 1] = EOS
    return y, y_len


def case_data(case):
    N, V, B, L = case
    return corpus(N, V, B, L), corpus(100 + N, V, B, L)


def key_bits(V):
    return max(1, (V - 1).bit_length())


def pack(tokens, bits):
    key = 0
    for t in tokens:
        key = (key << bits) | int(t)
    return key


def count_tables(y, y_len, N, V, tables=None):
    """The reference's update (ngram.py:28-36) -> per order (keys, counts): the packed (context, word) grams, sorted, with
    their counts.  ``tables``: counts to add to (several updates)."""
    bits = key_bits(V)
    out = []
    for n in range(N):
        grams = [pack(s[i - n:i + 1], bits) for s in (row[:max(0, min(int(m), len(row)))].tolist() for row, m in zip(y, y_len))
                 for i in range(max(1, n), len(s))]
        keys, counts = np.unique(np.asarray(grams, dtype=np.int64), return_counts=True)
        if tables is not None:
            allk = np.concatenate([tables[n][0], keys])
            keys, inv = np.unique(allk, return_inverse=True)
            counts = _add_counts(inv, np.concatenate([tables[n][1], counts]), len(keys))
        out.append((keys.astype(np.int64), counts.astype(np.int64)))
    return out


def _add_counts(inv, counts, n):
    total = np.zeros(n, dtype=np.int64)
    np.add.at(total, inv, counts)
    return total


def context_tables(tables, V):
    """Per order (context keys, totals): a context's total is the sum over its run of the gram table."""
    bits = key_bits(V)
    out = []
    for keys, counts in tables:
        ctx, inv = np.unique(keys >> bits, return_inverse=True)
        out.append((ctx, _add_counts(inv, counts, len(ctx))))
    return out


def to_counts(tables, V):
    """The reference's ``_count`` structure: per order {context tuple: [total, {word: count}]}."""
    bits = key_bits(V)
    mask = (1 << bits) - 1
    out = []
    for n, (keys, counts) in enumerate(tables):
        table = {}
        for key, c in zip(keys.tolist(), counts.tolist()):
            entry = table.setdefault(tuple((key >> (bits * (n - j))) & mask for j in range(n)), [0, {}])
            entry[0] += c
            entry[1][key & mask] = c
        out.append(table)
    return out


def _find(keys, key):
    j = int(np.searchsorted(keys, key, side="left"))
    return j if j < len(keys) and keys[j] == key else -1


_log = functools.lru_cache(maxsize=None)(math.log)


class Model:
    """The tables of a counted corpus with the device's lookups."""

    def __init__(self, N, V, tables):
        self.N, self.V, self.bits = N, V, key_bits(V)
        self.grams, self.ctxs = tables, context_tables(tables, V)

    def logprob(self, s, i, w, log_alpha, log_1m_alpha):
        """ngram.py:58-69 for position i of the utterance s and the candidate word w -> (log-probability, branch): the branch is
        ("order", n) where order n >= 1 had seen the word, "unigram_seen" or "unigram_unseen"."""
        lp = 0.0
        for n in range(min(self.N - 1, i), -1, -1):
            ctx = pack(s[i - n:i], self.bits)
            c = _find(self.ctxs[n][0], ctx)
            if c >= 0:
                g = _find(self.grams[n][0], (ctx << self.bits) | int(w))
                if n == 0:
                    seen = int(self.grams[0][1][g]) if g >= 0 else 0
                    lp += _log(seen + 1) - _log(int(self.ctxs[0][1][c]) + self.V)
                    return lp, ("unigram_seen" if seen else "unigram_unseen")
                if g >= 0:
                    lp += _log(int(self.grams[n][1][g])) - _log(int(self.ctxs[n][1][c])) + log_1m_alpha
                    return lp, ("order", n)
            lp += log_alpha
        raise Exception("Even unigram is not applicable.")

    def ce_loss(self, y, y_len, alpha):
        """calculate_ce_loss(tokenwise=True) -> (loss [B, L - 1] float32: the float64 value stored into a float32 array, as the
        reference's assignment into a float tensor rounds it; loss64, the same before rounding; the branch histogram)."""
        la, l1a = math.log(alpha), math.log(1 - alpha)
        B, L = y.shape
        loss64 = np.zeros((B, max(L - 1, 0)), dtype=np.float64)
        hist = {}
        for b in range(B):
            s = y[b, :max(0, min(int(y_len[b]), L))].tolist()
            for i in range(1, len(s)):
                lp, branch = self.logprob(s, i, s[i], la, l1a)
                loss64[b, i - 1] = -lp
                hist[branch] = hist.get(branch, 0) + 1
        return loss64.astype(np.float32), loss64, hist

    def probs(self, y, y_len, alpha):
        """exp(logprob) for every candidate word -> [B, L - 1, V] float64, zero rows outside the utterances.  Per position the
        candidates are walked order by order together: the words order n has seen after the context stop there."""
        la, l1a = math.log(alpha), math.log(1 - alpha)
        B, L = y.shape
        out = np.zeros((B, max(L - 1, 0), self.V), dtype=np.float64)
        for b in range(B):
            s = y[b, :max(0, min(int(y_len[b]), L))].tolist()
            for i in range(1, len(s)):
                lp = np.zeros(self.V, dtype=np.float64)
                open_ = np.ones(self.V, dtype=bool)
                base = 0.0                                   # the log_alpha terms so far: the same sum for every open word
                for n in range(min(self.N - 1, i), 0, -1):
                    ctx = pack(s[i - n:i], self.bits)
                    c = _find(self.ctxs[n][0], ctx)
                    if c >= 0:
                        keys, counts = self.grams[n]
                        lo, hi = np.searchsorted(keys, [ctx << self.bits, (ctx + 1) << self.bits])
                        for key, cnt in zip(keys[lo:hi].tolist(), counts[lo:hi].tolist()):
                            w = key & ((1 << self.bits) - 1)
                            if open_[w]:
                                lp[w] = base + (_log(cnt) - _log(int(self.ctxs[n][1][c])) + l1a)
                                open_[w] = False
                    base += la
                total = int(self.ctxs[0][1][0])
                seen = dict(zip(self.grams[0][0].tolist(), self.grams[0][1].tolist()))
                for w in np.flatnonzero(open_).tolist():
                    lp[w] = base + (_log(seen.get(w, 0) + 1) - _log(total + self.V))
                out[b, i - 1] = [math.exp(v) for v in lp.tolist()]
        return out


def n_tokens(y_len, L):
    return int(np.maximum(np.minimum(y_len, L) - 1, 0).sum())


def branches_allowed(case):
    """Every branch a case's N and V allow: orders N - 1 .. 1 seen, the unigram seen, the unigram unseen."""
    want = [("order", n) for n in range(1, case[0])] + ["unigram_seen"]
    return want + ([] if case in UNSEEN_UNIGRAM_EXEMPT else ["unigram_unseen"])


def ulp_distance(a, b):
    """|a - b| in float32 steps, elementwise, for finite float32 arrays: the distance of their places on the ordered float line."""
    def place(x):
        i = np.ascontiguousarray(x, dtype=np.float32).view(np.int32).astype(np.int64)
        return np.where(i < 0, -(i & 0x7fffffff), i)
    return np.abs(place(a) - place(b))
