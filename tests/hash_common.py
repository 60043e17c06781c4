"""A numpy integer oracle of the perceptual-hash definitions (include/cvcl_hip.h "Perceptual-hash duplicates") and the case builders
the hash tests share.  Everything is int64 arithmetic: a comparison with the kernels is exact or wrong.

grey     g = (19595 R + 38470 G + 7471 B + 32768) >> 16                                   (ITU-R 601, Pillow's convert("L"))
taps     per axis of n pixels and cell d: num = (2 d + 1) n - 16, i0 = num // 32, w1 = num - 32 i0, w0 = 32 - w1, i1 = min(i0 + 1, n - 1)
cells    r = (sum over the 2 x 2 taps of wy wx g + 512) >> 10
bits     bit 16 y + x = 256 r >= sum of the 256 r; word w = bits 64 w .. 64 w + 63, as int64
Hamming  the differing bits of two hashes
LCS      the plain dynamic programme, vectorised over the base strings
ratio    round_half_even(200 LCS / (la + lb)) by quotient and remainder"""
import numpy as np

SIDE, WORDS, DIGITS_MAX, NO_MATCH = 16, 4, 128, 257


def grey(rgb):
    """uint8 [N, 3, H, W] -> int64 [N, H, W]"""
    r, g, b = (rgb[:, c].astype(np.int64) for c in range(3))
    return (19595 * r + 38470 * g + 7471 * b + 32768) >> 16


def taps(n):
    """-> (i0, i1, w0, w1), each int64 [16]"""
    num = (2 * np.arange(SIDE, dtype=np.int64) + 1) * n - SIDE
    i0 = num // (2 * SIDE)
    w1 = num - 2 * SIDE * i0
    return i0, np.minimum(i0 + 1, n - 1), 2 * SIDE - w1, w1


def cells(rgb):
    """uint8 [N, 3, H, W] -> int64 [N, 16, 16], the rounded cell values (grey is evaluated at the taps only)"""
    y0, y1, wy0, wy1 = taps(rgb.shape[2])
    x0, x1, wx0, wx1 = taps(rgb.shape[3])

    def g(ys, xs):
        return grey(rgb[:, :, ys][:, :, :, xs])

    v = wy0[:, None] * (wx0 * g(y0, x0) + wx1 * g(y0, x1)) + wy1[:, None] * (wx0 * g(y1, x0) + wx1 * g(y1, x1))
    return (v + 512) >> 10


def bits_of_cells(r):
    """int64 [N, 16, 16] -> bool [N, 256]"""
    flat = r.reshape(r.shape[0], SIDE * SIDE)
    return 256 * flat >= flat.sum(axis=1, keepdims=True)


def words_of_bits(bits):
    """bool [N, 256] -> int64 [N, 4]"""
    w = np.zeros((bits.shape[0], WORDS), dtype=np.uint64)
    for i in range(SIDE * SIDE):
        w[:, i // 64] |= bits[:, i].astype(np.uint64) << np.uint64(i % 64)
    return w.view(np.int64)


def ahash(rgb):
    """uint8 [N, 3, H, W] -> (int64 [N, 4] words, int64 [N, 256] cells)"""
    r = cells(rgb)
    return words_of_bits(bits_of_cells(r)), r.reshape(r.shape[0], -1)


def bits_of_words(words):
    """int64 [N, 4] -> bool [N, 256]"""
    u = np.ascontiguousarray(words).view(np.uint64)
    return np.stack([(u[:, i // 64] >> np.uint64(i % 64)) & np.uint64(1) for i in range(SIDE * SIDE)], axis=1).astype(bool)


def ints_of_words(words):
    u = np.ascontiguousarray(words).view(np.uint64)
    return [sum(int(x) << (64 * k) for k, x in enumerate(row)) for row in u]


_POPCOUNT8 = np.array([bin(i).count("1") for i in range(256)], dtype=np.int64)


def hamming_matrix(q, b):
    """int64 [Nq, 4], [Nb, 4] -> int64 [Nq, Nb]: the set bits of the xor, byte by byte through a table"""
    q8, b8 = np.ascontiguousarray(q).view(np.uint8), np.ascontiguousarray(b).view(np.uint8)
    return np.stack([_POPCOUNT8[b8 ^ row[None, :]].sum(axis=1) for row in q8])


def nearest(values, eligible, lower, none):
    """the first arg-min (``lower``) or arg-max of every row of ``values`` [Nq, Nb] over its ``eligible`` entries -> (value, index);
    (none, -1) for a row without one, and for a maximum that does not exceed ``none`` (the reference's scan with a strict >)"""
    big = np.iinfo(np.int64).max
    v = np.where(eligible, values, big if lower else -big)
    idx = v.argmin(axis=1) if lower else v.argmax(axis=1)
    val = v[np.arange(v.shape[0]), idx]
    has = eligible.any(axis=1) & (np.ones_like(val, dtype=bool) if lower else val > none)
    return np.where(has, val, none), np.where(has, idx, -1)


def lcs_to_all(a, base, base_len):
    """LCS(a, base[j, :base_len[j]]) for all j by the plain dynamic programme L[i][k] = max(L[i-1][k], L[i][k-1], L[i-1][k-1] +
    match), one row per digit of ``a``; the dependence on L[i][k-1] is a running maximum along the row.  Column k depends on
    columns <= k only, so the padding behind a base string's length is never read."""
    nb, ld = base.shape
    row = np.zeros((nb, ld + 1), dtype=np.int64)
    for ca in a:
        row[:, 1:] = np.maximum.accumulate(np.maximum(row[:, 1:], row[:, :-1] + (base == ca)), axis=1)
    return row[np.arange(nb), base_len]


def half_even_ratio(lcs, la, lb):
    num, den = 200 * np.asarray(lcs, dtype=np.int64), np.asarray(la + lb, dtype=np.int64)
    q, r = num // den, num % den
    return q + ((2 * r > den) | ((2 * r == den) & (q % 2 == 1)))


def ratio_matrix(q, q_len, base, base_len):
    """uint8 digit rows and int lengths -> int64 [Nq, Nb]"""
    return np.stack([half_even_ratio(lcs_to_all(q[i, :q_len[i]], base, base_len), int(q_len[i]), base_len.astype(np.int64))
                     for i in range(q.shape[0])])


def digit_rows(strings, ld=DIGITS_MAX):
    """decimal strings -> (uint8 [N, ld] digit values, int32 [N] lengths)"""
    d = np.zeros((len(strings), ld), dtype=np.uint8)
    for i, s in enumerate(strings):
        d[i, :len(s)] = [int(c) for c in s]
    return d, np.array([len(s) for s in strings], dtype=np.int32)


# ---- case builders ---------------------------------------------------------------------------------------------------------------
def random_frames(seed, n, h, w):
    return np.random.default_rng(seed).integers(0, 256, (n, 3, h, w), dtype=np.uint8)


def frame_of_cells(values):
    """a 16 x 16 grey frame (R = G = B, so grey is the value itself) whose cells are ``values`` [256]"""
    v = np.asarray(values, dtype=np.uint8).reshape(1, 1, SIDE, SIDE)
    return np.repeat(v, 3, axis=1)


def tie_frame():
    """112 cells at 10, 112 at 20 and 32 at 15: the mean is exactly 15 and the 32 tie cells must be set"""
    v = np.array([10] * 112 + [20] * 112 + [15] * 32)
    return frame_of_cells(np.random.default_rng(5).permutation(v)), v


def random_hashes(seed, n):
    return np.random.default_rng(seed).integers(-2**63, 2**63, (n, WORDS), dtype=np.int64)


def flip_bits(row, positions):
    u = row.copy().view(np.uint64)
    for p in positions:
        u[p // 64] ^= np.uint64(1) << np.uint64(p % 64)
    return u.view(np.int64)
