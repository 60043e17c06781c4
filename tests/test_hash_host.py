"""CPU: the integer oracle of the perceptual hash (tests/hash_common.py) against what it must reduce to -- Pillow's grey, the identity
at 16 x 16, the mean of two pixels per axis at 224 x 224, a pure-Python LCS -- and the host side of multimodal/neighbors.py: the hash
<-> int <-> decimal string conversions, the bookkeeping of ``hash_duplicates`` on hand-made inputs (duplicates.py:81-105, :316-349),
the parser, and the refusal of CPU tensors."""
import json

import numpy as np
import pytest
import torch

import hash_common as HC
from multimodal import neighbors as N


def test_oracle_grey_is_pillow_convert_l():
    from PIL import Image
    x = HC.random_frames(0, 6, 37, 50)
    pil = np.stack([np.asarray(Image.fromarray(np.ascontiguousarray(f.transpose(1, 2, 0))).convert("L")) for f in x])
    assert np.array_equal(pil.astype(np.int64), HC.grey(x))
    edge = np.array([[0, 0, 0], [255, 255, 255], [255, 0, 0], [0, 255, 0], [0, 0, 255]], dtype=np.uint8).T.reshape(1, 3, 1, 5)
    assert HC.grey(edge).ravel().tolist() == [0, 255, 76, 150, 29]


def test_oracle_cells_at_16_are_the_grey_values():
    x = HC.random_frames(1, 3, 16, 16)
    assert np.array_equal(HC.cells(x), HC.grey(x))
    i0, i1, w0, w1 = HC.taps(16)
    assert i0.tolist() == list(range(16)) and w1.tolist() == [0] * 16 and i1[-1] == 15


def test_oracle_cells_at_224_are_the_rounded_mean_of_two_pixels_per_axis():
    x = HC.random_frames(2, 2, 224, 224)
    g = HC.grey(x)
    a, b = 14 * np.arange(16) + 6, 14 * np.arange(16) + 7
    four = g[:, a][:, :, a] + g[:, a][:, :, b] + g[:, b][:, :, a] + g[:, b][:, :, b]
    assert np.array_equal(HC.cells(x), (four + 2) >> 2)              # round half up of the mean of the four


def test_oracle_bits_words_and_ratio():
    f, v = HC.tie_frame()
    words, r = HC.ahash(f)
    assert int(r.sum()) == 256 * 15 and sorted(r[0].tolist()) == sorted(v.tolist())
    bits = HC.bits_of_words(words)[0]
    assert np.array_equal(bits, r[0] >= 15) and int(bits.sum()) == 112 + 32
    assert np.array_equal(HC.words_of_bits(HC.bits_of_words(words)), words)

    def lcs(a, b):
        prev = [0] * (len(b) + 1)
        for ca in a:
            cur = [0]
            for j, cb in enumerate(b):
                cur.append(prev[j] + 1 if ca == cb else max(prev[j + 1], cur[j]))
            prev = cur
        return prev[-1]

    rng = np.random.default_rng(3)
    strings = ["".join(map(str, rng.integers(0, 10, n))) for n in (1, 2, 5, 40, 63, 64, 65, 78, 127, 128)]
    d, l = HC.digit_rows(strings)
    for i, s in enumerate(strings):
        assert HC.lcs_to_all(d[i, :l[i]], d, l).tolist() == [lcs(s, t) for t in strings]
    # Python's round is round-half-to-even: the ratio in integers equals int(round(100 * 2 * LCS / (la + lb)))
    for la, lb, k in [(8, 8, 1), (8, 8, 3), (8, 8, 8), (3, 5, 1), (78, 77, 40), (1, 1, 0), (128, 128, 37)]:
        assert int(HC.half_even_ratio(k, la, np.int64(lb))) == int(round(100 * 2 * k / (la + lb)))
    assert int(HC.half_even_ratio(1, 8, np.int64(8))) == 12 and int(HC.half_even_ratio(3, 8, np.int64(8))) == 38


def test_hash_ints_and_digits_round_trip():
    words = np.zeros((5, 4), dtype=np.int64)
    words[1] = [1, 0, 0, 0]
    words[2] = [0, 0, 0, np.iinfo(np.int64).min]                      # bit 255 alone: a negative int64 word
    words[3] = [-1, -1, -1, -1]                                       # all 256 bits
    words[4] = HC.random_hashes(4, 1)[0]
    ints = N.hash_ints(torch.from_numpy(words))
    assert ints[:4] == [0, 1, 1 << 255, (1 << 256) - 1] and ints == HC.ints_of_words(words) == N.hash_ints(words)
    assert all(v >= 0 for v in ints)
    digits, lens = N.hash_digits(words)
    assert digits.dtype == np.uint8 and digits.shape == (5, 128) and lens.dtype == np.int32
    assert lens.tolist() == [len(str(v)) for v in ints] and lens[0] == 1 and digits[0, 0] == 0 and lens[3] == 78
    for i, v in enumerate(ints):
        assert "".join(map(str, digits[i, :lens[i]])) == str(v) and not digits[i, lens[i]:].any()
        assert int("".join(map(str, digits[i, :lens[i]]))) == v
    # the words come back from the int
    back = np.array([[(v >> (64 * k)) & (2**64 - 1) for k in range(4)] for v in ints], dtype=np.uint64).view(np.int64)
    assert np.array_equal(back, words)


def test_hash_duplicates_bookkeeping():
    h = HC.random_hashes(6, 7)
    # evaluation: two categories, given out of category order; e1 repeats e0's hash (the later name overwrites)
    eval_hashes = np.stack([h[0], h[0], h[1], h[2]])
    eval_labels, eval_names = ["cat", "cat", "ball", "ball"], ["e0", "e1", "e2", "e3"]
    # training: t0 = e0's hash in its category, t3 = e2's hash in ANOTHER category (exact, but not a category duplicate)
    train_hashes = np.stack([h[0], h[3], h[4], h[1], h[5]])
    train_labels, train_names = ["cat", "cat", "ball", "cat", "dog"], ["t0", "t1", "t2", "t3", "t4"]
    ratio = (np.array([100, 100, 41, 0]), np.array([0, 0, 2, -1]))
    dist = (np.array([0, 0, 120, 257]), np.array([0, 0, 2, -1]))
    res = N.hash_duplicates(None, eval_labels, None, train_labels, eval_names, train_names, hashes=(eval_hashes, train_hashes),
                            nearest_ratio=ratio, nearest_distance=dist)
    ints_e, ints_t = HC.ints_of_words(eval_hashes), HC.ints_of_words(train_hashes)
    assert res["hashed_eval_frames"] == {str(ints_e[0]): "e1", str(ints_e[2]): "e2", str(ints_e[3]): "e3"}
    assert res["hashed_train_frames"] == {str(v): n for v, n in zip(ints_t, train_names)}
    assert res["exact_duplicates"] == [str(v) for v in sorted({ints_e[0], ints_e[2]})] and res["n_exact_duplicates"] == 2
    assert res["n_category_duplicates"] == 1
    # categories in sorted order ("ball" first), frames in their given order; the reference's keys
    assert res["indirect_duplicates"] == [{"eval_frame": "e2", "train_frame": "t2", "distance": 41},
                                          {"eval_frame": "e3", "train_frame": "", "distance": 0},
                                          {"eval_frame": "e0", "train_frame": "t0", "distance": 100},
                                          {"eval_frame": "e1", "train_frame": "t0", "distance": 100}]
    assert res["hamming_duplicates"] == [{"eval_frame": "e2", "train_frame": "t2", "distance": 120},
                                         {"eval_frame": "e3", "train_frame": "", "distance": 257},
                                         {"eval_frame": "e0", "train_frame": "t0", "distance": 0},
                                         {"eval_frame": "e1", "train_frame": "t0", "distance": 0}]
    assert N.hash_summary(res) == ["total number of duplicates (using perceptual hash): 2", "Total number of duplicates: 1"]
    json.dumps(res)


def test_parser_accepts_the_hash_space():
    assert N.parser().parse_args(["--dataset", "synthetic", "--space", "hash"]).space == "hash"
    assert N.parser().parse_args([]).space == "both"
    with pytest.raises(SystemExit):
        N.parser().parse_args(["--space", "hashes"])


def test_python_layer_refuses_cpu_tensors():
    from multimodal._hip import CvclError
    with pytest.raises(CvclError):
        N.average_hash(torch.zeros(2, 3, 16, 16, dtype=torch.uint8))
    with pytest.raises(CvclError):
        N.nearest_hamming(torch.zeros(2, 4, dtype=torch.int64), torch.zeros(3, 4, dtype=torch.int64))
    with pytest.raises(CvclError):
        N.nearest_digit_ratio(torch.zeros(2, 4, dtype=torch.int64), torch.zeros(3, 4, dtype=torch.int64))
