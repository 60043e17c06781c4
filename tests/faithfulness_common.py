"""The yardstick of the map-faithfulness tests: a numpy / float64 restatement of what csrc/faithfulness.hip computes, written from the
definitions in include/cvcl_hip.h "Map faithfulness" and never calling the library.

  ranks     np.argsort(-m, kind="stable") inverted (the comparison is the float one: -0.0 == +0.0, subnormals by value)
  perturb   np.where on rank < count
  blur      float64 separable convolution over a reflect-padded copy (np.pad mode "reflect": the edge is not repeated), the x axis
            first, with the library's weights (float64 exp / sum, rounded once to fp32)
  pair dot  float64 dot;  auc: float64 trapezoid

Bounds (eps = 2^-24, the unit round-off of fp32):
  blur      4 (k + 2) eps max|x|: each pass is a k-term fp32 sum of products with weights that sum to 1 (about (k + 1) eps max|x|
            in the worst case), two passes, doubled for the weights' own rounding to fp32
  pair dot  (E + 2) eps ||a|| ||b||: the classic bound of an E-term fp32 dot in any order
  auc       (S + 4) eps max|y| against float64 of the device's own fp32 scores: S terms whose widths sum to 1"""
import numpy as np

EPS = 2.0 ** -24


def ranks(maps):
    """maps [M, ...] -> int32 ranks of the same shape, per map over the flattened pixels"""
    m = np.asarray(maps, dtype=np.float32)
    flat = m.reshape(m.shape[0], -1)
    out = np.empty(flat.shape, dtype=np.int32)
    for i, row in enumerate(flat):
        order = np.argsort(-row.astype(np.float64), kind="stable")          # (float64 holds every fp32, subnormals included, exactly)
        out[i, order] = np.arange(row.size, dtype=np.int32)
    return out.reshape(m.shape)


def perturb(images, baseline, rk, image_of_map, item_map, item_count, item_mode):
    """-> [n_items, C, H, W] with the inputs' bits (baseline None: zeros)"""
    images = np.asarray(images, dtype=np.float32)
    N, C, H, W = images.shape
    base = np.zeros_like(images) if baseline is None else np.asarray(baseline, dtype=np.float32)
    rk = np.asarray(rk).reshape(-1, H, W)
    out = np.empty((len(item_map), C, H, W), dtype=np.float32)
    for i, (m, k, mode) in enumerate(zip(item_map, item_count, item_mode)):
        n = m if image_of_map is None else image_of_map[m]
        top = (rk[m] < k)[None]
        out[i] = np.where(top, base[n], images[n]) if mode == 0 else np.where(top, images[n], base[n])
    return out


def gaussian_weights(k, sigma):
    i = np.arange(k, dtype=np.float64) - k // 2
    w = np.exp(-(i * i) / (2.0 * sigma * sigma))
    return (w / w.sum()).astype(np.float32)


def blur(x, k, sigma):
    """x [..., H, W] -> float64"""
    w = gaussian_weights(k, sigma).astype(np.float64)
    r = k // 2
    x = np.asarray(x, dtype=np.float64)
    H, W = x.shape[-2:]
    lead = [(0, 0)] * (x.ndim - 2)
    px = np.pad(x, lead + [(0, 0), (r, r)], mode="reflect")
    y = sum(w[t] * px[..., :, t:t + W] for t in range(k))
    py = np.pad(y, lead + [(r, r), (0, 0)], mode="reflect")
    return sum(w[t] * py[..., t:t + H, :] for t in range(k))


def blur_bound(k, x):
    return 4.0 * (k + 2) * EPS * float(np.abs(x).max())


def pair_dot(rows, targets, target_of_row):
    a, b = np.asarray(rows, dtype=np.float64), np.asarray(targets, dtype=np.float64)[np.asarray(target_of_row)]
    return (a * b).sum(axis=1)


def pair_dot_bound(rows, targets, target_of_row):
    a, b = np.asarray(rows, dtype=np.float64), np.asarray(targets, dtype=np.float64)[np.asarray(target_of_row)]
    return (a.shape[1] + 2) * EPS * np.linalg.norm(a, axis=1) * np.linalg.norm(b, axis=1)


def auc(y, x):
    """y [K, S + 1, M], x [S + 1] -> float64 [K, M]"""
    y, x = np.asarray(y, dtype=np.float64), np.asarray(x, dtype=np.float64)
    return ((x[1:] - x[:-1])[None, :, None] * (y[:, :-1] + y[:, 1:]) / 2.0).sum(axis=1)


def auc_bound(y):
    y = np.asarray(y)
    return (y.shape[1] - 1 + 4) * EPS * float(np.abs(y).max())


def step_counts(HW, steps):
    return [s * HW // steps for s in range(steps + 1)]


# ---- map contents of the rank tests --------------------------------------------------------------------------------------------------
CONTENTS = ("equal", "relu", "ints", "gauss")


def make_maps(content, M, H, W, seed=0):
    rng = np.random.default_rng([seed, M, H, W, CONTENTS.index(content)])
    n = M * H * W
    if content == "equal":
        m = np.full(n, 0.37, dtype=np.float32)
    elif content == "relu":                               # at least 60 % exact zeros
        m = np.maximum(rng.standard_normal(n) - 0.4, 0.0).astype(np.float32)
        m[rng.random(n) < 0.45] = 0.0
    elif content == "ints":                               # integers from a range of 5: long runs of ties
        m = rng.integers(-2, 3, n).astype(np.float32)
    else:                                                 # Gaussian with negatives, both zeros and subnormals of both signs
        m = rng.standard_normal(n).astype(np.float32)
        special = np.array([0.0, -0.0, 1e-40, -1e-40, 1.4e-45, -1.4e-45, 5e-39], dtype=np.float32)
        pick = rng.random(n) < 0.3
        m[pick] = special[rng.integers(0, len(special), int(pick.sum()))]
    return m.reshape(M, H, W)
