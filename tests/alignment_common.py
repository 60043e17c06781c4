"""Float64 restatement of the reference's alignment arithmetic (analysis_cvcl/alignment.py:106-110, :142-161, :182-195, :230-232,
analysis_cvcl/embeddings.py:106-111, analysis_tools/representation_similarity.py) in numpy, shared by the alignment tests and by
tools/gen_golden_alignment.py (which checks it against the reference's own fp32 values to 5e-6 relative), plus the seeded inputs
and the error bounds the GPU tests hold the kernels to."""
import numpy as np

U = 2.0 ** -24                                           # fp32 unit roundoff


def class_means64(x, labels, n_classes):
    x = np.asarray(x, dtype=np.float64)
    labels = np.asarray(labels)
    return np.stack([x[labels == c].mean(axis=0) if np.any(labels == c) else np.zeros(x.shape[1]) for c in range(n_classes)])


def cosine64(a, b=None, eps=1e-8):
    a = np.asarray(a, dtype=np.float64)
    b = a if b is None else np.asarray(b, dtype=np.float64)
    na = np.maximum(np.linalg.norm(a, axis=1), eps)
    nb = np.maximum(np.linalg.norm(b, axis=1), eps)
    return (a @ b.T) / (na[:, None] * nb[None, :])


def dissim64(a):
    return (1.0 - cosine64(a)) / 2.0


def triu_items(A):
    A = np.asarray(A)
    return A[np.triu_indices(A.shape[0], k=1, m=A.shape[1])]


def pearson64(x, y):
    """(r, n, mean_x, mean_y, var_x, var_y) with population variances; r = NaN when a side is constant"""
    x, y = np.asarray(x, dtype=np.float64), np.asarray(y, dtype=np.float64)
    mx, my = x.mean(), y.mean()
    dx, dy = x - mx, y - my
    qx, qy = float(dx @ dx), float(dy @ dy)
    const = x.min() == x.max() or y.min() == y.max()
    r = float("nan") if const else float(np.clip((dx @ dy) / (np.sqrt(qx) * np.sqrt(qy)), -1.0, 1.0))
    return r, x.size, float(mx), float(my), qx / x.size, qy / x.size


def rsa64(A, B):
    return pearson64(triu_items(A), triu_items(B))[0]


def paired_l2_64(x, y, eps=1e-6):
    d = np.asarray(x, dtype=np.float64) - np.asarray(y, dtype=np.float64) + eps
    return np.sqrt((d * d).sum(axis=1))


def interleave(image_rows, text_rows):
    out = np.empty((2 * image_rows.shape[0], image_rows.shape[1]), dtype=image_rows.dtype)
    out[0::2], out[1::2] = image_rows, text_rows
    return out


# ---- bounds (the issue's) ---------------------------------------------------------------------------------------------------------------
def mean_bound(x, labels, n_classes):
    """16 * 2^-24 * mean_i |x_i| per element of each class"""
    return 16.0 * U * class_means64(np.abs(np.asarray(x, dtype=np.float64)), labels, n_classes)


def cosine_bound(D):
    return 2.0 * D * U


def pearson_bound(D, tri_a64, tri_b64):
    """4 * delta / sigma_min: first-order perturbation of r under entrywise errors delta = cosine_bound(D)"""
    sigma_min = min(float(np.std(tri_a64)), float(np.std(tri_b64)))
    return 4.0 * cosine_bound(D) / sigma_min, sigma_min


# ---- seeded inputs -----------------------------------------------------------------------------------------------------------------------
def golden_inputs():
    """features [157, 64], labels over 7 classes of unequal size (one singleton, rows shuffled), text features [7, 64]"""
    rng = np.random.default_rng(20240607)
    sizes = [1, 5, 12, 19, 27, 40, 53]
    assert sum(sizes) == 157
    labels = np.concatenate([np.full(n, c, dtype=np.int32) for c, n in enumerate(sizes)])
    proto = rng.standard_normal((7, 64))
    feats = (proto[labels] + 0.7 * rng.standard_normal((157, 64))).astype(np.float32)
    order = rng.permutation(157)
    text = (0.8 * proto + 0.6 * rng.standard_normal((7, 64))).astype(np.float32)
    return feats[order], labels[order], text


def prototype_case(seed, n_classes, D, sizes=None, noise=0.5):
    """class prototypes plus noise (so that the similarities spread: sigma of the triangles stays well above 0.05), rows shuffled:
    (features [N, D] fp32, labels [N] int32, text [C, D] fp32).  Prototypes share a common direction of random strength, which
    makes the pairwise cosines differ from pair to pair at any D."""
    rng = np.random.default_rng(seed)
    if sizes is None:
        sizes = [1 + int(v) for v in rng.integers(0, 37, n_classes)]
        sizes[0] = 1
    labels = np.concatenate([np.full(n, c, dtype=np.int32) for c, n in enumerate(sizes)])
    common = rng.standard_normal(D)
    proto = rng.standard_normal((n_classes, D)) + rng.uniform(-2.5, 2.5, (n_classes, 1)) * common[None, :]
    feats = (proto[labels] + noise * rng.standard_normal((len(labels), D))).astype(np.float32)
    order = rng.permutation(len(labels))
    text = (proto + noise * rng.standard_normal((n_classes, D))).astype(np.float32)
    return feats[order], labels[order], text
