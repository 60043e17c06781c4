"""The reference's image-text alignment analysis (analysis_cvcl/alignment.py, analysis_cvcl/embeddings.py:106-118 and the helpers of
analysis_tools/representation_similarity.py) on the HIP path.

The reference encodes frame by frame, averages per category in numpy and fills its cosine matrices with one F.normalize /
F.cosine_similarity pair per entry.  Here the frames go through ``neighbors.extract_features`` in batches, the category words
through one ``encode_text`` call, and the rest is a handful of launches of csrc/alignment.hip: ``class_means`` (cvcl_class_mean_f32),
``cosine_matrix`` (cvcl_cosine_matrix_f32), ``rsa_of_dissim_matrices`` (cvcl_triu_pearson_f32) and ``paired_distances``
(cvcl_paired_l2_f32).  Inputs are contiguous fp32 device tensors; a CPU tensor raises, nothing falls back to torch arithmetic.
Frames are encoded at the size they are stored in; with ``--resize`` they go through ``preprocess.DevicePreprocess`` first, the
reference's Resize((224, 224), BICUBIC) -> ToTensor -> Normalize on the device, and may then be of any and mixed sizes."""
from __future__ import annotations

import csv
import json
import os

import numpy as np
import torch

from . import _hip as H
from . import neighbors as NB

COSINE_EPS = 1e-8                                    # F.cosine_similarity's default
PAIRWISE_EPS = 1e-6                                  # F.pairwise_distance's default
MAX_D, MAX_C, MAX_ROWS, MAX_N = 2048, 4096, 4096, 1 << 24
KITTY = {"cat": "kitty"}                             # alignment.py:119: eval_categories[3] = "kitty"
SYNTHETIC_WORDS = ("apple", "baby", "ball", "book", "car", "cat", "chair", "dog")     # all in vocab.json, in sorted order


def _rows(t, what):
    if torch.is_tensor(t) and (t.dim() != 2 or t.dtype != torch.float32):
        raise H.CvclError(f"{what}: expected [N, D] fp32 rows, got {tuple(t.shape)} {t.dtype}")
    if not torch.is_tensor(t) or not t.is_cuda:
        raise H.CvclError(f"{what}: the alignment analysis needs device tensors (got {type(t).__name__}"
                          f"{'' if not torch.is_tensor(t) else ' on ' + str(t.device)}); there is no CPU fallback")
    if t.shape[0] < 1 or t.shape[1] < 1:
        raise H.CvclError(f"{what}: empty operand {tuple(t.shape)}")
    return t.contiguous()


def _labels(label_ids, n, n_classes, device):
    """int32 device labels; the range check runs on the host copy when the ids come from the host (no synchronisation)"""
    if torch.is_tensor(label_ids) and label_ids.is_cuda:
        lo, hi = int(label_ids.min()), int(label_ids.max())
        lab = label_ids.to(torch.int32).contiguous()
    else:
        host = np.asarray(label_ids.cpu() if torch.is_tensor(label_ids) else label_ids)
        if host.dtype.kind not in "iu":
            raise ValueError(f"label ids must be integers, got {host.dtype}")
        lo, hi = (int(host.min()), int(host.max())) if host.size else (0, 0)
        lab = torch.from_numpy(host.astype(np.int32)).to(device)
    if tuple(lab.shape) != (n,):
        raise ValueError(f"label ids must be [{n}], got {tuple(lab.shape)}")
    if lo < 0 or hi >= n_classes:
        raise ValueError(f"label ids span {lo}..{hi}, outside [0, {n_classes})")
    return lab


def _class_means(features, label_ids, n_classes):
    x = _rows(features, "class_means(features)")
    N, D = x.shape
    n_classes = int(n_classes)
    if not (1 <= n_classes <= MAX_C) or D > MAX_D or N >= MAX_N:
        raise H.CvclError(f"class_means: N {N}, D {D}, C {n_classes} outside N < 2^24, D <= {MAX_D}, 1 <= C <= {MAX_C}")
    lab = _labels(label_ids, N, n_classes, x.device)
    lib = H.lib()
    means = torch.empty(n_classes, D, dtype=torch.float32, device=x.device)
    counts = torch.empty(n_classes, dtype=torch.int32, device=x.device)
    ws = torch.empty(lib.cvcl_class_mean_workspace_bytes(N, D, n_classes), dtype=torch.uint8, device=x.device)
    H.check(lib.cvcl_class_mean_f32(H.ptr(x), H.ptr(lab), N, D, n_classes, H.ptr(means), H.ptr(counts), H.ptr(ws), ws.numel(),
                                    H.stream_ptr()), "cvcl_class_mean_f32")
    return means, counts


def _refuse_empty(counts_host):
    empty = [int(i) for i in np.nonzero(np.asarray(counts_host) == 0)[0]]
    if empty:
        raise ValueError(f"classes without a member: {empty}")


def class_means(features, label_ids, n_classes):
    """np.mean(features[label == c], axis=0) for c in range(n_classes) (alignment.py:106-110): features [N, D] fp32 on the device,
    label_ids [N] integers in [0, n_classes) in any order -> (means [C, D] fp32, counts [C] int32), both on the device.  Sums in
    double, bit-identical from call to call.  A class without a member is a ValueError naming the ids (this check reads the
    counts back: one synchronisation)."""
    means, counts = _class_means(features, label_ids, n_classes)
    _refuse_empty(counts.cpu().numpy())
    return means, counts


def cosine_matrix(a, b=None, eps=COSINE_EPS):
    """[M, K] fp32 cosines of the rows of a [M, D] and b [K, D]; ``b=None``: of a with itself, the reference's
    cosine_matrix(A) (representation_similarity.py:5-12), exactly symmetric.  Entry (i, j) is also the value of
    F.cosine_similarity(F.normalize(a_i), F.normalize(b_j), dim=0) (alignment.py:148-161)."""
    a = _rows(a, "cosine_matrix(a)")
    b = a if b is None else _rows(b, "cosine_matrix(b)")
    (M, D), K = a.shape, b.shape[0]
    if b.shape[1] != D:
        raise H.CvclError(f"cosine_matrix: rows of a are {D} wide, rows of b {b.shape[1]}")
    if M > MAX_ROWS or K > MAX_ROWS or D > MAX_D:
        raise H.CvclError(f"cosine_matrix: M {M}, K {K}, D {D} outside M, K <= {MAX_ROWS}, D <= {MAX_D}")
    if b is not a and b.data_ptr() == a.data_ptr() and M != K:
        b = b.clone()                                    # (a prefix view of a: not the self-similarity case)
    out = torch.empty(M, K, dtype=torch.float32, device=a.device)
    H.check(H.lib().cvcl_cosine_matrix_f32(H.ptr(a), H.ptr(b), M, K, D, float(eps), H.ptr(out), H.stream_ptr()), "cvcl_cosine_matrix_f32")
    return out


def cosine_dissim_matrix(a):
    """(1 - cos(a_i, a_j)) / 2 (representation_similarity.py:15-18).  1 - c and the halving are exact or correctly rounded fp32
    steps on the device matrix (one fused elementwise launch of torch: bookkeeping, not a product)."""
    return (1.0 - cosine_matrix(a)) / 2.0


def strict_upper_tri_items(A):
    """A[np.triu_indices(A.shape[0], k=1, m=A.shape[1])] (representation_similarity.py:21-27) as a 1-D tensor on A's device, row by row"""
    if not torch.is_tensor(A) or A.dim() != 2:
        raise H.CvclError("strict_upper_tri_items: a 2-D tensor")
    i, j = torch.triu_indices(A.shape[0], A.shape[1], offset=1, device=A.device)
    return A[i, j]


def _triu_pearson(A, B):
    A, B = _rows(A, "rsa(A)"), _rows(B, "rsa(B)")
    Cn = A.shape[0]
    if A.shape != (Cn, Cn) or B.shape != (Cn, Cn):
        raise H.CvclError(f"rsa_of_dissim_matrices: two [C, C] matrices, got {tuple(A.shape)} and {tuple(B.shape)}")
    if not (3 <= Cn <= MAX_ROWS):
        raise H.CvclError(f"rsa_of_dissim_matrices: C {Cn} outside 3..{MAX_ROWS}")
    lib = H.lib()
    out = torch.empty(6, dtype=torch.float64, device=A.device)
    ws = torch.empty(lib.cvcl_triu_pearson_workspace_bytes(Cn), dtype=torch.uint8, device=A.device)
    H.check(lib.cvcl_triu_pearson_f32(H.ptr(A), H.ptr(B), Cn, H.ptr(out), H.ptr(ws), ws.numel(), H.stream_ptr()), "cvcl_triu_pearson_f32")
    return out


def pearson_p_value(r, n):
    """two-sided p of scipy.stats.pearsonr for correlation r over n pairs (its exact beta form), None without scipy"""
    try:
        from scipy import stats
    except ImportError:
        return None
    if not np.isfinite(r) or n < 3:
        return float("nan")
    ab = n / 2.0 - 1.0
    return float(2.0 * stats.beta(ab, ab, loc=-1.0, scale=2.0).cdf(-abs(float(r))))


def triu_moments(A, B):
    """the six doubles of cvcl_triu_pearson_f32 as a dict (n, r, mean_a, mean_b, var_a, var_b); one download"""
    m = _triu_pearson(A, B).cpu().numpy()
    return {"n": int(m[0]), "r": float(m[1]), "mean_a": float(m[2]), "mean_b": float(m[3]), "var_a": float(m[4]), "var_b": float(m[5])}


def rsa_of_dissim_matrices(A, B):
    """scipy.stats.pearsonr over the strict upper triangles of A and B (representation_similarity.py:30-39; alignment.py:230-232)
    -> (r, p): r from the device (NaN when a side is constant), p from scipy applied to (r, n), None when scipy is absent."""
    m = triu_moments(A, B)
    return m["r"], pearson_p_value(m["r"], m["n"])


def paired_distances(x, y, eps=PAIRWISE_EPS):
    """F.pairwise_distance(x_i, y_i, p=2) = ||x_i - y_i + eps||_2 per row (embeddings.py:106-111): x, y [C, D] -> [C] fp32"""
    x, y = _rows(x, "paired_distances(x)"), _rows(y, "paired_distances(y)")
    if x.shape != y.shape:
        raise H.CvclError(f"paired_distances: {tuple(x.shape)} against {tuple(y.shape)}")
    Cn, D = x.shape
    if Cn > MAX_C or D > MAX_D:
        raise H.CvclError(f"paired_distances: C {Cn}, D {D} outside C <= {MAX_C}, D <= {MAX_D}")
    d = torch.empty(Cn, dtype=torch.float32, device=x.device)
    H.check(H.lib().cvcl_paired_l2_f32(H.ptr(x), H.ptr(y), Cn, D, float(eps), H.ptr(d), H.stream_ptr()), "cvcl_paired_l2_f32")
    return d


def category_words(categories, use_kitty_label=False):
    """the word of each category folder; ``use_kitty_label``: cat -> kitty, the reference's eval_categories[3] = "kitty" """
    return [KITTY.get(c, c) if use_kitty_label else c for c in categories]


def word_ids(words, vocab):
    missing = [w for w in words if w not in vocab]
    if missing:
        raise KeyError(f"not in the vocabulary: {missing}")
    return [int(vocab[w]) for w in words]


def encode_words(model, words, vocab):
    """One single-token utterance of length 1 per word through ``encode_text``, all words in one batch (alignment.py:123-134 encodes
    them one by one) -> [C, E] fp32 on the model's device.  ``model``: a MultiModalModel or a MultiModalLitModel."""
    ids = word_ids(words, vocab)
    mm = getattr(model, "model", model)
    dev = next(mm.parameters()).device
    text = torch.tensor(ids, dtype=torch.long, device=dev).view(-1, 1)
    length = torch.ones(len(ids), dtype=torch.long, device=dev)
    with torch.no_grad():
        feats = mm.encode_text(text, length)[0]
    return feats.float().contiguous()


def interleave(image_rows, text_rows):
    """image_0, text_0, image_1, text_1, ... (alignment.py:142-146, with C rows instead of the hard-coded 22)"""
    if image_rows.shape != text_rows.shape:
        raise ValueError(f"{tuple(image_rows.shape)} image rows against {tuple(text_rows.shape)} text rows")
    return torch.stack((image_rows, text_rows), dim=1).reshape(2 * image_rows.shape[0], image_rows.shape[1]).contiguous()


def alignment(image_features, label_ids, text_features):
    """The matrices and the correlation of alignment.py:102-232 from frame features [N, D], their category ids [N] (host integers in
    [0, C)) and the word features [C, D]: a dict of numpy arrays ``mean_image_features`` [C, D], ``image_sims`` / ``text_sims`` /
    ``image_text_sims`` [C, C], ``combined_sims`` [2C, 2C] (image_0, text_0, image_1, ...), ``counts`` [C], and ``pearson_r`` /
    ``pearson_p`` / ``n_pairs`` of the two strict upper triangles.  Everything is enqueued first; the download at the end is the
    only synchronisation (the empty-class check runs on the downloaded counts)."""
    t = _rows(text_features, "alignment(text_features)")
    Cn = t.shape[0]
    means, counts = _class_means(image_features, label_ids, Cn)
    if means.shape[1] != t.shape[1]:
        raise H.CvclError(f"image features are {means.shape[1]} wide, text features {t.shape[1]}")
    image_sims, text_sims = cosine_matrix(means), cosine_matrix(t)
    image_text_sims = cosine_matrix(means, t)
    combined_sims = cosine_matrix(interleave(means, t))
    moments = _triu_pearson(image_sims, text_sims)
    out = {"mean_image_features": means.cpu().numpy(), "image_sims": image_sims.cpu().numpy(), "text_sims": text_sims.cpu().numpy(),
           "image_text_sims": image_text_sims.cpu().numpy(), "combined_sims": combined_sims.cpu().numpy(),
           "counts": counts.cpu().numpy()}
    _refuse_empty(out["counts"])
    m = moments.cpu().numpy()
    out["pearson_r"], out["n_pairs"] = float(m[1]), int(m[0])
    out["pearson_p"] = pearson_p_value(out["pearson_r"], out["n_pairs"])
    return out


# ---- sampling and the reference's files -----------------------------------------------------------------------------------------------
def sample_indices(labels, per_class=200, replace=True, seed=0):
    """np.random.choice(frames, size=min(len(frames), per_class)) per category in sorted order under np.random.seed(seed):
    with replacement as alignment.py:86 has it, ``replace=False`` as embeddings.py:72.  ``labels``: one category per frame, frames in
    sorted order inside a category -> (indices into the frames, their categories)."""
    cats = sorted({str(x) for x in labels})
    rs = np.random.RandomState(seed)                     # the stream of np.random.seed(seed); the global state is left alone
    idx, out_labels = [], []
    for c in cats:
        members = np.array([i for i, x in enumerate(labels) if str(x) == c])
        pick = rs.choice(members, size=min(len(members), per_class), replace=replace)
        idx.extend(int(i) for i in pick)
        out_labels.extend([c] * len(pick))
    return np.array(idx, dtype=np.int64), out_labels


def long_form_rows(image_sims, text_sims, words):
    """rows of <model>_joint_embeddings_sims: x outer, y inner (alignment.py:198-211)"""
    n = len(words)
    return [[float(image_sims[i, j]), float(text_sims[i, j]), words[i], words[j]] for i in range(n) for j in range(n)]


def _write_csv(path, header, rows):
    with open(path, "w", newline="") as f:                # pandas' to_csv(index=False): comma, \n, shortest float repr
        wr = csv.writer(f, lineterminator="\n")
        wr.writerow(header)
        wr.writerows(rows)


def tsne_rows(combined_sims, words):
    """alignment.py:163-175 in host numpy: TSNE(random_state=1, metric="precomputed", perplexity=7.5) on 1 - minmax(combined_sims).
    ``init="random"`` is passed explicitly: scikit-learn 1.7 refuses its default init="pca" with a precomputed metric, which the
    reference's older version silently replaced."""
    from sklearn.manifold import TSNE
    s = np.asarray(combined_sims, dtype=np.float64)
    normalized = (s - np.min(s)) / (np.max(s) - np.min(s))
    xy = TSNE(random_state=1, metric="precomputed", perplexity=7.5, init="random").fit_transform(1 - normalized)
    cats, mods = np.repeat(words, 2), np.tile(["image", "text"], len(words))
    return [[float(xy[i, 0]), float(xy[i, 1]), str(cats[i]), str(mods[i])] for i in range(len(cats))]


def write_results(out_dir, model_name, seed, words, all_image_features, all_text_features, res, distances, tsne=False, accuracies=None):
    """The reference's files (alignment.py:137-139, :178, :211, :226) plus alignment.json; returns the dict written to the latter."""
    os.makedirs(out_dir, exist_ok=True)
    stem = os.path.join(out_dir, f"{model_name}_")
    np.save(f"{stem}all_image_features_seed_{seed}.npy", np.asarray(all_image_features))
    np.save(f"{stem}mean_image_features_seed_{seed}.npy", res["mean_image_features"])
    np.save(f"{stem}all_text_features_seed_{seed}.npy", np.asarray(all_text_features))
    n = len(words)
    _write_csv(f"{stem}joint_embeddings_sims_seed_{seed}.csv", ["image_sims", "text_sims", "eval_category_x", "eval_category_y"],
               long_form_rows(res["image_sims"], res["text_sims"], words))
    _write_csv(f"{stem}image_text_embeddings_sims_seed_{seed}.csv", ["image_text_sims", "eval_category_x", "eval_category_y"],
               [[float(res["image_text_sims"][i, j]), words[i], words[j]] for i in range(n) for j in range(n)])
    if tsne:
        _write_csv(f"{stem}joint_embeddings_tsne_seed_{seed}.csv", ["x", "y", "eval_category", "modality"],
                   tsne_rows(res["combined_sims"], words))
    summary = {"r": res["pearson_r"], "p": res["pearson_p"], "n_pairs": res["n_pairs"],
               "paired_distances": {w: float(d) for w, d in zip(words, distances)}}
    if accuracies is not None:                           # embeddings.py:113-118: distance against classification accuracy
        missing = [w for w in words if w not in accuracies]
        if missing:
            raise KeyError(f"no accuracy for: {missing}")
        acc = np.array([float(accuracies[w]) for w in words], dtype=np.float64)
        d = np.asarray(distances, dtype=np.float64)
        r = float(np.corrcoef(d, acc)[0, 1]) if n >= 2 else float("nan")
        summary["distance_accuracy"] = {"r": r, "p": pearson_p_value(r, n), "n": n}
    with open(os.path.join(out_dir, "alignment.json"), "w") as f:
        json.dump(summary, f)
    return summary


# ---- alignment.py (the script) ---------------------------------------------------------------------------------------------------------
class ImageTower(torch.nn.Module):
    """encode_image's embedding as a plain [n, 3, H, W] -> [n, E] encoder (what neighbors.extract_features calls)"""

    def __init__(self, model):
        super().__init__()
        self.model = model

    def forward(self, x):
        return self.model.encode_image(x)[0].float()


def preprocessed_features(encoder, frames, device, batch=256):
    """features [N, D] fp32 of a list of uint8 [H, W, 3] frames of any sizes: each batch through the reference's evaluation transform
    on the device (preprocess.DevicePreprocess), then the encoder"""
    from .preprocess import DevicePreprocess
    pre = DevicePreprocess(device=device)
    feats = [NB.extract_features(encoder, pre(frames[s:s + batch]), batch) for s in range(0, len(frames), batch)]
    return torch.cat(feats)


def parser():
    import argparse
    ap = argparse.ArgumentParser(description="image-text alignment of a CVCL model (analysis_cvcl/alignment.py, embeddings.py:106-118)")
    ap.add_argument("--eval_dir", default=None, help="class-per-folder evaluation frames; the folder name is the category word")
    ap.add_argument("--dataset", default="folders", choices=("folders", "synthetic"))
    ap.add_argument("--random_init", action="store_true")
    ap.add_argument("--checkpoint", default=None, help="a MultiModalLitModel checkpoint (.ckpt)")
    ap.add_argument("--precision", default="32", choices=("32", "32-split"))
    ap.add_argument("--batch_size", type=int, default=256)
    ap.add_argument("--per_class", type=int, default=200)
    ap.add_argument("--no_replace", action="store_true", help="sample frames without replacement (embeddings.py:72)")
    ap.add_argument("--use_kitty_label", action="store_true", help='the word of category "cat" is "kitty" (alignment.py:119)')
    ap.add_argument("--resize", action="store_true",
                    help="resize every frame to 224 x 224 (bicubic, as the reference's transform) on the device; frames may differ in size")
    ap.add_argument("--seed", type=int, default=0)
    ap.add_argument("--model_name", default="cvc")
    ap.add_argument("--out", default=os.path.join("results", "alignment"))
    ap.add_argument("--tsne", action="store_true")
    ap.add_argument("--accuracies", default=None, help="JSON {word: percent correct}: adds the distance / accuracy correlation")
    return ap


def build_model(args, device, normalize_features=False):
    """the two-tower model: a checkpoint, or the reference's CVCL configuration (embedding text encoder, E = 512) at random weights
    (``normalize_features``: of the random model; a checkpoint keeps its own)"""
    import argparse
    from .multimodal import TextEncoder, VisionEncoder
    from .multimodal_data_module import read_vocab
    from .multimodal_lit import MultiModalLitModel
    torch.manual_seed(args.seed)
    if args.checkpoint:
        lit = MultiModalLitModel.load_from_checkpoint(args.checkpoint, map_location=device)
    elif args.random_init:
        cfg = argparse.Namespace(
            embedding_type="flat", embedding_dim=512, pretrained_cnn=False, cnn_model="resnext50_32x4d", cnn_dino=False, vit_dino=False,
            finetune_cnn=False, text_encoder="embedding", captioning=False, attention=False, attention_gate=False, crange=1,
            dropout_i=0.5, dropout_o=0.0, pos_embed_type="no_pos_embed", normalize_features=bool(normalize_features), sim="max",
            temperature=0.07, fix_temperature=True, tie=True, bias=True, lr=1e-4, weight_decay=0.1, lambda_mm=1.0, lambda_lm=0.0,
            lambda_ar=0.0, optimize_unused=True, lr_scheduler=True, optimizer=torch.optim.AdamW)
        lit = MultiModalLitModel(VisionEncoder(cfg), TextEncoder(read_vocab(), 2048, cfg), cfg)
    else:
        raise SystemExit("--checkpoint PATH or --random_init")
    lit.to(device).eval()
    lit.set_precision(args.precision)
    for p in lit.parameters():
        p.requires_grad = False
    return lit


def main(args):
    from .multimodal_data_module import read_vocab
    if not torch.cuda.is_available():
        raise H.CvclError("alignment.py needs a GPU (the analysis has no CPU fallback)")
    dev = torch.device("cuda:0")
    if args.dataset == "synthetic":
        d = NB.synthetic_sets(args.seed, n_classes=len(SYNTHETIC_WORDS))
        frames = d["train"]
        labels = [SYNTHETIC_WORDS[int(l.split("_")[1])] for l in d["train_labels"]]
    else:
        if not args.eval_dir:
            raise SystemExit("--eval_dir is required (or --dataset synthetic)")
        frames, labels, _names = (NB.load_folder_list_u8 if args.resize else NB.load_folder_u8)(args.eval_dir)
    idx, picked = sample_indices(labels, args.per_class, not args.no_replace, seed=0)
    categories = sorted(set(picked))
    words = category_words(categories, args.use_kitty_label)
    vocab = read_vocab()
    word_ids(words, vocab)                               # an unknown word fails before the model is built
    (label_ids,) = NB._label_ids(picked)
    lit = build_model(args, dev)
    if args.resize:
        chosen = [frames[int(i)].permute(1, 2, 0) if torch.is_tensor(frames) else frames[int(i)] for i in idx]     # [H, W, 3] each
        feats = preprocessed_features(ImageTower(lit.model), chosen, dev, args.batch_size)
    else:
        feats = NB.extract_features(ImageTower(lit.model), frames[torch.from_numpy(idx)].to(dev), args.batch_size)
    text = encode_words(lit, words, vocab)
    res = alignment(feats, label_ids, text)
    dist = paired_distances(torch.from_numpy(res["mean_image_features"]).to(dev), text).cpu().numpy()
    accuracies = None
    if args.accuracies:
        with open(args.accuracies) as f:
            accuracies = json.load(f)
    summary = write_results(args.out, args.model_name, args.seed, words, feats.cpu().numpy(), text.cpu().numpy(), res, dist,
                            tsne=args.tsne, accuracies=accuracies)
    print(dist)
    if "distance_accuracy" in summary:
        print(f"PearsonRResult(statistic={summary['distance_accuracy']['r']}, pvalue={summary['distance_accuracy']['p']})")
    print(f"PearsonRResult(statistic={res['pearson_r']}, pvalue={res['pearson_p']})")
    return summary
