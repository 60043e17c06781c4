"""Train / eval nearest-neighbour searches of the reference's leakage check (analysis_cvcl/duplicates.py) on the HIP path.

Feature space: ``nearest_cosine`` is F.cosine_similarity on broadcast operands + max / argmax (duplicates.py:576-577 + 604-605 per
category, :805-809 over all training frames) as one ``cvcl_nn_cosine`` launch sequence that never writes the queries x base
matrix; ``nn_classify`` and ``same_category_matches`` restate the bookkeeping around it (:795-838, :594-612).  Pixel space:
``nearest_pixels`` is the per-frame loop of :988-1002 on 8-bit frames (``cvcl_nn_l1_u8``: exact integer channel sums, the distance
in double).  ``extract_features`` runs the eval-mode pooled output of the DINO ResNeXt (fc = Identity, utils.py:199-214).

Beyond the reference, which has only the nearest frame: ``knn_cosine`` returns the k closest base rows per query (``cvcl_knn_cosine``,
the same arithmetic), ``knn_vote`` the weighted vote over them (``cvcl_knn_vote``) and ``knn_classify`` the weighted k-NN
classification that is the training-free evaluation of a DINO encoder (k = 20, T = 0.07).

Perceptual hash, the check the reference names first ("exact and approximate duplicates"): ``average_hash`` is ahash (:28-41) in an
integer definition of the project's own (``cvcl_ahash_u8``), ``nearest_hamming`` the closest hash by differing bits
(``cvcl_hamming_nn``), ``nearest_digit_ratio`` the nested fuzz.ratio loops of :333-342 as one grouped search
(``cvcl_digit_ratio_nn``), and ``hash_duplicates`` the bookkeeping of :81-105 and :316-349.  cv2 and thefuzz are not used, and the
definitions have not been compared with them (DESIGN.md section 9 "Perceptual-hash duplicates" names the departures)."""
from __future__ import annotations

import csv
import ctypes as C
import json
import os

import numpy as np
import torch

from . import _hip as H
from .linear_probe import IMAGENET_MEAN, IMAGENET_STD, MODEL_NAME

COSINE_EPS = 1e-8                                    # F.cosine_similarity's default


def _device_tensor(t, what):
    if not torch.is_tensor(t) or not t.is_cuda:
        raise H.CvclError(f"{what}: the nearest-neighbour searches need device tensors (got {type(t).__name__}"
                          f"{'' if not torch.is_tensor(t) else ' on ' + str(t.device)}); there is no CPU fallback")


def _group_ids(query_groups, base_groups, nq, nb, device):
    if (query_groups is None) != (base_groups is None):
        raise H.CvclError("query_groups and base_groups go together")
    if query_groups is None:
        return None, None
    qg = torch.as_tensor(query_groups).to(device=device, dtype=torch.int32).contiguous()
    bg = torch.as_tensor(base_groups).to(device=device, dtype=torch.int32).contiguous()
    if qg.shape != (nq,) or bg.shape != (nb,):
        raise H.CvclError(f"group arrays must be [{nq}] and [{nb}], got {tuple(qg.shape)} and {tuple(bg.shape)}")
    return qg, bg


def _rows_f32(t, what):
    if t.dim() != 2 or t.dtype != torch.float32:
        raise H.CvclError(f"{what}: expected [N, D] fp32 rows, got {tuple(t.shape)} {t.dtype}")
    return t if H.row_strided(t) else t.contiguous()


def _cosine_search(name, query, base, k, query_groups, base_groups, chunk, eps):
    """``nearest_cosine`` (k None: outputs [Nq], ``cvcl_nn_cosine``) and ``knn_cosine`` (outputs [Nq, k], ``cvcl_knn_cosine``)"""
    _device_tensor(query, f"{name}(query)")
    _device_tensor(base, f"{name}(base)")
    q, b = _rows_f32(query, "query"), _rows_f32(base, "base")
    (Nq, D), Nb = q.shape, b.shape[0]
    if b.shape[1] != D:
        raise H.CvclError(f"query rows are {D} wide, base rows {b.shape[1]}")
    qg, bg = _group_ids(query_groups, base_groups, Nq, Nb, q.device)
    shape, ks = ((Nq,), ()) if k is None else ((Nq, k), (k,))
    cos = torch.full(shape, float("-inf"), dtype=torch.float32, device=q.device)
    idx = torch.full(shape, -1, dtype=torch.int64, device=q.device)
    if Nq == 0 or Nb == 0:
        return cos, idx
    lib = H.lib()
    entry = "cvcl_nn_cosine" if k is None else "cvcl_knn_cosine"
    search, workspace_bytes = getattr(lib, entry), getattr(lib, entry + "_workspace_bytes")
    step = Nb if chunk is None else max(1, int(chunk))
    ws = torch.empty(workspace_bytes(Nq, min(step, Nb), D, *ks), dtype=torch.uint8, device=q.device)
    for s in range(0, Nb, step):
        n = min(step, Nb - s)
        H.check(search(*H.rows(q), *H.rows(b[s:s + n]), Nq, n, D, *ks, eps, H.ptr(qg), None if bg is None else H.ptr(bg[s:]),
                       s, int(s > 0), H.ptr(cos), H.ptr(idx), H.ptr(ws), ws.numel(), H.stream_ptr()), entry)
    return cos, idx


def nearest_cosine(query, base, query_groups=None, base_groups=None, chunk=None, eps=COSINE_EPS):
    """max_j / argmax_j of F.cosine_similarity(query[:, None, :], base[None, :, :], dim=-1): query [Nq, D], base [Nb, D] fp32 device
    rows (a row stride above D is read in place) -> (cos [Nq] fp32, idx [Nq] int64).  With groups (one integer per row on both
    sides) only pairs of equal group compete; a query without an eligible base row gets -inf and -1.  Ties go to the lower index.
    ``chunk``: base rows per launch sequence; the running best is merged on the device, bit for bit the one-shot result."""
    return _cosine_search("nearest_cosine", query, base, None, query_groups, base_groups, chunk, eps)


def knn_cosine(query, base, k, query_groups=None, base_groups=None, chunk=None, eps=COSINE_EPS):
    """The k base rows of largest cosine per query, sorted by (cosine descending, index ascending): query [Nq, D], base [Nb, D] fp32
    device rows (a row stride above D is read in place) -> (cos [Nq, k] fp32, idx [Nq, k] int64); slots beyond the number of
    eligible rows hold -inf and -1.  Groups and ``chunk`` as ``nearest_cosine``; a pair's cosine has ``nearest_cosine``'s bits, so
    k = 1 is that search.  ``cvcl_knn_cosine``: no queries x base matrix is written."""
    k = int(k)
    if not 1 <= k <= H.KNN_MAX_K:
        raise H.CvclError(f"knn_cosine: k {k} outside 1..{H.KNN_MAX_K}")
    return _cosine_search("knn_cosine", query, base, k, query_groups, base_groups, chunk, eps)


def knn_vote(cos, idx, base_labels, n_classes, temperature=0.07):
    """The weighted k-NN vote of the DINO evaluation over the lists ``knn_cosine`` returns: cos [Nq, k] fp32, idx [Nq, k] int64,
    base_labels [Nb] integers (all on the device) -> (scores [Nq, n_classes] fp32 = the sum of exp(cos / temperature) over the
    entries of each class, in double, one rounding; pred [Nq] int64 = its arg-max, the lowest class on a tie, -1 without an entry).
    ``temperature=0``: every entry weighs 1.  Entries of index -1 (or beyond the labels, or of a label outside the classes) are
    left out."""
    _device_tensor(cos, "knn_vote(cos)")
    _device_tensor(idx, "knn_vote(idx)")
    _device_tensor(base_labels, "knn_vote(base_labels)")
    if cos.dim() != 2 or cos.dtype != torch.float32 or idx.shape != cos.shape or idx.dtype != torch.int64:
        raise H.CvclError(f"knn_vote: expected cos [Nq, k] fp32 and idx [Nq, k] int64, got {tuple(cos.shape)} {cos.dtype} and "
                          f"{tuple(idx.shape)} {idx.dtype}")
    if base_labels.dim() != 1:
        raise H.CvclError(f"knn_vote: base_labels must be [Nb], got {tuple(base_labels.shape)}")
    Nq, k = cos.shape
    lab = base_labels.to(torch.int32).contiguous()
    scores = torch.zeros(Nq, int(n_classes), dtype=torch.float32, device=cos.device)
    pred = torch.full((Nq,), -1, dtype=torch.int64, device=cos.device)
    if Nq == 0:
        return scores, pred
    H.check(H.lib().cvcl_knn_vote(H.ptr(cos.contiguous()), H.ptr(idx.contiguous()), Nq, k, H.ptr(lab), lab.numel(), int(n_classes),
                                  float(temperature), H.ptr(scores), H.ptr(pred), H.stream_ptr()), "cvcl_knn_vote")
    return scores, pred


def pixel_weights(std):
    """w_c = 1 / (255 std_c): sum_c w_c sum_p |a - b| over 8-bit frames is sum |norm(a) - norm(b)| over ToTensor + Normalize frames"""
    return [1.0 / (255.0 * float(s)) for s in std]


def nearest_pixels(query_u8, base_u8, std=IMAGENET_STD, query_groups=None, base_groups=None, chunk=None):
    """min_j / argmin_j of sum |norm(query_i) - norm(base_j)| (duplicates.py:993-1002) on uint8 device frames [N, C, H, W] (or
    [N, C, HW]) -> (dist [Nq] float64, idx [Nq] int64, sums [Nq, C] int64: the winner's exact per-channel sums of absolute byte
    differences; dist = sums[0] w[0] + sums[1] w[1] + ... in double with w = pixel_weights(std)).  The channel sums are exact
    integers: unlike the reference's fp32 sum of 150 528 terms the distance carries no accumulated rounding.  Ties go to the lower
    index; a query without an eligible base frame gets +inf and -1.  ``base_u8`` may also be an iterable of device chunks (they
    need not be resident together; groups are not available then), and ``chunk`` splits a resident base set the same way."""
    _device_tensor(query_u8, "nearest_pixels(query)")
    resident = torch.is_tensor(base_u8)
    if resident:
        _device_tensor(base_u8, "nearest_pixels(base)")
    elif query_groups is not None or base_groups is not None:
        raise H.CvclError("groups need a resident base set")
    if query_u8.dtype != torch.uint8 or query_u8.dim() not in (3, 4):
        raise H.CvclError(f"expected uint8 frames [N, C, H, W], got {tuple(query_u8.shape)} {query_u8.dtype}")
    q = query_u8.contiguous()
    Nq, Cn = q.shape[0], q.shape[1]
    HW = int(np.prod(q.shape[2:]))
    w = pixel_weights(std)
    if len(w) != Cn:
        raise H.CvclError(f"{Cn} channels but {len(w)} std values")
    warr = (C.c_double * Cn)(*w)
    dist = torch.full((Nq,), float("inf"), dtype=torch.float64, device=q.device)
    idx = torch.full((Nq,), -1, dtype=torch.int64, device=q.device)
    sums = torch.zeros(Nq, Cn, dtype=torch.int32, device=q.device)               # uint32 bits
    lib = H.lib()

    def chunks():
        if not resident:
            for c in base_u8:
                _device_tensor(c, "nearest_pixels(base chunk)")
                yield c, None
            return
        step = base_u8.shape[0] if chunk is None else max(1, int(chunk))
        for s in range(0, base_u8.shape[0], step):
            yield base_u8[s:s + step], s

    qg, bg = _group_ids(query_groups, base_groups, Nq, base_u8.shape[0], q.device) if resident else (None, None)
    seen = 0
    for b, s in chunks():
        if b.dtype != torch.uint8 or tuple(b.shape[1:]) != tuple(query_u8.shape[1:]):
            raise H.CvclError(f"base frames {tuple(b.shape[1:])} {b.dtype} do not match the queries' {tuple(query_u8.shape[1:])} uint8")
        b = b.contiguous()
        n = b.shape[0]
        if n == 0 or Nq == 0:
            continue
        ws = torch.empty(lib.cvcl_nn_l1_u8_workspace_bytes(Nq, n, Cn), dtype=torch.uint8, device=q.device)
        H.check(lib.cvcl_nn_l1_u8(H.ptr(q), H.ptr(b), Nq, n, Cn, HW, warr, H.ptr(qg), None if bg is None else H.ptr(bg[s:]),
                                  seen, int(seen > 0), H.ptr(dist), H.ptr(idx), H.ptr(sums), H.ptr(ws), ws.numel(), H.stream_ptr()),
                "cvcl_nn_l1_u8")
        seen += n
    return dist, idx, sums.to(torch.int64) & 0xFFFFFFFF


# ---- perceptual hash (duplicates.py:28-41, :333-342) ------------------------------------------------------------------------------
HASH_NO_MATCH = 64 * H.AHASH_WORDS + 1               # the Hamming distance of a query without an eligible base row: 257


def average_hash(frames_u8, layout="NCHW", return_cells=False):
    """ahash (duplicates.py:28-41) of 8-bit RGB device frames, in the project's integer definition (cvcl_hip.h ``cvcl_ahash_u8``:
    ITU-R 601 grey as Pillow's convert("L"), bilinear 16 x 16 at half-pixel centres without antialiasing, bit i = 16 y + x set where
    the cell is >= the mean): uint8 [N, 3, H, W] (``layout="NCHW"``) or [N, H, W, 3] (``"NHWC"``), H, W >= 16, read in place
    through its strides (a crop or a permuted view is not copied) -> int64 [N, 4] on the device, word w = bits 64 w .. 64 w + 63.
    ``return_cells``: also the 16 x 16 rounded cell values, int32 [N, 256]."""
    _device_tensor(frames_u8, "average_hash(frames)")
    if layout not in ("NCHW", "NHWC"):
        raise H.CvclError(f"average_hash: layout {layout!r} (NCHW or NHWC)")
    t = frames_u8
    if t.dtype != torch.uint8 or t.dim() != 4 or t.shape[1 if layout == "NCHW" else 3] != 3:
        raise H.CvclError(f"average_hash: expected uint8 RGB frames in {layout}, got {tuple(t.shape)} {t.dtype}")
    if layout == "NHWC":
        t = t.permute(0, 3, 1, 2)
    N, _, Hh, Ww = t.shape
    if Hh < H.AHASH_SIDE or Ww < H.AHASH_SIDE:
        raise H.CvclError(f"average_hash: frames of {Hh} x {Ww} are below {H.AHASH_SIDE} x {H.AHASH_SIDE}")
    if min(t.stride()) < 1:                              # (an expanded view)
        t = t.contiguous()
    out = torch.zeros(N, H.AHASH_WORDS, dtype=torch.int64, device=t.device)
    cells = torch.zeros(N, H.AHASH_SIDE * H.AHASH_SIDE, dtype=torch.int32, device=t.device) if return_cells else None
    if N:
        sn, sc, sy, sx = t.stride()
        H.check(H.lib().cvcl_ahash_u8(t.data_ptr(), N, Hh, Ww, sn, sc, sy, sx, H.ptr(out), H.ptr(cells), H.stream_ptr()), "cvcl_ahash_u8")
    return (out, cells) if return_cells else out


def _hash_words(hashes):
    a = hashes.detach().cpu().numpy() if torch.is_tensor(hashes) else np.asarray(hashes)
    if a.ndim != 2 or a.shape[1] != H.AHASH_WORDS or a.dtype != np.int64:
        raise H.CvclError(f"expected int64 [N, {H.AHASH_WORDS}] hash words, got {a.shape} {a.dtype}")
    return a.view(np.uint64)


def hash_ints(hashes):
    """the reference's ``hash_value`` (duplicates.py:40) of each row of ``average_hash``'s output, as Python ints: the words are
    taken as unsigned, word w weighs 2^(64 w)"""
    return [sum(int(w) << (64 * k) for k, w in enumerate(row)) for row in _hash_words(hashes)]


def hash_digits(hashes):
    """str(hash_value) per row, on the host, as ``cvcl_digit_ratio_nn`` reads it -> (uint8 [N, 128] numpy array of digit values
    0..9, zero beyond the length; int32 [N] lengths).  The zero hash is "0", length 1; a 256-bit hash has at most 78 digits."""
    ints = hash_ints(hashes)
    digits = np.zeros((len(ints), H.DIGITS_MAX), dtype=np.uint8)
    lens = np.zeros(len(ints), dtype=np.int32)
    for i, v in enumerate(ints):
        s = str(v)
        lens[i] = len(s)
        digits[i, :len(s)] = np.frombuffer(s.encode(), dtype=np.uint8) - ord("0")
    return digits, lens


def nearest_hamming(query, base, query_groups=None, base_groups=None):
    """min_j / the lowest argmin_j of popcount(query_i xor base_j) over int64 [N, 4] device hashes (``cvcl_hamming_nn``) ->
    (dist [Nq] int32, idx [Nq] int64).  Groups as ``nearest_cosine``; a query without an eligible base row gets 257 and -1."""
    _device_tensor(query, "nearest_hamming(query)")
    _device_tensor(base, "nearest_hamming(base)")
    for t, what in ((query, "query"), (base, "base")):
        if t.dim() != 2 or t.shape[1] != H.AHASH_WORDS or t.dtype != torch.int64:
            raise H.CvclError(f"nearest_hamming: {what} must be int64 [N, {H.AHASH_WORDS}], got {tuple(t.shape)} {t.dtype}")
    q, b = query.contiguous(), base.contiguous()
    Nq, Nb = q.shape[0], b.shape[0]
    qg, bg = _group_ids(query_groups, base_groups, Nq, Nb, q.device)
    dist = torch.full((Nq,), HASH_NO_MATCH, dtype=torch.int32, device=q.device)
    idx = torch.full((Nq,), -1, dtype=torch.int64, device=q.device)
    if Nq == 0 or Nb == 0:
        return dist, idx
    lib = H.lib()
    ws = torch.empty(lib.cvcl_hamming_nn_workspace_bytes(Nq, Nb), dtype=torch.uint8, device=q.device)
    H.check(lib.cvcl_hamming_nn(H.ptr(q), H.ptr(b), Nq, Nb, H.ptr(qg), H.ptr(bg), H.ptr(dist), H.ptr(idx), H.ptr(ws), ws.numel(),
                                H.stream_ptr()), "cvcl_hamming_nn")
    return dist, idx


def nearest_digit_strings(query_digits, query_len, base_digits, base_len, query_groups=None, base_groups=None):
    """max_j / the lowest argmax_j of fuzz.ratio between digit strings (``cvcl_digit_ratio_nn``): uint8 [N, ld] device rows of digit
    VALUES 0..9 with ld <= 128 on both sides and int32 [N] lengths in 1..ld -> (ratio [Nq] int32, idx [Nq] int64);
    ratio = round_half_even(200 LCS / (la + lb)).  A maximum of 0, or no eligible row, gives 0 and -1.  Groups as ``nearest_cosine``."""
    for t, what in ((query_digits, "query_digits"), (query_len, "query_len"), (base_digits, "base_digits"), (base_len, "base_len")):
        _device_tensor(t, f"nearest_digit_strings({what})")
    q, b = query_digits.contiguous(), base_digits.contiguous()
    if q.dim() != 2 or b.dim() != 2 or q.dtype != torch.uint8 or b.dtype != torch.uint8 or q.shape[1] != b.shape[1]:
        raise H.CvclError(f"nearest_digit_strings: expected uint8 [N, ld] rows of one width, got {tuple(q.shape)} {q.dtype} and "
                          f"{tuple(b.shape)} {b.dtype}")
    (Nq, ld), Nb = q.shape, b.shape[0]
    ql, bl = query_len.to(torch.int32).contiguous(), base_len.to(torch.int32).contiguous()
    if ql.shape != (Nq,) or bl.shape != (Nb,):
        raise H.CvclError(f"nearest_digit_strings: lengths must be [{Nq}] and [{Nb}], got {tuple(ql.shape)} and {tuple(bl.shape)}")
    qg, bg = _group_ids(query_groups, base_groups, Nq, Nb, q.device)
    ratio = torch.zeros(Nq, dtype=torch.int32, device=q.device)
    idx = torch.full((Nq,), -1, dtype=torch.int64, device=q.device)
    if Nq == 0 or Nb == 0:
        return ratio, idx
    lib = H.lib()
    ws = torch.empty(lib.cvcl_digit_ratio_nn_workspace_bytes(Nq, Nb), dtype=torch.uint8, device=q.device)
    H.check(lib.cvcl_digit_ratio_nn(H.ptr(q), H.ptr(ql), H.ptr(b), H.ptr(bl), Nq, Nb, ld, H.ptr(qg), H.ptr(bg), H.ptr(ratio), H.ptr(idx),
                                    H.ptr(ws), ws.numel(), H.stream_ptr()), "cvcl_digit_ratio_nn")
    return ratio, idx


def nearest_digit_ratio(query_hashes, base_hashes, query_groups=None, base_groups=None):
    """The reference's scan of duplicates.py:333-342 as one search: per query hash the base hash of largest
    fuzz.ratio(str(hash), str(hash)), the lowest index on a tie -> (ratio [Nq] int32, idx [Nq] int64; 0 and -1 where nothing
    scores above 0).  int64 [N, 4] device hashes; the decimal strings are written on the host (``hash_digits``)."""
    _device_tensor(query_hashes, "nearest_digit_ratio(query)")
    _device_tensor(base_hashes, "nearest_digit_ratio(base)")
    dev = query_hashes.device
    (qd, ql), (bd, bl) = hash_digits(query_hashes), hash_digits(base_hashes)
    return nearest_digit_strings(torch.from_numpy(qd).to(dev), torch.from_numpy(ql).to(dev), torch.from_numpy(bd).to(dev),
                                 torch.from_numpy(bl).to(dev), query_groups, base_groups)


def normalize_u8(frames_u8):
    """ToTensor + Normalize(ImageNet) of uint8 [N, 3, H, W] frames on their device, in linear_probe.load_image's arithmetic"""
    mean = torch.tensor(IMAGENET_MEAN, device=frames_u8.device).view(1, 3, 1, 1)
    std = torch.tensor(IMAGENET_STD, device=frames_u8.device).view(1, 3, 1, 1)
    return (frames_u8.float().div_(255.0) - mean) / std


def extract_features(model, frames, batch=256, precision=None):
    """Eval-mode features [N, D] fp32 of device frames (uint8 [N, 3, H, W], normalised here, or fp32 already normalised), ``batch``
    frames per pass.  A ``resnext.ResNet`` gives its pooled 2048-wide vector, which is what the reference's fc = Identity model
    returns (utils.py:199-214); any other encoder is called and must return [n, D].  ``precision``: "32" or "32-split"."""
    from .linear_probe import set_precision
    from .resnext import ResNet
    _device_tensor(frames, "extract_features(frames)")
    if precision is not None:
        if precision not in ("32", "32-split"):
            raise H.CvclError(f"extract_features: precision {precision!r} (the searches compare fp32 features: 32 or 32-split)")
        set_precision(model, precision)
    model.eval()
    out = None
    with torch.no_grad():
        for s in range(0, frames.shape[0], batch):
            x = frames[s:s + batch]
            x = normalize_u8(x) if x.dtype == torch.uint8 else x
            f = model.trunk(x)[0] if isinstance(model, ResNet) else model(x)
            if out is None:
                out = torch.empty(frames.shape[0], f.shape[1], dtype=torch.float32, device=frames.device)
            out[s:s + f.shape[0]] = f
    return out if out is not None else torch.empty(0, 0, dtype=torch.float32, device=frames.device)


# ---- bookkeeping (duplicates.py:594-612, 795-838) --------------------------------------------------------------------------------
def _label_ids(*label_lists):
    names = sorted({str(x) for labels in label_lists for x in labels})
    ids = {n: i for i, n in enumerate(names)}
    return [np.array([ids[str(x)] for x in labels], dtype=np.int32) for labels in label_lists]


def _host_pair(nearest):
    v, i = nearest
    v = v.detach().cpu().numpy() if torch.is_tensor(v) else np.asarray(v)
    i = i.detach().cpu().numpy() if torch.is_tensor(i) else np.asarray(i)
    return v, i.astype(np.int64)


def nn_classify(eval_feats, eval_labels, train_feats, train_labels, eval_filenames=None, train_filenames=None, nearest=None,
                chunk=None):
    """1-NN classification of every evaluation frame over ALL training frames (duplicates.py:795-838): category by category in
    sorted order, frames in their given order; the neighbour's label is the prediction.  ``nearest`` = a precomputed (cos, idx)
    pair replaces the search (the features are then not read).  Returns a dict: ``per_category`` {category: accuracy}, ``total``,
    ``matched_sims`` / ``mismatched_sims``, ``matched_train_filenames`` / ``matched_eval_filenames``, and ``rows`` =
    [eval_filename, train_filename, cosine_sim, "match" | "mismatch"].  Accuracies divide by the actual frame counts; the
    reference hard-codes ``/ 100`` per category and ``/ 2200`` in total, which is the same on Labeled-S only."""
    n_eval = len(eval_labels)
    eval_filenames = list(eval_filenames) if eval_filenames is not None else [str(i) for i in range(n_eval)]
    train_filenames = list(train_filenames) if train_filenames is not None else [str(i) for i in range(len(train_labels))]
    cos, idx = _host_pair(nearest if nearest is not None else nearest_cosine(eval_feats, train_feats, chunk=chunk))
    res = {"per_category": {}, "matched_sims": [], "mismatched_sims": [], "matched_train_filenames": [],
           "matched_eval_filenames": [], "rows": []}
    total = 0
    for cat in sorted({str(x) for x in eval_labels}):
        members = [j for j in range(n_eval) if str(eval_labels[j]) == cat]
        hits = 0
        for j in members:
            t = int(idx[j])
            sim = float(cos[j])
            if str(train_labels[t]) == cat:
                hits += 1
                res["matched_sims"].append(sim)
                res["matched_train_filenames"].append(train_filenames[t])
                res["matched_eval_filenames"].append(eval_filenames[j])
                res["rows"].append([eval_filenames[j], train_filenames[t], sim, "match"])
            else:
                res["mismatched_sims"].append(sim)
                res["rows"].append([eval_filenames[j], train_filenames[t], sim, "mismatch"])
        res["per_category"][cat] = hits / len(members)
        total += hits
    res["total"] = total / n_eval if n_eval else 0.0
    return res


def knn_classify(eval_feats, eval_labels, train_feats, train_labels, k=20, temperature=0.07, eval_filenames=None, train_filenames=None,
                 neighbours=None, votes=None, chunk=None):
    """Weighted k-NN classification of every evaluation frame over ALL training frames, the training-free evaluation of a DINO
    encoder (defaults k = 20, T = 0.07): ``knn_cosine`` + ``knn_vote`` with the bookkeeping of ``nn_classify`` -- categories in
    sorted order, frames in their given order, accuracies divided by the actual counts.  The classes are the sorted label names of
    both sets.  ``neighbours`` = a precomputed (cos [Nq, k], idx [Nq, k]) pair replaces the search and ``votes`` = a precomputed
    (scores [Nq, C], pred [Nq]) pair the vote (with both, the features are not read).  Returns a dict: ``k``, ``temperature``,
    ``per_category`` {category: accuracy}, ``total``, ``top5_total`` (the true class is among the five classes of largest score
    that got a vote at all; equal scores go to the lower class) and ``rows`` = [eval_filename, rank (from 1), train_filename,
    cosine_sim, train_label] for every list entry.  With k = 1 and temperature = 0 ``per_category`` and ``total`` are
    ``nn_classify``'s."""
    n_eval = len(eval_labels)
    eval_filenames = list(eval_filenames) if eval_filenames is not None else [str(i) for i in range(n_eval)]
    train_filenames = list(train_filenames) if train_filenames is not None else [str(i) for i in range(len(train_labels))]
    names = sorted({str(x) for labels in (eval_labels, train_labels) for x in labels})
    eval_ids, train_ids = _label_ids(eval_labels, train_labels)
    if neighbours is None:
        neighbours = knn_cosine(eval_feats, train_feats, k, chunk=chunk)
    if votes is None:
        cos_d, idx_d = neighbours
        votes = knn_vote(cos_d, idx_d, torch.from_numpy(train_ids).to(cos_d.device), len(names), temperature)
    cos, idx = _host_pair(neighbours)
    scores, pred = _host_pair(votes)
    res = {"k": int(cos.shape[1]), "temperature": float(temperature), "per_category": {}, "rows": []}
    total = top5 = 0
    for cat in sorted({str(x) for x in eval_labels}):
        members = [j for j in range(n_eval) if str(eval_labels[j]) == cat]
        hits = 0
        for j in members:
            hits += int(pred[j] >= 0 and names[int(pred[j])] == cat)
            best = np.argsort(-scores[j].astype(np.float64), kind="stable")[:5]
            top5 += int(any(c == eval_ids[j] and scores[j][c] > 0 for c in best))
            for r in range(cos.shape[1]):
                t = int(idx[j][r])
                if t >= 0:
                    res["rows"].append([eval_filenames[j], r + 1, train_filenames[t], float(cos[j][r]), str(train_labels[t])])
        res["per_category"][cat] = hits / len(members)
        total += hits
    res["total"] = total / n_eval if n_eval else 0.0
    res["top5_total"] = top5 / n_eval if n_eval else 0.0
    return res


def knn_summary(res):
    """the printed lines of a ``knn_classify`` result, in ``classify_summary``'s wording"""
    lines = [f"{res['k']}-NN accuracy for {cat}: {acc}" for cat, acc in res["per_category"].items()]
    lines.append(f"{res['k']}-NN total accuracy (T = {res['temperature']}): {res['total']}")
    lines.append(f"{res['k']}-NN top-5 accuracy: {res['top5_total']}")
    return lines


def write_top_k_matches(rows, path):
    """top_k_matches.csv, laid out as ``write_matched_results`` does"""
    with open(path, "w", newline="") as f:
        wr = csv.writer(f, lineterminator="\n")
        wr.writerow(["eval_filename", "rank", "train_filename", "cosine_sim", "train_label"])
        wr.writerows(rows)


def same_category_matches(eval_feats, eval_labels, train_feats, train_labels, eval_filenames, train_filenames, nearest=None,
                          chunk=None):
    """The top training frame of the SAME category for each evaluation frame (duplicates.py:594-612), as one grouped search:
    [{"train_frame", "eval_frame", "max_cosine_sim"}], categories in sorted order, frames in their given order.  ``nearest`` = a
    precomputed grouped (cos, idx) pair replaces the search.  A frame whose category has no training frame gets None, None."""
    if nearest is None:
        qg, bg = _label_ids(eval_labels, train_labels)
        nearest = nearest_cosine(eval_feats, train_feats, qg, bg, chunk=chunk)
    cos, idx = _host_pair(nearest)
    out = []
    for cat in sorted({str(x) for x in eval_labels}):
        for j in range(len(eval_labels)):
            if str(eval_labels[j]) != cat:
                continue
            t = int(idx[j])
            out.append({"train_frame": train_filenames[t] if t >= 0 else None, "eval_frame": eval_filenames[j],
                        "max_cosine_sim": float(cos[j]) if t >= 0 else None})
    return out


def pixel_records(eval_frames, eval_labels, train_frames, train_labels, dist, idx):
    """the records of duplicates.py:1013-1020, one per evaluation frame"""
    dist, idx = _host_pair((dist, idx))
    out = []
    for j in range(len(eval_frames)):
        t = int(idx[j])
        out.append({"eval_frame": eval_frames[j], "eval_label": str(eval_labels[j]), "min_label": str(train_labels[t]),
                    "min_frame": train_frames[t], "min_distance": float(dist[j]),
                    "correct": str(train_labels[t]) == str(eval_labels[j])})
    return out


def hash_duplicates(eval_frames, eval_labels, train_frames, train_labels, eval_names, train_names, layout="NCHW", hashes=None,
                    nearest_ratio=None, nearest_distance=None):
    """The perceptual-hash half of the leakage check: ``average_hash`` of both sets, then the bookkeeping of duplicates.py:81-105
    (calculate_exact_duplicates) and :316-349 (calculate_indirect_duplicates_with_hash), with one grouped search in place of the
    nested loops.  ``hashes`` = a precomputed (eval [Ne, 4], train [Nt, 4]) int64 pair replaces the hashing (the frames are then
    not read); ``nearest_ratio`` / ``nearest_distance`` = precomputed grouped (value, index) pairs replace the two searches.
    Returns a dict:
    ``hashed_eval_frames`` / ``hashed_train_frames`` {str(hash): file name}, a later frame overwriting an earlier one of the same
    hash as in the reference; ``exact_duplicates`` = the hashes in both (ascending) and ``n_exact_duplicates``;
    ``n_category_duplicates`` = the sum over the evaluation categories of the hashes that occur on both sides of the category;
    ``indirect_duplicates`` = [{"eval_frame", "train_frame", "distance"}] with the reference's keys: the same-category training
    frame of largest fuzz.ratio and that ratio ("" and 0 where nothing scores above 0), categories in sorted order, frames in their
    given order; ``hamming_duplicates`` = the same records with the same-category training frame of smallest Hamming distance
    ("" and 257 where the category has no training frame)."""
    if hashes is None:
        hashes = average_hash(eval_frames, layout), average_hash(train_frames, layout)
    eh, th = hashes
    ei, ti = hash_ints(eh), hash_ints(th)
    if len(ei) != len(eval_labels) or len(ti) != len(train_labels):
        raise H.CvclError(f"{len(ei)} / {len(ti)} hashes but {len(eval_labels)} / {len(train_labels)} labels")
    qg, bg = _label_ids(eval_labels, train_labels)
    if nearest_ratio is None:
        nearest_ratio = nearest_digit_ratio(eh, th, qg, bg)
    if nearest_distance is None:
        nearest_distance = nearest_hamming(eh, th, qg, bg)
    (ratio, ridx), (dist, didx) = _host_pair(nearest_ratio), _host_pair(nearest_distance)
    res = {"hashed_eval_frames": {str(h): n for h, n in zip(ei, eval_names)},
           "hashed_train_frames": {str(h): n for h, n in zip(ti, train_names)}}
    res["exact_duplicates"] = [str(h) for h in sorted(set(ei) & set(ti))]
    res["n_exact_duplicates"] = len(res["exact_duplicates"])
    res["n_category_duplicates"] = 0
    res["indirect_duplicates"], res["hamming_duplicates"] = [], []
    for cat in sorted({str(x) for x in eval_labels}):
        res["n_category_duplicates"] += len({h for h, l in zip(ei, eval_labels) if str(l) == cat}
                                            & {h for h, l in zip(ti, train_labels) if str(l) == cat})
        for j in range(len(eval_labels)):
            if str(eval_labels[j]) != cat:
                continue
            r, d = int(ridx[j]), int(didx[j])
            res["indirect_duplicates"].append({"eval_frame": eval_names[j], "train_frame": train_names[r] if r >= 0 else "",
                                               "distance": int(ratio[j]) if r >= 0 else 0})
            res["hamming_duplicates"].append({"eval_frame": eval_names[j], "train_frame": train_names[d] if d >= 0 else "",
                                              "distance": int(dist[j])})
    return res


def hash_summary(res):
    """the printed lines of duplicates.py:105 and :324"""
    return [f"total number of duplicates (using perceptual hash): {res['n_exact_duplicates']}",
            f"Total number of duplicates: {res['n_category_duplicates']}"]


def classify_summary(res):
    """the printed lines of duplicates.py:835-846"""
    lines = [f"Accuracy for {cat}: {acc}" for cat, acc in res["per_category"].items()]
    lines.append(f"Total accuracy: {res['total']}")
    m = np.array(res["matched_sims"], dtype=np.float64)
    n = len(res["matched_sims"]) + len(res["mismatched_sims"])
    lines.append(f"Total of matched cosine sims > 0.999: {int(np.sum(m > 0.99))}")          # (the reference's text and threshold)
    lines.append(f"Proportion of matched cosine sims > 0.95: {np.sum(m > 0.95) / n}")
    lines.append(f"Proportion of matched cosine sims > 0.9: {np.sum(m > 0.9) / n}")
    return lines


def matches_summary(matches):
    """the printed lines of duplicates.py:706-713"""
    s = np.array([m["max_cosine_sim"] for m in matches if m["max_cosine_sim"] is not None], dtype=np.float64)
    n = len(s)
    return [f"Proportion of max cosine sims between 0.7 and 0.8: {np.sum((s >= 0.7) & (s < 0.8)) / n}",
            f"Proportion of max cosine sims between 0.8 and 0.9: {np.sum((s >= 0.8) & (s < 0.9)) / n}",
            f"Proportion of max cosine sims between 0.9 and 1: {np.sum(s >= 0.9) / n}"]


def write_matched_results(rows, path):
    """matched_results.csv as pandas' to_csv(index=False) lays it out (duplicates.py:865-868)"""
    with open(path, "w", newline="") as f:
        wr = csv.writer(f, lineterminator="\n")
        wr.writerow(["eval_filename", "train_filename", "cosine_sim", "matched"])
        wr.writerows(rows)


# ---- data --------------------------------------------------------------------------------------------------------------------------
def load_folder_u8(root):
    """class-per-folder frames in ImageFolder's order -> (uint8 [N, 3, H, W] CPU tensor, labels, file names)"""
    from PIL import Image
    from .linear_probe import ImageFolder
    ds = ImageFolder(root, cache=False)
    frames = []
    for path, _ in ds.samples:
        with open(path, "rb") as f:
            frames.append(torch.from_numpy(np.asarray(Image.open(f).convert("RGB"), dtype=np.uint8).copy()).permute(2, 0, 1))
    if len({tuple(a.shape) for a in frames}) != 1:
        raise ValueError(f"{root}: frames of different sizes cannot be compared pixel by pixel")
    return torch.stack(frames), [ds.classes[t] for t in ds.targets], [p for p, _ in ds.samples]


def load_folder_list_u8(root):
    """class-per-folder frames in ImageFolder's order, of any and mixed sizes -> (list of uint8 [H, W, 3] CPU tensors as decoded,
    labels, file names): what ``preprocess.DevicePreprocess`` takes"""
    from PIL import Image
    from .linear_probe import ImageFolder
    ds = ImageFolder(root, cache=False)
    frames = []
    for path, _ in ds.samples:
        with open(path, "rb") as f:
            frames.append(torch.from_numpy(np.asarray(Image.open(f).convert("RGB"), dtype=np.uint8).copy()))
    return frames, [ds.classes[t] for t in ds.targets], [p for p, _ in ds.samples]


def synthetic_sets(seed=0, n_classes=4, train_per_class=12, eval_per_class=4, size=64):
    """A small seeded train / eval pair: blocky colour patterns plus noise.  In every class evaluation frame 0 is an exact copy of a
    training frame of its class and frame 1 a copy with +-1 on a few pixels.  Returns a dict of uint8 CPU tensors, labels, names
    and ``planted`` = [(eval index, train index, "duplicate" | "near")]."""
    rng = np.random.default_rng(seed)

    def frame():
        coarse = rng.integers(0, 256, (3, 8, 8))
        a = np.kron(coarse, np.ones((size // 8, size // 8), dtype=np.int64)) + rng.integers(-20, 21, (3, size, size))
        return np.clip(a, 0, 255).astype(np.uint8)

    train = np.stack([frame() for _ in range(n_classes * train_per_class)])
    train_labels = [f"class_{c:02d}" for c in range(n_classes) for _ in range(train_per_class)]
    evalf = np.stack([frame() for _ in range(n_classes * eval_per_class)])
    eval_labels = [f"class_{c:02d}" for c in range(n_classes) for _ in range(eval_per_class)]
    planted = []
    for c in range(n_classes):
        t0, t1 = c * train_per_class + int(rng.integers(train_per_class)), c * train_per_class + int(rng.integers(train_per_class))
        e0 = c * eval_per_class
        evalf[e0] = train[t0]
        planted.append((e0, t0, "duplicate"))
        near = train[t1].astype(np.int64)
        for _ in range(6):
            ch, y, x = int(rng.integers(3)), int(rng.integers(size)), int(rng.integers(size))
            near[ch, y, x] += 1 if near[ch, y, x] < 128 else -1
        evalf[e0 + 1] = near.astype(np.uint8)
        planted.append((e0 + 1, t1, "near"))
    return {"train": torch.from_numpy(train), "train_labels": train_labels,
            "train_names": [f"train/{l}/img_{i:04d}.png" for i, l in enumerate(train_labels)],
            "eval": torch.from_numpy(evalf), "eval_labels": eval_labels,
            "eval_names": [f"eval/{l}/img_{i:04d}.png" for i, l in enumerate(eval_labels)], "planted": planted}


# ---- nearest_neighbors.py ---------------------------------------------------------------------------------------------------------
def parser():
    import argparse
    ap = argparse.ArgumentParser(description="train / eval nearest neighbours in feature and pixel space (analysis_cvcl/duplicates.py)")
    ap.add_argument("--train_dir", default=None, help="class-per-folder training frames")
    ap.add_argument("--eval_dir", default=None, help="class-per-folder evaluation frames")
    ap.add_argument("--dataset", default="folders", choices=("folders", "synthetic"))
    ap.add_argument("--space", default="both", choices=("features", "pixels", "both", "hash"),
                    help="both: features and pixels; hash: the perceptual-hash duplicates")
    ap.add_argument("--random_init", action="store_true")
    ap.add_argument("--checkpoint", default=None, help="DINO checkpoint of the ResNeXt (default: $CVCL_PRETRAINED_DIR)")
    ap.add_argument("--precision", default="32", choices=("32", "32-split"))
    ap.add_argument("--batch_size", type=int, default=256)
    ap.add_argument("--chunk", type=int, default=None, help="base frames per search call (default: all at once)")
    ap.add_argument("--top_k", type=int, default=1, help="above 1: also the k closest training frames per evaluation frame "
                    "(top_k_matches.csv) and the weighted k-NN classification over them (knn_results.json)")
    ap.add_argument("--knn_temperature", type=float, default=0.07, help="T of the k-NN vote's weights exp(cos / T); 0: majority vote")
    ap.add_argument("--seed", type=int, default=0)
    ap.add_argument("--out_dir", default=os.path.join("results", "duplicates"))
    return ap


def build_encoder(args, device):
    from .utils import build_dino_mugs, load_dino_mugs, load_model
    torch.manual_seed(args.seed)
    if args.checkpoint:
        model = build_dino_mugs("resnext50_32x4d", None)
        load_dino_mugs(model, args.checkpoint, "teacher")
    else:
        model = load_model(MODEL_NAME, pretrained=not args.random_init)
    for p in model.parameters():
        p.requires_grad = False
    return model.to(device)


def main(args):
    if not torch.cuda.is_available():
        raise H.CvclError("nearest_neighbors.py needs a GPU (the searches have no CPU fallback)")
    dev = torch.device("cuda:0")
    if args.dataset == "synthetic":
        d = synthetic_sets(args.seed)
        train, train_labels, train_names = d["train"], d["train_labels"], d["train_names"]
        evalf, eval_labels, eval_names = d["eval"], d["eval_labels"], d["eval_names"]
    else:
        if not args.train_dir or not args.eval_dir:
            raise SystemExit("--train_dir and --eval_dir are required (or --dataset synthetic)")
        train, train_labels, train_names = load_folder_u8(args.train_dir)
        evalf, eval_labels, eval_names = load_folder_u8(args.eval_dir)
    train, evalf = train.to(dev), evalf.to(dev)
    os.makedirs(args.out_dir, exist_ok=True)
    print(f"Number of train frames: {len(train_labels)}\nNumber of eval frames: {len(eval_labels)}")
    if args.space in ("features", "both"):
        model = build_encoder(args, dev)
        tf = extract_features(model, train, args.batch_size, args.precision)
        ef = extract_features(model, evalf, args.batch_size, args.precision)
        np.savez(os.path.join(args.out_dir, "features.npz"), train_features=tf.cpu().numpy(), eval_features=ef.cpu().numpy())
        res = nn_classify(ef, eval_labels, tf, train_labels, eval_names, train_names, chunk=args.chunk)
        print("\n".join(classify_summary(res)))
        write_matched_results(res["rows"], os.path.join(args.out_dir, "matched_results.csv"))
        matches = same_category_matches(ef, eval_labels, tf, train_labels, eval_names, train_names, chunk=args.chunk)
        print("\n".join(matches_summary(matches)))
        with open(os.path.join(args.out_dir, "max_cosine_sims.json"), "w") as f:
            json.dump(matches, f)
        with open(os.path.join(args.out_dir, "nn_features_summary.json"), "w") as f:
            json.dump({"per_category": res["per_category"], "total": res["total"]}, f)
        if args.top_k > 1:
            knn = knn_classify(ef, eval_labels, tf, train_labels, args.top_k, args.knn_temperature, eval_names, train_names,
                               chunk=args.chunk)
            print("\n".join(knn_summary(knn)))
            write_top_k_matches(knn["rows"], os.path.join(args.out_dir, "top_k_matches.csv"))
            with open(os.path.join(args.out_dir, "knn_results.json"), "w") as f:
                json.dump({key: knn[key] for key in ("k", "temperature", "per_category", "total", "top5_total")}, f)
    if args.space in ("pixels", "both"):
        dist, idx, _ = nearest_pixels(evalf, train, chunk=args.chunk)
        recs = pixel_records(eval_names, eval_labels, train_names, train_labels, dist, idx)
        print(f"Accuracy: {sum(r['correct'] for r in recs) / len(recs)}")
        with open(os.path.join(args.out_dir, "nn_pixel_space_results.json"), "w") as f:
            json.dump(recs, f)
    if args.space == "hash":
        res = hash_duplicates(evalf, eval_labels, train, train_labels, eval_names, train_names)
        print("\n".join(hash_summary(res)))
        for name, key in (("hashed_eval_frames.json", "hashed_eval_frames"), ("hashed_train_frames.json", "hashed_train_frames"),
                          ("indirect_duplicates.json", "indirect_duplicates"), ("hash_duplicates.json", "hamming_duplicates")):
            with open(os.path.join(args.out_dir, name), "w") as f:
                json.dump(res[key], f)
