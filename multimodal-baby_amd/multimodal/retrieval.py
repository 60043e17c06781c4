"""Image-text retrieval evaluation of the joint embedding on the HIP path: for every frame, how far down the list of all utterances
sorted by cosine its own stands, and the reverse -- Recall@K, median / mean rank, MRR.  The reference has no retrieval code; the
protocol is the usual one of contrastive image-text models.

``retrieval_ranks`` is two launch sequences over the base rows, neither of which writes a queries x base matrix:
``neighbors.nearest_cosine`` with the keys as groups finds each query's best positive, and ``cvcl_rank_cosine`` counts the negatives
that beat it on the same tile walk (csrc/neighbors.hip), so a pair's cosine has the same bits in both passes and ties resolve as a
stable descending sort would resolve them.  ``rank_summary`` turns the ranks into the figures on the host (one download of Nq
integers), ``image_text_retrieval`` builds the keys of both directions from the pairs' text ids."""
from __future__ import annotations

import json
import os

import numpy as np
import torch

from . import _hip as H
from . import neighbors as NB

COSINE_EPS = NB.COSINE_EPS


def retrieval_ranks(query, base, query_keys, base_keys, chunk=None, eps=COSINE_EPS):
    """query [Nq, D], base [Nb, D] fp32 device rows (a row stride above D is read in place), query_keys [Nq] / base_keys [Nb]
    integers: query i's positives are the base rows of its key, every other row is a negative -> (rank [Nq] int64 = the 0-based
    position of the query's best positive among the negatives in a stable descending sort by cosine, -1 without a positive;
    best_cos [Nq] fp32, best_idx [Nq] int64 = that positive, ``nearest_cosine``'s grouped result), all on the device.  ``chunk``:
    base rows per launch sequence; the counts add up to the one-shot ranks exactly."""
    NB._device_tensor(query, "retrieval_ranks(query)")
    NB._device_tensor(base, "retrieval_ranks(base)")
    if query_keys is None or base_keys is None:
        raise H.CvclError("retrieval_ranks: query_keys and base_keys are both required")
    best_cos, best_idx = NB.nearest_cosine(query, base, query_keys, base_keys, chunk=chunk, eps=eps)
    q, b = NB._rows_f32(query, "query"), NB._rows_f32(base, "base")
    (Nq, D), Nb = q.shape, b.shape[0]
    qk, bk = NB._group_ids(query_keys, base_keys, Nq, Nb, q.device)
    rank = torch.full((Nq,), -1, dtype=torch.int64, device=q.device)
    if Nq == 0 or Nb == 0:
        return rank, best_cos, best_idx
    lib = H.lib()
    step = Nb if chunk is None else max(1, int(chunk))
    ws = torch.empty(lib.cvcl_rank_cosine_workspace_bytes(Nq, min(step, Nb), D), dtype=torch.uint8, device=q.device)
    for s in range(0, Nb, step):
        n = min(step, Nb - s)
        H.check(lib.cvcl_rank_cosine(*H.rows(q), *H.rows(b[s:s + n]), Nq, n, D, eps, H.ptr(qk), H.ptr(bk[s:]), H.ptr(best_cos),
                                     H.ptr(best_idx), s, int(s > 0), H.ptr(rank), H.ptr(ws), ws.numel(), H.stream_ptr()),
                "cvcl_rank_cosine")
    return rank, best_cos, best_idx


def rank_summary(rank, ks=(1, 5, 10), n_candidates=None):
    """The figures of a rank vector (0-based, -1 = the query has no positive and is left out) as a dict: ``n_queries`` (ranked),
    ``n_without_positive``, ``recall@k`` = the share of ranked queries with rank < k, ``median_rank`` / ``mean_rank`` (1-based),
    ``mrr``, and with ``n_candidates`` ``chance_recall@k`` = min(1, k / n_candidates).  float64 numpy on the host; a device tensor is
    downloaded once."""
    r = rank.detach().cpu().numpy() if torch.is_tensor(rank) else np.asarray(rank)
    if r.ndim != 1 or r.dtype.kind not in "iu":
        raise ValueError(f"rank_summary: expected a 1-D integer vector, got {r.shape} {r.dtype}")
    r = r.astype(np.int64)
    ranked = r[r >= 0].astype(np.float64)
    n = int(ranked.size)
    out = {"n_queries": n, "n_without_positive": int(r.size - n)}
    for k in ks:
        out[f"recall@{int(k)}"] = float(np.mean(ranked < k)) if n else float("nan")
    out["median_rank"] = float(np.median(ranked + 1.0)) if n else float("nan")
    out["mean_rank"] = float(np.mean(ranked + 1.0)) if n else float("nan")
    out["mrr"] = float(np.mean(1.0 / (ranked + 1.0))) if n else float("nan")
    if n_candidates is not None:
        for k in ks:
            out[f"chance_recall@{int(k)}"] = min(1.0, int(k) / int(n_candidates))
    return out


def retrieval_keys(text_ids):
    """The keys of both directions from text_ids [N] (the id of pair i's token sequence; equal sequences share an id) -> (dense
    [N] int64 = the ids renumbered 0 .. T - 1 in order of first appearance, first [T] int64 = the first pair of each distinct text).
    image -> text: queries = frames with key dense[i], base = text_features[first] with key 0 .. T - 1 (a single positive);
    text -> image: queries = text_features[first] with key 0 .. T - 1, base = all frames with key dense[j] (every frame paired with
    the text is a positive)."""
    ids = np.asarray(text_ids.cpu() if torch.is_tensor(text_ids) else text_ids)
    if ids.ndim != 1 or ids.dtype.kind not in "iu":
        raise ValueError(f"text_ids: expected a 1-D integer vector, got {ids.shape} {ids.dtype}")
    _, first, inverse = np.unique(ids, return_index=True, return_inverse=True)
    order = np.argsort(first, kind="stable")             # distinct texts in order of first appearance
    renumber = np.empty(len(order), dtype=np.int64)
    renumber[order] = np.arange(len(order))
    return renumber[inverse.reshape(-1)].astype(np.int64), first[order].astype(np.int64)


def image_text_retrieval(image_features, text_features, text_ids, ks=(1, 5, 10), chunk=None):
    """Both directions of the retrieval protocol over N (frame, utterance) pairs: image_features, text_features [N, D] fp32 on the
    device, text_ids [N] integers, identical token sequences being ONE text.  ``image_to_text`` ranks each frame against the
    distinct texts (a single positive); ``text_to_image`` ranks each distinct text against all frames, every frame paired with it
    being a positive and the rank the best positive's.  Returns {"image_to_text": summary, "text_to_image": summary,
    "n_pairs", "n_texts", "ranks_image_to_text", "ranks_text_to_image" (numpy int64)}."""
    NB._device_tensor(image_features, "image_text_retrieval(image_features)")
    NB._device_tensor(text_features, "image_text_retrieval(text_features)")
    dense, first = retrieval_keys(text_ids)
    N, T = len(dense), len(first)
    if image_features.shape[0] != N or text_features.shape[0] != N:
        raise H.CvclError(f"image_text_retrieval: {image_features.shape[0]} frames, {text_features.shape[0]} texts, {N} text ids")
    texts = text_features[torch.from_numpy(first).to(text_features.device)].contiguous()
    text_keys = np.arange(T, dtype=np.int64)
    r_i2t = retrieval_ranks(image_features, texts, dense, text_keys, chunk=chunk)[0].cpu().numpy()
    r_t2i = retrieval_ranks(texts, image_features, text_keys, dense, chunk=chunk)[0].cpu().numpy()
    return {"image_to_text": rank_summary(r_i2t, ks, n_candidates=T), "text_to_image": rank_summary(r_t2i, ks, n_candidates=N),
            "n_pairs": N, "n_texts": T, "ranks_image_to_text": r_i2t, "ranks_text_to_image": r_t2i}


def require_cosine_model(model):
    """Ranks are by cosine; a model with ``normalize_features`` off orders its logits by the dot product instead, and its ranks
    would not be the ones reported here: refused."""
    mm = getattr(model, "model", model)
    if not bool(getattr(mm, "normalize_features", False)):
        raise H.CvclError("retrieval ranks are by cosine, but this model has normalize_features off: its logits are ordered by the dot "
                          "product of un-normalised features, and ranking those is not built (cosine ranks would not be the model's)")
    if getattr(mm, "embedding_type", "flat") != "flat":
        raise H.CvclError(f"retrieval needs one feature row per frame and utterance (embedding_type flat, got {mm.embedding_type})")


def text_ids_of(token_rows):
    """text_ids [N] int64 from padded token rows [N, L]: equal rows share an id (ids count the distinct rows in sorted order)"""
    rows = np.asarray(token_rows.cpu() if torch.is_tensor(token_rows) else token_rows)
    if rows.ndim != 2:
        raise ValueError(f"token rows: expected [N, L], got {rows.shape}")
    _, inverse = np.unique(rows, axis=0, return_inverse=True)
    return inverse.reshape(-1).astype(np.int64)


def embed_pairs(model, datamodule, loader, device):
    """encode_image / encode_text over a loader of (img, tokens, length, raw) pair batches, the joint-space features the logits
    use -> (image [N, E], text [N, E] fp32 on the device, token rows [N, L] padded with 0 on the host)"""
    from .alignment import ImageTower
    mm = getattr(model, "model", model)
    tower = ImageTower(mm)
    img_f, txt_f, tokens = [], [], []
    with torch.no_grad():
        for batch in loader:
            img, idxs, length = batch[0].to(device), batch[1].to(device), batch[2].to(device)
            img = datamodule.on_after_batch_transfer((img, idxs, length), training=False)[0]
            img_f.append(NB.extract_features(tower, img, batch=img.shape[0]))
            txt_f.append(mm.encode_text(idxs, length)[0].float())
            tokens.append(idxs.cpu().numpy())
    L = max(t.shape[1] for t in tokens)
    tokens = np.concatenate([np.pad(t, ((0, 0), (0, L - t.shape[1]))) for t in tokens])
    return torch.cat(img_f).contiguous(), torch.cat(txt_f).contiguous(), tokens


# ---- retrieval.py (the script) ---------------------------------------------------------------------------------------------------------
def parser():
    import argparse
    ap = argparse.ArgumentParser(description="image <-> text retrieval of a CVCL model: Recall@K, median rank, MRR")
    ap.add_argument("--checkpoint", default=None, help="a MultiModalLitModel checkpoint (.ckpt)")
    ap.add_argument("--random_init", action="store_true")
    ap.add_argument("--dataset", default=None, choices=("synthetic",), help="synthetic: no files needed; otherwise --data_dir")
    ap.add_argument("--data_dir", default=None, metavar="DIR", help="dataset root in the reference's layout (default: $CVCL_DATA_DIR)")
    ap.add_argument("--frame_store", default=None, metavar="PATH", help="a store written by tools/pack_frames.py")
    ap.add_argument("--split", required=True, choices=("val", "test"))
    ap.add_argument("--ks", type=int, nargs="+", default=[1, 5, 10])
    ap.add_argument("--precision", default="32", choices=("32", "32-split"))
    ap.add_argument("--batch_size", type=int, default=64, help="pairs per encoder pass")
    ap.add_argument("--chunk", type=int, default=None, help="base rows per search call (default: all at once)")
    ap.add_argument("--seed", type=int, default=0)
    ap.add_argument("--save_features", action="store_true", help="also features_image.npy, features_text.npy, text_ids.npy")
    ap.add_argument("--out", default=os.path.join("results", "retrieval"))
    return ap


def build_datamodule(args):
    import argparse
    from .multimodal_data_module import SyntheticDataModule, data_dir_from
    cfg = argparse.Namespace(batch_size=args.batch_size, val_batch_size=args.batch_size, num_workers=0, seed=args.seed,
                             data_dir=args.data_dir, frame_store=args.frame_store)
    if args.dataset == "synthetic":
        dm = SyntheticDataModule(cfg)
    else:
        if not data_dir_from(cfg):
            raise SystemExit("--dataset synthetic, or --data_dir DIR (or $CVCL_DATA_DIR) with a dataset in the reference's layout")
        from .multimodal_saycam_data_module import MultiModalSAYCamDataModule
        dm = MultiModalSAYCamDataModule(cfg)
    dm.prepare_data()
    dm.setup()
    return dm


def main(args):
    from .alignment import build_model
    if not torch.cuda.is_available():
        raise H.CvclError("retrieval.py needs a GPU (the searches have no CPU fallback)")
    dev = torch.device("cuda:0")
    lit = build_model(args, dev, normalize_features=True)
    require_cosine_model(lit)
    dm = build_datamodule(args)
    loader = (dm.val_dataloader() if args.split == "val" else dm.test_dataloader())[0]
    image, text, tokens = embed_pairs(lit, dm, loader, dev)
    text_ids = text_ids_of(tokens)
    res = image_text_retrieval(image, text, text_ids, tuple(args.ks), args.chunk)
    os.makedirs(args.out, exist_ok=True)
    np.save(os.path.join(args.out, "ranks_image_to_text.npy"), res["ranks_image_to_text"])
    np.save(os.path.join(args.out, "ranks_text_to_image.npy"), res["ranks_text_to_image"])
    if args.save_features:
        np.save(os.path.join(args.out, "features_image.npy"), image.cpu().numpy())
        np.save(os.path.join(args.out, "features_text.npy"), text.cpu().numpy())
        np.save(os.path.join(args.out, "text_ids.npy"), text_ids)
    record = {"image_to_text": res["image_to_text"], "text_to_image": res["text_to_image"], "split": args.split, "N": res["n_pairs"],
              "n_texts": res["n_texts"], "precision": args.precision, "checkpoint": args.checkpoint}
    with open(os.path.join(args.out, "retrieval.json"), "w") as f:
        json.dump(record, f)
    for name in ("image_to_text", "text_to_image"):
        s = res[name]
        print(f"{name}: " + ", ".join(f"R@{k} {s[f'recall@{k}']:.4f}" for k in args.ks)
              + f", median rank {s['median_rank']}, mean rank {s['mean_rank']:.2f}, MRR {s['mrr']:.4f} "
              f"({s['n_queries']} queries, {s['n_without_positive']} without a positive)")
    return record
