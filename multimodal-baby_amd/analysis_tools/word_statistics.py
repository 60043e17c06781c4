"""``word_statistics.py``: per-word loss / perplexity tables, mean hidden vectors and next-word predictions of a language model
over a data split (analysis_tools.processing on the HIP path).

    python word_statistics.py --random_init --dataset synthetic --split val --out results/word_statistics

Writes into --out: ``token_items.csv`` (token, pos, cnt, mean_loss, ppl; one row per word under its majority tag, sorted by token id),
``token_vectors.npy`` (the words' mean hidden vectors, in the row order of the csv), ``losses.npy`` (per utterance its token losses,
zero-padded to the longest) and ``top_predictions.csv`` (per tagged position: utterance, position, token, pos, label_prob and the
top_k predicted words with their probabilities).

``--ngram N [--ngram_alpha 0.1]`` sets the reference's baseline beside them: a back-off N-gram model (ngram.NGramModel) counted on
the TRAIN split of the same data module and run over --split, written as ``ngram_token_items.csv`` (the columns of
token_items.csv), ``ngram_losses.npy`` and ``ngram_top_predictions.csv`` (its "probabilities" are back-off scores, not normalised
over the words).  Without --ngram the outputs are the four files above and nothing else."""
import argparse
import csv
import json
import os

import numpy as np
import torch

from multimodal import _hip as H

from . import processing as P

DEFAULT_TAG = "X"


def parser():
    ap = argparse.ArgumentParser(description="per-word language-model statistics (analysis_tools/processing.py)")
    ap.add_argument("--checkpoint", default=None, help="a MultiModalLitModel checkpoint (.ckpt) with an LSTM language model")
    ap.add_argument("--random_init", action="store_true")
    ap.add_argument("--dataset", default="synthetic", choices=("synthetic",))
    ap.add_argument("--split", default="val", choices=("val", "test"))
    ap.add_argument("--pos_tags", default=None, help="JSON: per utterance the list of its tokens' tags (<sos> and <eos> included); "
                                                     f"without it every position is tagged {DEFAULT_TAG}")
    ap.add_argument("--top_k", type=int, default=5)
    ap.add_argument("--batch_size", type=int, default=64)
    ap.add_argument("--seed", type=int, default=0)
    ap.add_argument("--ngram", type=int, default=0, metavar="N", help="also run a back-off N-gram baseline counted on the train split")
    ap.add_argument("--ngram_alpha", type=float, default=0.1, help="the share of probability the n-gram leaves to the lower orders")
    ap.add_argument("--out", default=os.path.join("results", "word_statistics"))
    return ap


def build_model(args, device):
    """a checkpoint, or the reference's LSTM language-model configuration (E = H = 512, tied output layer) at random weights"""
    from multimodal.multimodal import TextEncoder, VisionEncoder
    from multimodal.multimodal_data_module import read_vocab
    from multimodal.multimodal_lit import MultiModalLitModel
    torch.manual_seed(args.seed)
    if args.checkpoint:
        lit = MultiModalLitModel.load_from_checkpoint(args.checkpoint, map_location=device)
    elif args.random_init:
        cfg = argparse.Namespace(
            embedding_type="flat", embedding_dim=512, pretrained_cnn=False, cnn_model="resnext50_32x4d", cnn_dino=False, vit_dino=False,
            finetune_cnn=False, text_encoder="lstm", captioning=False, attention=False, attention_gate=False, crange=1,
            dropout_i=0.5, dropout_o=0.0, pos_embed_type="no_pos_embed", normalize_features=False, sim="max", temperature=0.07,
            fix_temperature=True, tie=True, bias=True, lr=1e-4, weight_decay=0.1, lambda_mm=0.0, lambda_lm=1.0, lambda_ar=0.0,
            optimize_unused=True, lr_scheduler=True, optimizer=torch.optim.AdamW)
        lit = MultiModalLitModel(VisionEncoder(cfg), TextEncoder(read_vocab(), 2048, cfg), cfg)
    else:
        raise SystemExit("--checkpoint PATH or --random_init")
    lit.to(device).eval()
    for p in lit.parameters():
        p.requires_grad = False
    return lit


def data_module(args):
    from multimodal.multimodal_data_module import SyntheticDataModule
    data = SyntheticDataModule(argparse.Namespace(batch_size=args.batch_size, val_batch_size=args.batch_size, num_workers=0,
                                                  seed=args.seed))
    data.setup()
    return data


def split_batches(args):
    data = data_module(args)
    loader = (data.val_dataloader() if args.split == "val" else data.test_dataloader())[0]       # the pair batches, not the trials
    return list(loader)


def write_results(out_dir, items, predictions, idx2word, top_k, prefix="", with_vectors=True):
    os.makedirs(out_dir, exist_ok=True)
    with open(os.path.join(out_dir, prefix + "token_items.csv"), "w", newline="") as f:
        wr = csv.writer(f)
        wr.writerow(["token", "pos", "cnt", "mean_loss", "ppl"])
        for key, value in items.token_items.items():
            wr.writerow([idx2word[key.token_id], key.pos, int(value.cnt), repr(float(value.mean_loss)), repr(float(value.ppl))])
    if with_vectors:
        vectors = [value.mean_vector for value in items.token_items.values()]
        np.save(os.path.join(out_dir, prefix + "token_vectors.npy"), np.stack(vectors) if vectors else np.zeros((0, 0), dtype=np.float32))
    losses = np.zeros((len(items.losses), max((len(l) for l in items.losses), default=0)), dtype=np.float32)
    for r, l in enumerate(items.losses):
        losses[r, :len(l)] = l
    np.save(os.path.join(out_dir, prefix + "losses.npy"), losses)
    with open(os.path.join(out_dir, prefix + "top_predictions.csv"), "w", newline="") as f:
        wr = csv.writer(f)
        wr.writerow(["utterance", "position", "token", "pos", "label_prob"] +
                    [c for j in range(top_k) for c in (f"top{j + 1}", f"top{j + 1}_prob")])
        for u, l, key, label_prob, top_prob, top_idx in predictions:
            wr.writerow([u, l, idx2word[key.token_id], key.pos, repr(float(label_prob))] +
                        [c for p, i in zip(top_prob, top_idx) for c in (idx2word[int(i)], repr(float(p)))])


def main(args):
    if not torch.cuda.is_available():
        raise H.CvclError("word_statistics.py needs a GPU (the analysis has no CPU fallback)")
    dev = torch.device("cuda:0")
    batches = split_batches(args)
    if args.pos_tags:
        with open(args.pos_tags) as f:
            pos_tags = json.load(f)
    else:
        pos_tags = [[DEFAULT_TAG] * int(n) for batch in batches for n in batch[2]]
    lit = build_model(args, dev)
    items = P.get_model_items(lit, batches, pos_tags)
    top = list(P.iter_top_predictions(lit, batches, pos_tags, top_k=args.top_k))
    idx2word = lit.text_encoder.idx2word
    write_results(args.out, items, top, idx2word, args.top_k)
    n_tok = sum(int(v.cnt) for v in items.token_items.values())
    print(f"{len(items.losses)} utterances, {n_tok} tagged positions, {len(items.token_pos_items)} (word, tag) keys, "
          f"{len(items.token_items)} words -> {args.out}")
    if args.ngram:
        baseline = P.build_ngram_model(args.ngram, len(idx2word), data_module(args).train_dataloader(), device=dev)
        baseline.alpha = args.ngram_alpha
        ngram_items = P.get_model_items(baseline, batches, pos_tags)
        ngram_top = list(P.iter_top_predictions(baseline, batches, pos_tags, top_k=args.top_k))
        write_results(args.out, ngram_items, ngram_top, idx2word, args.top_k, prefix="ngram_", with_vectors=False)
        n_tok = sum(len(l) - 1 for l in ngram_items.losses if len(l))
        mean = sum(float(l.sum()) for l in ngram_items.losses) / max(n_tok, 1)
        print(f"{args.ngram}-gram baseline (alpha {args.ngram_alpha}): mean token loss {mean:.4f} over {n_tok} tokens -> {args.out}")
    return items
