"""4-way forced-choice evaluation with the reference's CLI and output format (reference eval.py:27-331).

    python eval.py --checkpoint checkpoints/<exp>/epoch=0.ckpt --eval_dataset synthetic --stage test --save_predictions

Per trial the reference runs ``model(img, label, label_len)`` once (batch 1: four images vs one label for
``--eval_type image``, one image vs four labels for ``--eval_type text``), takes the soft-max of the 4 logits, the arg-max
as the prediction (target at index 0) and appends one record to ``results/<dataset>/<name>_predictions.json``
(``{"data": [{checkpoint, model, seed, shuffle_utterances, augment_frames, multiple_frames, cnn, eval_type, eval_dataset,
stage, trial_idx, categories, logits, pred, correct}, ...]}``).  Same records here; the difference is how the device is
used: ``--trial_batch T`` trials are encoded together (4T images + T labels in one pass through the HIP encoders, eval-mode
BatchNorm is per-sample so the numbers are those of the batch-1 calls) and each trial's 4 logits are read off the
block diagonal of the T x 4T logit matrix -- the batch-1 path is launch-latency bound (~0.6 ms per trial).

``--clip_eval --clip_checkpoint PATH --clip_bpe PATH`` scores the same trials with an OpenAI-layout CLIP (the reference's upper-bound
baseline, eval.py:29-45, 122-124, 205-207, 224-226, 287-288) through multimodal/clip_model.py: the weights (a TorchScript archive or
a state dict) and the tokenizer's merges file are the user's; frames get CLIP's normalisation and labels CLIP's tokenizer in the
data module.

``--eval_dataset saycam --data_dir DIR [--frame_store PATH] --eval_metadata_filename F`` scores the trials of ``DIR/F`` (a dataset
directory in the reference's layout, multimodal/multimodal_saycam_data_module.py; ``$CVCL_DATA_DIR`` stands in for ``--data_dir``).
``saycam`` without a dataset directory or under ``--clip_eval`` is not available here; ``synthetic`` uses the synthetic trials of the
data module (same item layout).

``--eval_dataset object_categories --data_dir DIR [--object_categories_dir DIR2] [--seed S]`` is the reference's out-of-distribution
evaluation (eval.py:149-160): 4-way trials over the category folders ``DIR/object_categories/<category>/*.jpg``
(multimodal/object_categories_data_module.py; ``DIR/eval_object_categories.json`` is used if present and generated from ``--seed``
otherwise), with a checkpoint or under ``--clip_eval``; without the directory the run exits.  It has one set of trials: ``--stage`` is
recorded and selects nothing.  Its trials share their frames (5 trials per image, 3 foil images each from the same folders) and
their ~64 one-word labels, so they are not encoded per trial: every distinct frame is encoded once, ``4 * --trial_batch`` frames per
pass, every category word once, and all trials are scored from an index table in one launch (multimodal/trials.py,
``cvcl_trial_scores``) with one copy to the host.  Spatial embeddings with ``sim == "max"`` and runs that write attention maps have
no table form and go through the per-trial path above over the same trials, as does any run under ``--no_trial_table``
(``--no_trial_table --trial_batch 1`` is the reference's loop)."""
import argparse
import glob
import json
import os
import sys

import numpy as np
import torch

sys.path.insert(0, os.path.join(os.path.dirname(os.path.abspath(__file__)), "multimodal-baby_amd"))

from multimodal.multimodal_data_module import (EOS_TOKEN_ID, SOS_TOKEN_ID, SyntheticDataModule, data_dir_from,   # noqa: E402
                                               load_data)
from multimodal.multimodal_saycam_data_module import MultiModalSAYCamDataModule   # noqa: E402
from multimodal.object_categories_data_module import OBJECT_CATEGORIES_DIRNAME, ObjectCategoriesDataModule   # noqa: E402
from multimodal.multimodal_lit import MultiModalLitModel                          # noqa: E402
from train import _setup_parser                                                   # noqa: E402


def config_from_checkpoint_name(name):
    """The run attributes the reference recovers from the checkpoint's directory name (eval.py:61-100)."""
    cfg = {"model": next((m for m in ("lstm", "transformer", "embedding") if m in name), None)}
    cfg["seed"] = next((i for i in (0, 1, 2) if f"seed_{i}" in name), None)
    cfg["shuffle_utterances"] = "shuffle_utterances" in name
    if "pretrained_cnn_True_finetune_cnn_True" in name:
        cfg["cnn"] = "finetune_pretrained"
    elif "pretrained_cnn_False_finetune_cnn_True" in name:
        cfg["cnn"] = "finetune_random_init"
    elif "pretrained_cnn_False_finetune_cnn_False" in name:
        cfg["cnn"] = "frozen_random_init"
    else:
        cfg["cnn"] = "frozen_pretrained"
    cfg["augment_frames"] = "augment_frames_False" not in name
    cfg["multiple_frames"] = "multiple_frames_False" not in name
    return cfg


def resolve_checkpoint(name, root="checkpoints"):
    """A .ckpt path is used as is; a run name resolves to its last.ckpt (shuffled-utterance runs) or its epoch*.ckpt
    (the best-val-loss checkpoint ModelCheckpoint kept), as eval.py:50-58 does under the reference's checkpoint root."""
    if name.endswith(".ckpt"):
        return name
    if "shuffle_utterances_True" in name:
        return os.path.join(root, name, "last.ckpt")
    found = sorted(glob.glob(os.path.join(root, name, "epoch*.ckpt")))
    if not found:
        raise FileNotFoundError(f"no epoch*.ckpt under {os.path.join(root, name)}")
    return found[0]


def results_filename(args, cfg):
    """eval.py:293-310."""
    d, m, c, s = args.eval_dataset, cfg["model"], cfg["cnn"], cfg["seed"]
    tail = f"{args.eval_type}_{d}_{args.stage}"
    if args.eval_metadata_filename == "eval_filtered_test.json":
        return f"results/{d}/{m}_{c}_seed_{s}_{tail}_eval_filtered_predictions.json"
    if args.eval_metadata_filename == "eval_manual_filtered_test.json":
        return f"results/{d}/{m}_{c}_seed_{s}_{tail}_eval_manual_filtered_predictions.json"
    if cfg["shuffle_utterances"]:
        return f"results/{d}/shuffle_{m}_{c}_seed_{s}_{tail}_eval_predictions.json"
    if not cfg["augment_frames"]:
        return f"results/{d}/{m}_{c}_augment_frames_{cfg['augment_frames']}_seed_{s}_{tail}_eval_predictions.json"
    if not cfg["multiple_frames"]:
        return f"results/{d}/{m}_{c}_multiple_frames_{cfg['multiple_frames']}_seed_{s}_{tail}_eval_predictions.json"
    return f"results/{d}/{m}_{c}_seed_{s}_{tail}_eval_predictions.json"


@torch.no_grad()
def evaluate_trials(model, trials, eval_type, device, datamodule=None, attention_maps=False, rollout=False, clip=False,
                    discard_ratio=0.0):
    """trials: list of collated batch-1 items (img, label, label_len, raw_label).  Returns per trial (soft-max list, pred).
    All trials of the list are encoded in one pass; trial t's logits are the t-th diagonal block.
    ``attention_maps``: returns (per-trial results, Grad-CAM maps [T, 4, h, w]) -- per trial the maps of its 4 images w.r.t. its
    label (``image``) or of its image w.r.t. its 4 labels (``text``), from the same encoder pass as the logits.  A ViT encoder has
    no Grad-CAM: its maps are the CLS token's last-block self-attention [T, 4, gh, gw], which do not depend on the label (``text``:
    the one image's map repeated 4 times, so the array keeps its shape); with ``rollout`` they are the CLS token's attention rollout
    over all blocks instead, same shape; a non-zero ``discard_ratio`` zeroes that share of every block's weakest attentions before
    the chain (attention_maps.vit_attention_rollout_discard).
    ``clip``: the labels are CLIP token rows ([1, 1, 77] / [1, 4, 77] per trial, reference eval.py:205-207, 224-226): stacked to
    [T, 77] / [4T, 77] and scored by ``model(imgs, tokens)``."""
    T = len(trials)
    if clip:
        imgs = torch.cat([t[0].squeeze(0) for t in trials], 0).to(device)
        n_per = trials[0][0].shape[1] if eval_type == "image" else trials[0][1].shape[1]
        tokens = torch.cat([t[1].squeeze(0) for t in trials], 0).to(device)
    elif eval_type == "image":
        imgs = torch.cat([t[0].squeeze(0) for t in trials], 0).to(device)                    # [4T, ...]
        n_per = trials[0][0].shape[1]
        L = max(t[1].shape[1] for t in trials)
        labels = torch.zeros(T, L, dtype=torch.long)
        for i, t in enumerate(trials):
            labels[i, : t[1].shape[1]] = t[1][0]
        lens = torch.cat([t[2].reshape(1) for t in trials]).long()
    else:
        imgs = torch.cat([t[0].squeeze(0) for t in trials], 0).to(device)                    # [T, ...]
        n_per = trials[0][1].shape[1]
        L = max(t[1].shape[2] for t in trials)
        labels = torch.zeros(T * n_per, L, dtype=torch.long)
        for i, t in enumerate(trials):
            labels[i * n_per:(i + 1) * n_per, : t[1].shape[2]] = t[1][0]
        lens = torch.cat([t[2].reshape(-1) for t in trials]).long()
    if imgs.dtype in (torch.uint8, torch.int64) and datamodule is not None:      # --device_frames / --frame_store: base transform on the GPU
        imgs = datamodule.on_after_batch_transfer((imgs,), 1, training=False)[0]
    maps = None
    if clip:
        logits_per_image, logits_per_text = model(imgs, tokens)
    elif attention_maps and getattr(getattr(model, "vision_encoder", None), "vit_dino", False):
        if rollout and discard_ratio:
            from multimodal.attention_maps import vit_attention_rollout_discard
            maps = vit_attention_rollout_discard(model.vision_encoder, imgs, discard_ratio)
            logits_per_image, logits_per_text = model(imgs, labels.to(device), lens.to(device))
        else:
            logits_per_image, logits_per_text, maps = model.self_attention_maps(imgs, labels.to(device), lens.to(device), rollout=rollout)
        if eval_type == "image":                          # [4T, gh, gw] -> [T, 4, gh, gw]
            maps = maps.view(T, n_per, *maps.shape[1:])
        else:                                             # one image per trial: its map along the 4 axis
            maps = maps[:, None].expand(T, n_per, *maps.shape[1:]).contiguous()
    elif attention_maps:                                  # label t with images 4t .. 4t + 3, or image t with labels 4t .. 4t + 3
        pairs = ("block", n_per, "text" if eval_type == "image" else "image")
        logits_per_image, logits_per_text, maps = model.attention_maps(imgs, labels.to(device), lens.to(device), pairs=pairs)
    else:
        logits_per_image, logits_per_text = model(imgs, labels.to(device), lens.to(device))
    out = []
    for i in range(T):
        if eval_type == "image":
            row = logits_per_text[i, i * n_per:(i + 1) * n_per]
        else:
            row = logits_per_image[i, i * n_per:(i + 1) * n_per]
        out.append((torch.softmax(row.float(), dim=-1).cpu().numpy().tolist(), int(torch.argmax(row))))
    return (out, maps) if attention_maps else out


def plot_attention(path, image, cam):
    """One overlay PNG (reference eval_shuffled.py:195-228): the frame with its Grad-CAM (ViT: self-attention) map blended in."""
    try:
        import matplotlib
        matplotlib.use("Agg")
        import matplotlib.pyplot as plt
    except ImportError as e:
        raise SystemExit(f"--plot_attention needs matplotlib ({e})")
    from multimodal.attention_maps import bicubic_resize, getAttMap, imshow, n_inv
    att = bicubic_resize(cam[None], image.shape[1:])[0].cpu().numpy()
    img = n_inv(image.float().cpu()).permute(1, 2, 0).clamp(0, 1).numpy()
    fig, ax = plt.subplots()
    imshow(ax, getAttMap(img, att))
    plt.savefig(path, bbox_inches="tight")
    plt.close(fig)


def write_attention_overlays(paths, frames, cams):
    """--attention_overlays: the PNGs --plot_attention names, without matplotlib -- ``frames`` [T, 3, H, W] normalised device frames
    with ``cams`` [T, h, w], rendered in one batch on the device (attention_maps.overlay_attention_maps: bicubic resize, scipy's
    gaussian blur, min-max normalisation, viridis, the attn ** 0.7 blend of getAttMap) and written at the frames' own size with PIL."""
    try:
        from PIL import Image
    except ImportError as e:
        raise SystemExit(f"--attention_overlays needs Pillow ({e})")
    from multimodal.attention_maps import overlay_attention_maps
    tiles = overlay_attention_maps(frames.float(), cams).cpu().numpy()             # uint8 [T, H, W, 3]
    for path, tile in zip(paths, tiles):
        Image.fromarray(tile).save(path)


CLIP_CONFIG = {"model": "clip", "seed": None, "shuffle_utterances": None, "cnn": "clip", "augment_frames": None,
               "multiple_frames": None}                    # the run attributes of a --clip_eval record (eval.py:39-47)


def clip_results_filename(args):
    """eval.py:287-288."""
    return f"results/{args.eval_dataset}/clip_{args.eval_type}_{args.eval_dataset}_{args.stage}_eval_predictions.json"


def check_clip_args(args):
    """What --clip_eval needs and what it does not combine with, before anything is loaded."""
    if not (args.clip_checkpoint and args.clip_bpe):
        raise SystemExit("--clip_eval needs --clip_checkpoint PATH (OpenAI CLIP weights: a TorchScript archive such as ViT-L-14.pt, or a "
                         "state_dict file) and --clip_bpe PATH (CLIP's bpe_simple_vocab_16e6.txt or .txt.gz); neither is shipped or fetched")
    for flag, on in (("--attention_maps", args.attention_maps), ("--plot_attention", args.plot_attention),
                     ("--attention_overlays", getattr(args, "attention_overlays", False)),
                     ("--attention_rollout", args.attention_rollout), ("--hip_graph", args.hip_graph)):
        if on:
            raise SystemExit(f"{flag} is not built for --clip_eval (CLIP attention maps and graph replay of the CLIP towers are out of scope)")
    if args.precision not in ("32", "bf16"):
        raise SystemExit(f"--clip_eval runs in --precision 32 or bf16, not {args.precision}")


def object_categories_dir(args):
    """--object_categories_dir, else object_categories/ under the dataset root, else None"""
    if args.object_categories_dir:
        return args.object_categories_dir
    root = data_dir_from(args)
    return os.path.join(root, OBJECT_CATEGORIES_DIRNAME) if root else None


def main(args):
    if not 0 <= args.rollout_discard_ratio < 1:            # (false for nan)
        raise SystemExit(f"--rollout_discard_ratio {args.rollout_discard_ratio}: a share R of the attentions with 0 <= R < 1")
    if args.rollout_discard_ratio and not args.attention_rollout:
        raise SystemExit("--rollout_discard_ratio R thins the blocks' attentions of --attention_rollout; give that flag as well")
    if args.clip_eval:
        check_clip_args(args)
    saycam = args.eval_dataset == "saycam" and not args.clip_eval and bool(data_dir_from(args))
    objcat = args.eval_dataset == "object_categories" and os.path.isdir(object_categories_dir(args) or "")
    if args.eval_dataset != "synthetic" and not saycam and not objcat:
        raise SystemExit(f"--eval_dataset {args.eval_dataset} reads the reference's private evaluation frames from hard-coded "
                         "cluster paths and is not available here; use --eval_dataset synthetic"
                         + (", or give --eval_dataset saycam a dataset directory in the reference's layout with --data_dir DIR (or "
                            "$CVCL_DATA_DIR; not under --clip_eval)" if args.eval_dataset == "saycam" else "")
                         + (", or give --eval_dataset object_categories the category folders: DIR/object_categories/<category>/*.jpg "
                            "with --data_dir DIR (or $CVCL_DATA_DIR), or --object_categories_dir DIR"
                            if args.eval_dataset == "object_categories" else ""))
    device = torch.device("cuda:0")
    data_args = _setup_parser().parse_args("")
    if args.clip_eval:                                     # eval.py:29-47
        from multimodal import clip_model
        checkpoint_name = "clip_vitl_14"
        model, _ = clip_model.load(args.clip_checkpoint, device)
        model.set_precision(args.precision)
        cfg = dict(CLIP_CONFIG)
        data_args.clip_eval, data_args.clip_bpe = True, args.clip_bpe      # CLIP's frame statistics and tokenizer (eval.py:122-124)
    else:
        checkpoint_name = args.checkpoint
        checkpoint = resolve_checkpoint(checkpoint_name, args.checkpoints_root)
        cfg = config_from_checkpoint_name(checkpoint_name)
        model = MultiModalLitModel.load_from_checkpoint(checkpoint, map_location=device)
        model.to(device)
        model.eval()
        if args.precision != "32":                         # (32: the exact-fp32 mode a loaded model starts in)
            model.set_precision(args.precision)
        if args.hip_graph:                                 # replay the image encoder's launches as a HIP graph per batch shape
            model.vision_encoder.enable_hip_graphs(True)
        for key, value in model.args.items():
            setattr(data_args, key, value)
    data_args.augment_frames = False                       # deterministic frames (eval.py:115)
    data_args.eval_include_sos_eos = args.eval_include_sos_eos
    data_args.eval_type = args.eval_type
    data_args.eval_metadata_filename = args.eval_metadata_filename
    data_args.n_eval_trials = args.n_trials
    if objcat:
        # where the data is and what seeds a generated metadata file are this run's, not the checkpoint's training run's
        data_args.data_dir, data_args.object_categories_dir, data_args.seed = data_dir_from(args), args.object_categories_dir, args.seed
        data = ObjectCategoriesDataModule(data_args)
    elif saycam:
        # where the data is and how its frames travel are this run's, not the checkpoint's training run's
        data_args.data_dir, data_args.frame_store = data_dir_from(args), args.frame_store
        data_args.device_frames = bool(getattr(data_args, "device_frames", False)) and not args.frame_store
        data = MultiModalSAYCamDataModule(data_args)
    else:
        data = SyntheticDataModule(data_args)
    data.prepare_data()
    data.setup()
    if objcat:                                             # eval.py:149-160: one set of trials, whatever --stage
        dataloader = data.test_dataloader()
    else:
        loaders = {"dev": data.val_dataloader, "test": data.test_dataloader}[args.stage]()
        dataloader = loaders[1]                            # the second dataloader holds the evaluation trials
    if objcat:
        vocab = data.vocab
        eval_data = data.data
    elif saycam:                                           # eval.py:134-148 (the classes are the metadata's targets: no directory listing)
        vocab = data.read_vocab()
        eval_data = load_data(os.path.join(data.data_dir, data_args.eval_metadata_filename))
    else:
        vocab = None
        eval_data = data.eval_sets["val" if args.stage == "dev" else "test"].metadata()
    classes = sorted({t["target_category"] for t in eval_data})
    if objcat:                                             # eval.py:159: the module's category list (and whatever else the metadata scores)
        classes = list(data.object_categories) + [c for c in classes if c not in data.object_categories]
    # eval.py:162-165, 181-194: "cat" trials are scored with the word "kitty"
    kitty = bool((saycam or (objcat and not args.clip_eval)) and args.use_kitty_label)
    if kitty and "cat" in classes:
        classes.remove("cat")
        classes.append("kitty")
    correct_pred = {c: 0 for c in classes}
    total_pred = {c: 0 for c in classes}

    if args.attention_rollout and not getattr(model.vision_encoder, "vit_dino", False):        # (never under --clip_eval)
        raise SystemExit("--attention_rollout is defined for a ViT checkpoint (--vit_dino) only: a ResNeXt encoder has no "
                         "self-attention to roll out; its --attention_maps are Grad-CAM maps")
    if args.attention_rollout and not (args.attention_maps or args.plot_attention or args.attention_overlays):
        raise SystemExit("--attention_rollout selects the kind of map --attention_maps DIR / --plot_attention write; give one of them")

    results, pending, first = [], [], 0
    want_maps = bool(args.attention_maps or args.plot_attention or args.attention_overlays)
    cams = []
    if args.plot_attention or args.attention_overlays:
        os.makedirs(args.attention_maps or "results", exist_ok=True)

    def record(i, class_label, logits_list, pred):
        """trial i's record and its count; -> the class it was counted under"""
        if kitty and class_label == "cat":
            class_label = "kitty"
        correct = pred == 0                                # the target is always at index 0
        correct_pred[class_label] += int(correct)
        total_pred[class_label] += 1
        trial = eval_data[i]
        results.append({
            "checkpoint": checkpoint_name, "model": cfg["model"], "seed": cfg["seed"],
            "shuffle_utterances": cfg["shuffle_utterances"], "augment_frames": cfg["augment_frames"],
            "multiple_frames": cfg["multiple_frames"], "cnn": cfg["cnn"], "eval_type": args.eval_type,
            "eval_dataset": args.eval_dataset, "stage": args.stage, "trial_idx": i,
            "categories": [trial["target_category"]] + trial["foil_categories"],
            "logits": logits_list, "pred": pred, "correct": bool(correct)})
        return class_label

    def flush():
        nonlocal first
        res = evaluate_trials(model, pending, args.eval_type, device, data, attention_maps=want_maps, rollout=args.attention_rollout,
                              clip=args.clip_eval, discard_ratio=args.rollout_discard_ratio)
        if want_maps:
            res, maps = res
            cams.append(maps.cpu())
        overlay_paths, overlay_frames = [], []
        for k, (logits_list, pred) in enumerate(res):
            i = first + k
            class_label = record(i, pending[k][3][0][0], logits_list, pred)
            if args.plot_attention or args.attention_overlays:     # the target (index 0): its frame and its map w.r.t. the label
                frames = pending[k][0].squeeze(0).to(device)
                if frames.dtype in (torch.uint8, torch.int64):
                    frames = data.on_after_batch_transfer((frames,), 1, training=False)[0]
                name = f"{cfg['model']}_{class_label}_{i % 100}_attn_map.png"
                if args.plot_attention:
                    plot_attention(os.path.join(args.attention_maps or "results", name), frames[0], maps[k, 0])
                else:                                      # rendered below, the whole pending batch in one device pass
                    overlay_paths.append(os.path.join(args.attention_maps or "results", name))
                    overlay_frames.append(frames[0])
        if overlay_paths:
            write_attention_overlays(overlay_paths, torch.stack(overlay_frames), maps[:len(overlay_paths), 0].contiguous())
        first += len(pending)
        pending.clear()

    # object categories: frames and words encoded once, all trials scored from an index table in one launch (multimodal/trials.py)
    # -- unless the model has no table form (sim == "max"), maps are asked for (they come from the per-trial encoder pass), or the
    # run says --no_trial_table
    use_table = False
    if objcat and not args.no_trial_table and not want_maps:
        from multimodal import trials as trial_table
        use_table = trial_table.table_route(model) is None
    if use_table:
        res = trial_table.evaluate_trial_table(model, data, args.eval_type, kitty, frame_batch=4 * max(args.trial_batch, 1))
        for i, (logits_list, pred) in enumerate(res):
            record(i, eval_data[i]["target_category"], logits_list, pred)
        dataloader = ()

    for batch in dataloader:
        if kitty and batch[3][0][0] == "cat":
            img, label, label_len, raw = batch
            if args.eval_type == "image":                  # replace the single label
                ids = [vocab["kitty"]]
                ids = [SOS_TOKEN_ID] + ids + [EOS_TOKEN_ID] if args.eval_include_sos_eos else ids
                label, label_len = torch.LongTensor([ids]), torch.tensor([len(ids)])
            else:                                          # replace the true class's word only
                label = label.clone()
                label[0, 0, 1 if args.eval_include_sos_eos else 0] = vocab["kitty"]
            batch = (img, label, label_len, raw)
        pending.append(batch)
        if len(pending) == max(args.trial_batch, 1):
            flush()
    if pending:
        flush()

    for classname, correct_count in correct_pred.items():
        if objcat and not total_pred[classname]:           # a category folder that an existing metadata file leaves out
            continue
        print(f"Accuracy for class {classname:8s} is: {float(correct_count) / total_pred[classname]:.1%}")
    print(f"Total accuracy: {sum(correct_pred.values()) / sum(total_pred.values()):%}")

    if args.attention_maps:
        os.makedirs(args.attention_maps, exist_ok=True)
        out = os.path.join(args.attention_maps, "cams.npy")
        print(f"Saving attention maps to {out}")
        np.save(out, torch.cat(cams, 0).numpy())

    if args.save_predictions:
        filename = clip_results_filename(args) if args.clip_eval else results_filename(args, cfg)
        os.makedirs(os.path.dirname(filename), exist_ok=True)
        print(f"Saving predictions to {filename}")
        with open(filename, "w") as f:
            json.dump({"data": results}, f)
    return results


def _parser():
    parser = argparse.ArgumentParser()
    parser.add_argument("--checkpoint", type=str, help="path to checkpoint to use for evaluation")
    parser.add_argument("--clip_eval", action="store_true", help="Use CLIP model for evaluation")
    parser.add_argument("--stage", type=str, default="test", choices=["dev", "test"],
                        help="which evaluation stage to use (object_categories has one set of trials: recorded, selects nothing)")
    parser.add_argument("--eval_include_sos_eos", action="store_true", help="include SOS/EOS tokens for eval labels")
    parser.add_argument("--eval_type", type=str, default="image", choices=["image", "text"],
                        help="Run evaluation using multiple images or multiple labels")
    parser.add_argument("--eval_dataset", type=str, default="saycam", choices=["saycam", "object_categories", "synthetic"],
                        help="Which evaluation dataset to use")
    parser.add_argument("--eval_metadata_filename", type=str, default="eval_test.json",
                        help="JSON file with metadata evaluation split to use")
    parser.add_argument("--use_kitty_label", action="store_true", help="replaces cat label with kitty (ignored under --clip_eval)")
    parser.add_argument("--save_predictions", action="store_true", help="save model predictions to JSON")
    # additions of this implementation
    parser.add_argument("--data_dir", type=str, default=None, metavar="DIR",
                        help="--eval_dataset saycam / object_categories: the dataset root in the reference's layout (default: "
                             "$CVCL_DATA_DIR)")
    parser.add_argument("--object_categories_dir", type=str, default=None, metavar="DIR",
                        help="--eval_dataset object_categories: the folder of <category>/*.jpg folders (default: "
                             "object_categories/ under --data_dir; without --data_dir the metadata file sits beside DIR)")
    parser.add_argument("--seed", type=int, default=0,
                        help="--eval_dataset object_categories: seeds the draws of a GENERATED eval_object_categories.json (an "
                             "existing file is used as it is)")
    parser.add_argument("--no_trial_table", action="store_true",
                        help="--eval_dataset object_categories: encode every trial's 4 frames and its label(s) per trial, "
                             "--trial_batch trials a pass, instead of every distinct frame and word once and one scoring launch "
                             "(with --trial_batch 1: the reference's loop)")
    parser.add_argument("--frame_store", type=str, default=None, metavar="PATH",
                        help="--eval_dataset saycam: a store written by tools/pack_frames.py (it must hold the frames of the trials); "
                             "the trials travel as frame indices")
    parser.add_argument("--clip_checkpoint", type=str, default=None, metavar="PATH",
                        help="--clip_eval: OpenAI CLIP weights (TorchScript archive, e.g. ViT-L-14.pt, or a state_dict file); not shipped")
    parser.add_argument("--clip_bpe", type=str, default=None, metavar="PATH",
                        help="--clip_eval: CLIP's BPE merges file bpe_simple_vocab_16e6.txt(.gz); not shipped")
    parser.add_argument("--trial_batch", type=int, default=64,
                        help="trials encoded per device pass (1 = the reference's loop); object_categories from its trial table: "
                             "4 * T distinct frames per encoder pass")
    parser.add_argument("--hip_graph", action="store_true", help="capture the eval-mode image encoder into a HIP graph per batch "
                                                                  "shape and replay it (removes the host's launch lead; same results)")
    parser.add_argument("--precision", type=str, default="32", choices=["32", "bf16", "32-split"],
                        help="image/text encoder arithmetic: exact fp32 (default), bf16, or fp32 storage with split-bf16 trunk products")
    parser.add_argument("--checkpoints_root", type=str, default="checkpoints", help="where run names resolve to checkpoints")
    parser.add_argument("--n_trials", type=int, default=32, help="number of synthetic trials")
    parser.add_argument("--attention_maps", type=str, default=None, metavar="DIR",
                        help="write the Grad-CAM maps of every trial (layer 4, same pass as the logits) to DIR/cams.npy "
                             "[n_trials, 4, h, w]: the trial's 4 images w.r.t. its label (image) or its image w.r.t. its 4 labels (text). "
                             "With a ViT checkpoint (--vit_dino) the maps are the CLS token's last-block self-attention over the patch "
                             "grid, averaged over the heads, [n_trials, 4, gh, gw]: unlike Grad-CAM they do not depend on the label "
                             "(--eval_type text: the trial's one map repeated 4 times)")
    parser.add_argument("--plot_attention", action="store_true",
                        help="save one overlay PNG per trial, {model}_{class}_{i %% 100}_attn_map.png, under the --attention_maps "
                             "directory (results/ without it); needs matplotlib")
    parser.add_argument("--attention_overlays", action="store_true",
                        help="the PNGs of --plot_attention without matplotlib: every pending batch of trials is rendered in one pass on "
                             "the device (resize, blur, normalisation, viridis, blend) and written with Pillow at the frames' own size; "
                             "with --plot_attention as well, that flag's matplotlib figures are written")
    parser.add_argument("--attention_rollout", action="store_true",
                        help="ViT checkpoints: the maps of --attention_maps / --plot_attention are the CLS token's attention rollout "
                             "over all blocks (head-mean attention plus the residual path, multiplied through the blocks) instead of "
                             "the last block's CLS row; same shape [n_trials, 4, gh, gw].  An error with a ResNeXt checkpoint")
    parser.add_argument("--rollout_discard_ratio", type=float, default=0.0, metavar="R",
                        help="with --attention_rollout: before the blocks are multiplied, set the share R (0 <= R < 1; vit-explain "
                             "plots 0.9) of the weakest attentions of every block and image to zero, which keeps the maps of a deep "
                             "ViT from coming out near uniform; 0 (default): the plain rollout")
    return parser


if __name__ == "__main__":
    main(_parser().parse_args())
