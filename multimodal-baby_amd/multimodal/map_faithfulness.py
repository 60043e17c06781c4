"""Deletion / insertion faithfulness of attention maps on the HIP path (Petsiuk et al., RISE, 2018): does a map point at what the
image-text score depends on?  The pixels a map ranks highest are removed from the frame a slice at a time (deletion, towards a
baseline frame) or restored into a baseline frame (insertion), the frame is re-encoded after every slice, and the areas under the two
score curves are the figures: a faithful map has a LOW deletion AUC and a HIGH insertion AUC.  No masks or boxes are needed, and the
measure is the same for every map kind the project produces (Grad-CAM, the ViT's CLS attention, rollout with and without
discard_ratio) and for a random map, the chance control.  The reference has no such code.

Device side (csrc/faithfulness.hip): ``pixel_ranks`` (cvcl_map_ranks: an exact stable sort per map), ``perturb`` (cvcl_map_perturb: a
pure select), ``gaussian_blur`` (the blurred insertion baseline), ``pair_dot`` and ``curve_auc``.  ``deletion_insertion`` strings them
around ``model.encode_image``; ``maps_of`` calls the existing map producers; ``parser`` / ``main`` are attention_faithfulness.py."""
from __future__ import annotations

import json
import os
import sys

import numpy as np
import torch

from . import _hip as H

MAP_KINDS = ("gradcam", "cls_attention", "rollout", "rollout_discard", "random")
ROLLOUT_DISCARD_RATIO = 0.9                               # the ratio people plot (attention_maps.vit_attention_rollout_discard)
MAX_PIXELS = 65536                                        # cvcl_map_ranks: pixel indices travel as 16 bits


def _device(t, what):
    if not torch.is_tensor(t) or not t.is_cuda:
        raise H.CvclError(f"{what} needs device tensors (got {'a CPU tensor' if torch.is_tensor(t) else type(t).__name__}); "
                          "there is no CPU fallback")


def _host_i32(v, n, what):
    a = np.ascontiguousarray(np.asarray(v.cpu() if torch.is_tensor(v) else v).reshape(-1))
    if a.dtype.kind not in "iu" or a.size != n:
        raise ValueError(f"{what}: {n} integers expected, got {a.shape} {a.dtype}")
    return a.astype(np.int32)


def step_counts(HW, steps):
    """The pixels removed (restored) after step s = 0 .. steps: ``s * HW // steps`` in integer arithmetic; the curves' abscissa is
    ``x[s] = counts[s] / HW``, from 0 to 1 exactly."""
    HW, steps = int(HW), int(steps)
    if HW < 1 or steps < 1:
        raise ValueError(f"step_counts: HW {HW} and steps {steps} are positive")
    return [s * HW // steps for s in range(steps + 1)]


def pixel_ranks(maps):
    """maps [M, h, w] (or [M, HW]) fp32 on the device -> ranks int32 of the same shape: ``ranks[m][p]`` = the position of pixel p when
    map m's pixels are ordered by value descending, ties to the lower flat index (-0.0 == +0.0), a permutation of 0 .. HW - 1 per
    map.  HW <= 65536; NaN is not supported."""
    _device(maps, "pixel_ranks")
    if maps.dim() not in (2, 3):
        raise ValueError(f"pixel_ranks: maps are [M, h, w] or [M, HW], got {tuple(maps.shape)}")
    m = maps.to(torch.float32).contiguous()
    M, HW = m.shape[0], m[0].numel() if m.shape[0] else 0
    lib = H.lib()
    ranks = torch.empty(m.shape, dtype=torch.int32, device=m.device)
    ws = torch.empty(max(16, lib.cvcl_map_ranks_scratch_bytes(M, HW)), dtype=torch.uint8, device=m.device)
    H.check(lib.cvcl_map_ranks(H.ptr(m), H.ptr(ranks), M, HW, H.ptr(ws), ws.numel(), H.stream_ptr()), "cvcl_map_ranks")
    return ranks


def perturb(images, baseline, ranks, image_of_map, item_map, item_count, item_mode, out=None):
    """One cvcl_map_perturb call: work item i -> out[i] [C, H, W] = frame ``image_of_map[item_map[i]]`` with the ``item_count[i]``
    highest-ranked pixels of map ``item_map[i]`` taken from ``baseline`` (``item_mode[i]`` 0, deletion) or ONLY those taken from the
    frame and the rest from ``baseline`` (1, insertion).  images, baseline [N, C, H, W] fp32 (baseline None: zeros) and ranks
    [M, H, W] int32 on the device; image_of_map [M] (None: map m over image m) and the three item vectors are host integers,
    checked before the launch.  ``out``: a [>= n_items, C, H, W] buffer to reuse."""
    _device(images, "perturb")
    _device(ranks, "perturb")
    if baseline is not None:
        _device(baseline, "perturb")
        if baseline.shape != images.shape:
            raise ValueError(f"perturb: baseline {tuple(baseline.shape)} and images {tuple(images.shape)} differ in shape")
    if images.dim() != 4:
        raise ValueError(f"perturb: images are [N, C, H, W], got {tuple(images.shape)}")
    N, C, Hh, Ww = images.shape
    M = ranks.shape[0]
    if ranks.dtype != torch.int32 or ranks.numel() != M * Hh * Ww:
        raise ValueError(f"perturb: ranks are int32 [M, {Hh}, {Ww}], got {tuple(ranks.shape)} {ranks.dtype}")
    n_items = int(np.asarray(item_map.cpu() if torch.is_tensor(item_map) else item_map).size)
    im, ic, imode = (_host_i32(v, n_items, w) for v, w in ((item_map, "item_map"), (item_count, "item_count"), (item_mode, "item_mode")))
    iom = None if image_of_map is None else _host_i32(image_of_map, M, "image_of_map")
    if out is None:
        out = torch.empty(n_items, C, Hh, Ww, dtype=torch.float32, device=images.device)
    _device(out, "perturb")
    if out.dtype != torch.float32 or out.dim() != 4 or out.shape[0] < n_items or tuple(out.shape[1:]) != (C, Hh, Ww):
        raise ValueError(f"perturb: out is fp32 [>= {n_items}, {C}, {Hh}, {Ww}], got {tuple(out.shape)} {out.dtype}")
    H.check(H.lib().cvcl_map_perturb(H.ptr(images, torch.float32), H.ptr(baseline, torch.float32), H.ptr(ranks),
                                     None if iom is None else iom.ctypes.data, im.ctypes.data, ic.ctypes.data, imode.ctypes.data, n_items,
                                     N, M, C, Hh, Ww, H.ptr(out), H.stream_ptr()), "cvcl_map_perturb")
    return out[:n_items]


def gaussian_weights(k, sigma):
    """exp(-(i - r)^2 / (2 sigma^2)) / sum over i = 0 .. k - 1, r = k // 2, formed in float64 and rounded once to fp32"""
    k = int(k)
    i = np.arange(k, dtype=np.float64) - k // 2
    w = np.exp(-(i * i) / (2.0 * float(sigma) ** 2))
    return (w / w.sum()).astype(np.float32)


def gaussian_blur(x, k=11, sigma=5.0):
    """The separable k-tap Gaussian of the last two dimensions of an fp32 device tensor, reflect-padded as torch's "reflect" pads (the
    edge is not repeated), rows then columns: the blurred frame the insertion curve starts from.  k odd, k // 2 < min(H, W)."""
    _device(x, "gaussian_blur")
    if x.dim() < 2:
        raise ValueError(f"gaussian_blur: [..., H, W] expected, got {tuple(x.shape)}")
    x = x.to(torch.float32).contiguous()
    Hh, Ww = x.shape[-2:]
    w = gaussian_weights(k, sigma)
    y, tmp = torch.empty_like(x), torch.empty_like(x)
    H.check(H.lib().cvcl_gaussian_blur_f32(H.ptr(x), H.ptr(y), w.ctypes.data, int(k), x.numel() // max(1, Hh * Ww), Hh, Ww, H.ptr(tmp),
                                           H.stream_ptr()), "cvcl_gaussian_blur_f32")
    return y


def pair_dot(rows, targets, target_of_row, out=None):
    """out[r] = <rows[r], targets[target_of_row[r]]>: rows [R, E], targets [M, E] fp32, target_of_row [R] integers, all on the device"""
    _device(rows, "pair_dot")
    _device(targets, "pair_dot")
    _device(target_of_row, "pair_dot")
    rows, targets = rows.to(torch.float32).contiguous(), targets.to(torch.float32).contiguous()
    idx = target_of_row.to(torch.int32).contiguous()
    if rows.dim() != 2 or targets.dim() != 2 or rows.shape[1] != targets.shape[1] or idx.shape != (rows.shape[0],):
        raise ValueError(f"pair_dot: rows {tuple(rows.shape)}, targets {tuple(targets.shape)}, target_of_row {tuple(idx.shape)}")
    if out is None:
        out = torch.empty(rows.shape[0], dtype=torch.float32, device=rows.device)
    H.check(H.lib().cvcl_pair_dot(H.ptr(rows), H.ptr(targets), H.ptr(idx), H.ptr(out, torch.float32), rows.shape[0], targets.shape[0],
                                  rows.shape[1], H.stream_ptr()), "cvcl_pair_dot")
    return out


def curve_auc(y, x):
    """Trapezoid areas: y [K, S + 1, M], x [S + 1] fp32 on the device -> [K, M] = sum_s (x[s + 1] - x[s]) (y[s] + y[s + 1]) / 2"""
    _device(y, "curve_auc")
    _device(x, "curve_auc")
    y, x = y.to(torch.float32).contiguous(), x.to(torch.float32).contiguous()
    if y.dim() != 3 or x.shape != (y.shape[1],):
        raise ValueError(f"curve_auc: y [K, S + 1, M] and x [S + 1], got {tuple(y.shape)} and {tuple(x.shape)}")
    K, S1, M = y.shape
    auc = torch.empty(K, M, dtype=torch.float32, device=y.device)
    H.check(H.lib().cvcl_curve_auc(H.ptr(y), H.ptr(x), H.ptr(auc), K, S1 - 1, M, H.stream_ptr()), "cvcl_curve_auc")
    return auc


def work_items(M, steps, HW):
    """The work items of one deletion_insertion call as host int32 vectors (item_map, item_count, item_mode): mode (0 deletion, then 1
    insertion), then step ascending, then map ascending."""
    counts = np.asarray(step_counts(HW, steps), dtype=np.int32)
    mode = np.repeat(np.arange(2, dtype=np.int32), (steps + 1) * M)
    count = np.tile(np.repeat(counts, M), 2)
    maps = np.tile(np.arange(M, dtype=np.int32), 2 * (steps + 1))
    return maps, count, mode


def _baseline(spec, images, what):
    if isinstance(spec, str):
        if spec == "zero":
            return None
        if spec == "blur":
            return gaussian_blur(images)
        raise ValueError(f"{what} = {spec!r}: 'zero', 'blur' or a tensor shaped as the images")
    _device(spec, f"deletion_insertion({what})")
    if spec.shape != images.shape:
        raise ValueError(f"{what}: {tuple(spec.shape)} is not the images' shape {tuple(images.shape)}")
    return spec.to(torch.float32).contiguous()


@torch.no_grad()
def deletion_insertion(model, images, targets, maps, image_of_map=None, steps=14, deletion_baseline="zero", insertion_baseline="blur",
                       chunk=256):
    """The deletion and insertion curves of M maps and their areas.

      model    a MultiModalModel (or a lit model, whose ``.model`` is used) in eval mode; everything runs under no_grad
      images   [N, 3, H, W] fp32, normalised, on the device; H W <= 65536
      targets  [M, E]: the text features as ``encode_text`` returns them (normalised when the model normalises)
      maps     [M, h, w] fp32; smaller than the frames: resized with ``attention_maps.bicubic_resize``
      image_of_map  as ``overlay_attention_maps``' image_index: the frame under map m (None: frame m, needs M = N)
      deletion_baseline / insertion_baseline  "zero" (the normalised frame's 0, the dataset mean), "blur"
               (``gaussian_blur(images)``: 11 taps, sigma 5) or a tensor [N, 3, H, W]

    The score of a perturbed frame is ``<encode_image(frame)[0], target>``: the model's logit without the temperature.  Step s removes
    (restores) the ``step_counts(H W, steps)[s]`` highest-ranked pixels; ``x[s]`` is that count over H W.

    ORDER OF THE WORK: the 2 (steps + 1) M work items are ordered by mode (deletion, then insertion), then step ascending, then map
    ascending, and cut into consecutive chunks of ``chunk`` items.  Each chunk is perturbed into one reused buffer (one
    cvcl_map_perturb call per mode present in the chunk: a baseline belongs to a mode) and encoded by ONE ``model.encode_image`` call
    on those ``<= chunk`` frames in that order, so whoever encodes the same frames in the same partition gets the same bits.

    -> {"deletion", "insertion": [M, steps + 1], "auc_deletion", "auc_insertion": [M], "x": [steps + 1]}, fp32 on the device."""
    from .attention_maps import bicubic_resize
    mm = getattr(model, "model", model)
    for t, what in ((images, "images"), (targets, "targets"), (maps, "maps")):
        _device(t, f"deletion_insertion({what})")
    if images.dim() != 4 or maps.dim() != 3 or targets.dim() != 2 or targets.shape[0] != maps.shape[0]:
        raise ValueError(f"deletion_insertion: images [N, 3, H, W], targets [M, E], maps [M, h, w]; got {tuple(images.shape)}, "
                         f"{tuple(targets.shape)}, {tuple(maps.shape)}")
    steps, chunk = int(steps), int(chunk)
    if steps < 1 or chunk < 1:
        raise ValueError(f"deletion_insertion: steps {steps} and chunk {chunk} are positive")
    images = images.to(torch.float32).contiguous()
    targets = targets.to(torch.float32).contiguous()
    N, C, Hh, Ww = images.shape
    M, HW, dev = maps.shape[0], Hh * Ww, images.device
    if HW > MAX_PIXELS:
        raise H.CvclError(f"deletion_insertion: {Hh} x {Ww} frames have more than {MAX_PIXELS} pixels (cvcl_map_ranks' limit)")
    if image_of_map is None:
        if M != N:
            raise ValueError(f"{M} maps for {N} images: give image_of_map (one image per map)")
        iom = np.arange(M, dtype=np.int32)
    else:
        iom = _host_i32(image_of_map, M, "image_of_map")
        if ((iom < 0) | (iom >= N)).any():
            raise ValueError(f"image_of_map has entries outside [0, {N})")
    maps = maps.to(torch.float32).contiguous()
    if tuple(maps.shape[1:]) != (Hh, Ww):
        maps = bicubic_resize(maps, (Hh, Ww))
    ranks = pixel_ranks(maps)
    baselines = (_baseline(deletion_baseline, images, "deletion_baseline"), _baseline(insertion_baseline, images, "insertion_baseline"))
    item_map, item_count, item_mode = work_items(M, steps, HW)
    n_items = item_map.size
    per_mode = n_items // 2
    item_map_dev = torch.from_numpy(item_map).to(dev)
    scores = torch.empty(n_items, dtype=torch.float32, device=dev)
    buf = torch.empty(min(chunk, n_items), C, Hh, Ww, dtype=torch.float32, device=dev)
    for s in range(0, n_items, chunk):
        e = min(s + chunk, n_items)
        for mode in (0, 1):                                # the part of the chunk that lies in this mode's items
            a, b = max(s, mode * per_mode), min(e, (mode + 1) * per_mode)
            if a < b:
                perturb(images, baselines[mode], ranks, iom, item_map[a:b], item_count[a:b], item_mode[a:b], out=buf[a - s:b - s])
        feats = mm.encode_image(buf[:e - s])[0]
        pair_dot(feats.float(), targets, item_map_dev[s:e], out=scores[s:e])
    y = scores.view(2, steps + 1, M)
    x = torch.tensor(np.asarray(step_counts(HW, steps), dtype=np.float64) / HW, dtype=torch.float32, device=dev)
    auc = curve_auc(y, x)
    return {"deletion": y[0].t().contiguous(), "insertion": y[1].t().contiguous(), "auc_deletion": auc[0], "auc_insertion": auc[1], "x": x}


@torch.no_grad()
def maps_of(lit, images, texts, text_lengths, kind, seed=0):
    """Frame n's map for utterance n at the frames' size, [N, H, W] fp32, from the existing producers: ``"gradcam"``
    (attention_maps.gradCAM_pairs, diagonal pairs, the targets being ``encode_text``'s features), ``"cls_attention"``, ``"rollout"``,
    ``"rollout_discard"`` (ratio 0.9) -- the ViT's maps, which do not depend on the text -- or ``"random"``: a ``torch.rand`` map seeded
    with ``seed``, the chance control.  A producer that is not defined for the model's encoder refuses as it always does."""
    from . import attention_maps as AM
    if kind not in MAP_KINDS:
        raise ValueError(f"kind = {kind!r}: one of {MAP_KINDS}")
    _device(images, "maps_of")
    mm = getattr(lit, "model", lit)
    size = tuple(images.shape[2:])
    if kind == "random":
        g = torch.Generator(device=images.device).manual_seed(int(seed))
        return torch.rand(images.shape[0], *size, dtype=torch.float32, device=images.device, generator=g)
    if kind == "gradcam":
        targets = mm.encode_text(texts, text_lengths)[0].float().contiguous()
        return AM.gradCAM_pairs(mm.image_embed, images, targets, normalize_features=bool(mm.normalize_features), pairs="diagonal", resize=size)
    if kind == "cls_attention":
        return AM.vit_cls_attention(mm.image_embed, images, size=size)
    if kind == "rollout":
        return AM.vit_attention_rollout(mm.image_embed, images, size=size)
    return AM.vit_attention_rollout_discard(mm.image_embed, images, ROLLOUT_DISCARD_RATIO, size=size)


# ---- attention_faithfulness.py (the script) --------------------------------------------------------------------------------------------
def _mean_std(v):
    v = np.asarray(v, dtype=np.float64)
    return {"mean": float(v.mean()) if v.size else float("nan"), "std": float(v.std()) if v.size else float("nan")}


def faithfulness_record(auc_deletion, auc_insertion, class_of_frame, class_names, settings):
    """The layout of faithfulness.json from {kind: [n] areas} of both curves: {"kinds": {kind: {"n", "auc_deletion", "auc_insertion",
    "auc_difference": {"mean", "std"} (difference = insertion - deletion, std over the frames, population form), "per_class":
    {class: {"n", "auc_deletion", "auc_insertion", "auc_difference"} (means)}}}, "settings": settings}."""
    cls = np.asarray(class_of_frame, dtype=np.int64)
    kinds = {}
    for kind in auc_deletion:
        d, i = np.asarray(auc_deletion[kind], dtype=np.float64), np.asarray(auc_insertion[kind], dtype=np.float64)
        if d.shape != cls.shape or i.shape != cls.shape:
            raise ValueError(f"{kind}: {d.shape} / {i.shape} areas for {cls.shape[0]} frames")
        per_class = {}
        for c, name in enumerate(class_names):
            sel = cls == c
            if sel.any():
                per_class[name] = {"n": int(sel.sum()), "auc_deletion": float(d[sel].mean()), "auc_insertion": float(i[sel].mean()),
                                   "auc_difference": float((i[sel] - d[sel]).mean())}
        kinds[kind] = {"n": int(d.size), "auc_deletion": _mean_std(d), "auc_insertion": _mean_std(i), "auc_difference": _mean_std(i - d),
                       "per_class": per_class}
    return {"kinds": kinds, "settings": dict(settings)}


def parser():
    import argparse
    ap = argparse.ArgumentParser(description="deletion / insertion faithfulness of attention maps (AUC of the image-text score)")
    ap.add_argument("--checkpoint", default=None, help="a MultiModalLitModel checkpoint (.ckpt)")
    ap.add_argument("--random_init", action="store_true")
    ap.add_argument("--data_dir", default=None, metavar="DIR", help="class-per-folder frames; the folder name is the class word")
    ap.add_argument("--num_samples_per_class", type=int, default=8)
    ap.add_argument("--seed", type=int, default=0, help="seeds the per-class selection, the random maps (and --synthetic's model and frames)")
    ap.add_argument("--use_kitty_label", action="store_true", help='the word of class "cat" is "kitty"')
    ap.add_argument("--synthetic", action="store_true", help="generated frames (no files needed)")
    ap.add_argument("--maps", nargs="+", default=["gradcam", "random"], choices=MAP_KINDS, help="the map kinds to score")
    ap.add_argument("--steps", type=int, default=14, help="slices of the curves")
    ap.add_argument("--chunk", type=int, default=256, help="perturbed frames per encoder pass")
    ap.add_argument("--precision", default="32", choices=("32", "bf16", "32-split"), help="image/text encoder arithmetic")
    ap.add_argument("--out", default=os.path.join("results", "attention_faithfulness"))
    return ap


def check_args(args):
    """What the run needs, before anything is loaded."""
    if args.num_samples_per_class < 1 or args.steps < 1 or args.chunk < 1:
        raise SystemExit("--num_samples_per_class, --steps and --chunk are positive")
    if bool(args.checkpoint) == bool(args.random_init):
        raise SystemExit("--checkpoint PATH or --random_init (one of them)")
    if bool(args.data_dir) == bool(args.synthetic):
        raise SystemExit("--data_dir DIR (one sub-folder per class) or --synthetic (one of them)")
    if len(set(args.maps)) != len(args.maps):
        raise SystemExit("--maps names every kind once")


def _figure_script():
    """generate_attention_maps.py (top level): its loader and its per-class selection are reused, so the figures it draws and the
    numbers written here describe the same frames"""
    root = os.path.dirname(os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
    if root not in sys.path:
        sys.path.insert(0, root)
    import generate_attention_maps
    return generate_attention_maps


def main(args):
    check_args(args)
    G = _figure_script()
    from .alignment import build_model, category_words, word_ids
    from .multimodal_data_module import read_vocab
    from .preprocess import DevicePreprocess
    if not torch.cuda.is_available():
        raise H.CvclError("attention_faithfulness.py needs a GPU (there is no CPU fallback)")
    dev = torch.device("cuda:0")
    frames, frame_class, classes = G.load_frames(args)
    ids = word_ids(category_words(classes, args.use_kitty_label), read_vocab())      # an unknown class word fails here
    lit = build_model(args, dev)
    mm = lit.model
    picked = G.select_per_class(frame_class, len(classes), args.num_samples_per_class, args.seed)
    pre = DevicePreprocess(device=dev)
    curves = {k: [] for k in args.maps}
    aucs = {k: ([], []) for k in args.maps}
    class_of_frame = []
    for c in range(len(classes)):
        if not picked[c]:
            continue
        x = pre([frames[i] for i in picked[c]])                          # [K, 3, 224, 224], normalised
        n = x.shape[0]
        class_of_frame += [c] * n
        text = torch.full((n, 1), ids[c], dtype=torch.long, device=dev)
        length = torch.ones(n, dtype=torch.long, device=dev)
        with torch.no_grad():
            targets = mm.encode_text(text, length)[0].float().contiguous()
        for kind in args.maps:
            maps = maps_of(lit, x, text, length, kind, seed=args.seed + c)
            r = deletion_insertion(mm, x, targets, maps, steps=args.steps, chunk=args.chunk)
            curves[kind].append(torch.stack([r["deletion"], r["insertion"]]).cpu().numpy())          # [2, n, steps + 1]
            aucs[kind][0].append(r["auc_deletion"].cpu().numpy())
            aucs[kind][1].append(r["auc_insertion"].cpu().numpy())
    settings = {"maps": list(args.maps), "steps": args.steps, "chunk": args.chunk, "precision": args.precision, "seed": args.seed,
                "num_samples_per_class": args.num_samples_per_class, "checkpoint": args.checkpoint, "synthetic": bool(args.synthetic),
                "data_dir": args.data_dir, "use_kitty_label": bool(args.use_kitty_label), "deletion_baseline": "zero",
                "insertion_baseline": "blur", "classes": list(classes)}
    record = faithfulness_record({k: np.concatenate(aucs[k][0]) for k in args.maps}, {k: np.concatenate(aucs[k][1]) for k in args.maps},
                                 class_of_frame, classes, settings)
    os.makedirs(args.out, exist_ok=True)
    np.save(os.path.join(args.out, "curves.npy"), np.stack([np.concatenate(curves[k], axis=1) for k in args.maps]))   # [kinds, 2, n, steps + 1]
    with open(os.path.join(args.out, "faithfulness.json"), "w") as f:
        json.dump(record, f)
    for kind in args.maps:
        s = record["kinds"][kind]
        print(f"{kind}: deletion AUC {s['auc_deletion']['mean']:.4f} +- {s['auc_deletion']['std']:.4f}, insertion AUC "
              f"{s['auc_insertion']['mean']:.4f} +- {s['auc_insertion']['std']:.4f}, difference {s['auc_difference']['mean']:.4f} "
              f"({s['n']} frames)")
    return record
