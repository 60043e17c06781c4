"""The object-category evaluation data (reference multimodal/object_categories_data_module.py): 4-way trials over folders of
naturalistic object photographs, one folder per category, the model's out-of-distribution evaluation (reference eval.py:149-160).

Layout, under the dataset root DIR (``--data_dir`` / ``$CVCL_DATA_DIR``; the reference's paths are hard-coded)::

    DIR/object_categories/<category>/*.jpg          (``--object_categories_dir`` names another folder)
    DIR/eval_object_categories.json                 {"data": [{"trial_num", "target_category", "target_img_filename",
                                                               "foil_categories", "foil_img_filenames"}]}
    DIR/vocab.json                                  (optional: the packaged vocabulary otherwise)

The public names, the item layouts and the trial generation are the reference's.  Where this module departs from it:

* The categories are the folder names that are vocabulary words, SORTED; the reference keeps the file system's order.
* An existing ``eval_object_categories.json`` is used as it is (file names absolute, or relative to DIR).  Otherwise it is
  generated with the reference's constants (5 trials per image, 3 foils), keys and order of random draws --
  ``choice(foil categories, 3, replace=False)``, then one ``choice`` of image per foil -- but over sorted listings and from a
  ``np.random.RandomState(seed)`` (``--seed``, default 0), so that a directory gives the same trials on every machine.  The
  reference draws from the unseeded global generator over an unordered glob: its file differs from run to run.
* A category folder without a ``.jpg`` is an error that names it (the reference fails inside ``np.random.choice``).
* ``eval_include_sos_eos`` is forwarded to the datasets; the reference's module drops it (its setup builds both datasets without
  it), so its object-category labels never carry <sos> / <eos>.
* As in the reference (:106-111) the TEXT dataset keeps the base transform under ``clip_eval`` -- CLIP then sees frames stretched to
  224 x 224 under the ImageNet statistics, not its own resize / crop / statistics.  That looks like an oversight of the reference; it
  is kept so that the numbers are comparable, and flagged here.
* Pixels: decoding (PIL, ``convert("RGB")``) stays on the host; resize, ToTensor and Normalize are ``preprocess.DevicePreprocess``
  (Pillow-exact bicubic on the device), so the datasets' frames are device tensors and the loader has no workers.  There is no CPU
  pixel path.

Besides the per-trial datasets the module exposes the evaluation as tables (``frame_files``, ``trial_table``): every distinct
frame and every category word once, and per trial the rows it compares -- what ``multimodal/trials.py`` scores in one launch."""
from __future__ import annotations

import json
import os
from collections import Counter

import numpy as np
import torch

from .lightning import LightningDataModule
from .multimodal_data_module import (CLIP_EVAL, EOS_TOKEN_ID, EVAL_INCLUDE_SOS_EOS, EVAL_TYPE, IMAGE_H, SOS_TOKEN_ID, VOCAB_FILENAME,
                                     data_dir_from, load_data, multiModalDataset_collate_fn, read_vocab)
from .multimodal_saycam_data_module import TRAIN_METADATA_FILENAME

OBJECT_CATEGORIES_DIRNAME = "object_categories"
OBJECT_CATEGORIES_EVAL_METADATA_FILENAME = "eval_object_categories.json"
N_EVALUATIONS_PER_EXAMPLE = 5
N_FOILS = 3
TRIAL_KEYS = ("trial_num", "target_category", "target_img_filename", "foil_categories", "foil_img_filenames")


def _resolve(data_dir, filename):
    return filename if os.path.isabs(filename) or data_dir is None else os.path.join(data_dir, filename)


def _decode(path):
    from PIL import Image
    return Image.open(path).convert("RGB")


def _word_label(vocab, word, sos_eos):
    label = [vocab[word]]
    return [SOS_TOKEN_ID] + label + [EOS_TOKEN_ID] if sos_eos else label      # [<sos>, label, <eos>] to match LM training


def _transforms(clip_eval):
    """(the image dataset's transform, the text dataset's): see the module docstring for the text one under clip_eval"""
    from .preprocess import DevicePreprocess
    base = DevicePreprocess(IMAGE_H, "stretch")
    if clip_eval:
        from .clip_model import clip_preprocess
        return clip_preprocess(), base
    return base, base


class ObjectCategoriesEvalDataset(torch.utils.data.Dataset):
    """One category word and 4 photographs (reference :28-93): item = (imgs [4, 3, 224, 224] on the device with the target image
    first, label ids [1] ([3] with sos / eos), its length, [raw target category]).  ``clip_eval``: CLIP's transform, and the label is
    the raw category through CLIP's tokenizer, [1, 77], with length 1 (its row count, as in the reference)."""

    def __init__(self, data, vocab, eval_include_sos_eos=False, clip_eval=False, data_dir=None, clip_bpe=None):
        self.data, self.vocab, self.eval_include_sos_eos, self.clip_eval = data, vocab, eval_include_sos_eos, clip_eval
        self.data_dir, self.clip_bpe = data_dir, clip_bpe
        if clip_eval and not clip_bpe:
            raise ValueError("clip_eval needs clip_bpe: the path of CLIP's bpe_simple_vocab_16e6.txt(.gz)")
        self.transform = _transforms(clip_eval)[0]

    def __getitem__(self, idx):
        trial = self.data[idx]
        names = [trial["target_img_filename"]] + list(trial["foil_img_filenames"])       # the target image is always the first
        imgs = self.transform([_decode(_resolve(self.data_dir, n)) for n in names])
        raw_label = trial["target_category"]
        if self.clip_eval:
            from .clip_model import tokenize
            label = tokenize([raw_label], self.clip_bpe)
        else:
            label = torch.LongTensor(_word_label(self.vocab, raw_label, self.eval_include_sos_eos))
        return imgs, label, len(label), [raw_label]

    def __len__(self):
        return len(self.data)


class ObjectCategoriesTextEvalDataset(torch.utils.data.Dataset):
    """One photograph and 4 category words (reference :95-154): item = (img [1, 3, 224, 224] on the device, label ids [4, 1]
    ([4, 3] with sos / eos; [4, 77] CLIP tokens under ``clip_eval``) with the target category first, [4 lengths], [raw target
    category]).  The transform is the base one even under ``clip_eval``, as in the reference (module docstring)."""

    def __init__(self, data, vocab, eval_include_sos_eos=False, clip_eval=False, data_dir=None, clip_bpe=None):
        self.data, self.vocab, self.eval_include_sos_eos, self.clip_eval = data, vocab, eval_include_sos_eos, clip_eval
        self.data_dir, self.clip_bpe = data_dir, clip_bpe
        if clip_eval and not clip_bpe:
            raise ValueError("clip_eval needs clip_bpe: the path of CLIP's bpe_simple_vocab_16e6.txt(.gz)")
        self.transform = _transforms(clip_eval)[1]

    def __getitem__(self, idx):
        trial = self.data[idx]
        img = self.transform([_decode(_resolve(self.data_dir, trial["target_img_filename"]))])
        raw_target_label = trial["target_category"]
        raw_labels = [raw_target_label] + list(trial["foil_categories"])
        if self.clip_eval:
            from .clip_model import tokenize
            return img, tokenize(raw_labels, self.clip_bpe), [1] * len(raw_labels), [raw_target_label]
        labels = [_word_label(self.vocab, w, self.eval_include_sos_eos) for w in raw_labels]
        return img, torch.LongTensor(labels), [len(l) for l in labels], [raw_target_label]

    def __len__(self):
        return len(self.data)


class ObjectCategoriesDataModule(LightningDataModule):
    """The data module of the object-category evaluation (reference :157-199): ``prepare_data`` lists the categories and writes the
    metadata file if there is none, ``setup`` reads it and builds the dataset of ``args.eval_type``, ``test_dataloader`` yields one
    trial per batch.  After ``setup``: ``object_categories``, ``data`` (the trials), ``frame_files`` and ``trial_table``."""

    def __init__(self, args=None) -> None:
        super().__init__()
        self.args = vars(args) if args is not None and not isinstance(args, dict) else dict(args or {})
        self.eval_type = self.args.get("eval_type", EVAL_TYPE) or EVAL_TYPE
        self.clip_eval = bool(self.args.get("clip_eval", CLIP_EVAL))
        self.clip_bpe = self.args.get("clip_bpe")
        self.eval_include_sos_eos = bool(self.args.get("eval_include_sos_eos", EVAL_INCLUDE_SOS_EOS))
        self.seed = int(self.args.get("seed", 0) or 0)
        self.object_categories_dir = self.args.get("object_categories_dir") or None
        self.data_dir = data_dir_from(self.args)
        if not self.data_dir and self.object_categories_dir:   # the metadata file then sits beside the folder
            self.data_dir = os.path.dirname(os.path.abspath(self.object_categories_dir))
        if not self.data_dir:
            raise ValueError("the object-category data module needs a dataset directory: --data_dir DIR or $CVCL_DATA_DIR (or "
                             "--object_categories_dir DIR)")
        if not self.object_categories_dir:
            self.object_categories_dir = os.path.join(self.data_dir, OBJECT_CATEGORIES_DIRNAME)
        self.metadata_filename = os.path.join(self.data_dir, OBJECT_CATEGORIES_EVAL_METADATA_FILENAME)

    def read_vocab(self):
        own = os.path.join(self.data_dir, "vocab.json")
        return read_vocab(own if os.path.exists(own) else VOCAB_FILENAME)

    def prepare_data(self, *args, **kwargs) -> None:
        self.vocab = self.read_vocab()
        self.object_categories = _get_object_categories(self.vocab, self.object_categories_dir)
        _generate_object_category_eval_metadata(self.object_categories, self.object_categories_dir, self.metadata_filename, self.seed)

    def setup(self, *args, **kwargs) -> None:
        self.vocab = self.read_vocab()
        if not hasattr(self, "object_categories"):
            self.object_categories = _get_object_categories(self.vocab, self.object_categories_dir)
        self.data = load_data(self.metadata_filename)
        cls = ObjectCategoriesEvalDataset if self.eval_type == "image" else ObjectCategoriesTextEvalDataset
        self.eval_dataset = cls(self.data, self.vocab, eval_include_sos_eos=self.eval_include_sos_eos, clip_eval=self.clip_eval,
                                data_dir=self.data_dir, clip_bpe=self.clip_bpe)
        self.frame_files = sorted({_resolve(self.data_dir, n) for t in self.data
                                   for n in [t["target_img_filename"]] + list(t["foil_img_filenames"])})

    def test_dataloader(self, shuffle=False):
        """One trial per batch (:187-196); no workers: an item is made on the device."""
        return torch.utils.data.DataLoader(self.eval_dataset, collate_fn=multiModalDataset_collate_fn, shuffle=shuffle, batch_size=1,
                                           num_workers=0, pin_memory=False)

    # ---- the evaluation as tables -------------------------------------------------------------------------------------------------
    def frame_transform(self, eval_type=None):
        """The device transform the dataset of ``eval_type`` applies to a decoded frame."""
        return _transforms(self.clip_eval)[0 if (eval_type or self.eval_type) == "image" else 1]

    def load_frames(self, files, eval_type=None):
        """files -> [len(files), 3, 224, 224] on the device: host decode, one preprocessing launch for the (mixed-size) batch."""
        return self.frame_transform(eval_type)([_decode(f) for f in files])

    def trial_table(self, eval_type=None, use_kitty_label=False):
        """Every trial as rows of two tables.  -> dict with

        ``words``      the category words to encode, one row each: the module's categories, then any other category the metadata
                       names, then "kitty" when ``use_kitty_label`` is set (``kitty_row``: its row, else None)
        ``word_rows``  int64 [C, L] the words as the datasets write a label (L = 1, or 3 with sos / eos; [C, 77] CLIP tokens under
                       clip_eval), ``word_lens`` int64 [C] (None under clip_eval)
        ``q_idx``      int32 [T]: the trial's query row -- ``image``: the target's WORD row; ``text``: the target's FRAME row
        ``c_idx``      int32 [T, 4]: its candidate rows, target first -- ``image``: FRAME rows; ``text``: WORD rows
        Frame rows index ``frame_files``.  ``use_kitty_label`` replaces the word of "cat" TARGETS only (a foil "cat" stays "cat"),
        as eval.py does per trial."""
        eval_type = eval_type or self.eval_type
        words = list(self.object_categories)
        for t in self.data:
            for w in [t["target_category"]] + list(t["foil_categories"]):
                if w not in words:
                    words.append(w)
        kitty_row = None
        if use_kitty_label:
            kitty_row = len(words)
            words.append("kitty")
        word_row = {w: i for i, w in enumerate(words)}
        frame_row = {f: i for i, f in enumerate(self.frame_files)}
        if self.clip_eval:
            from .clip_model import tokenize
            word_rows, word_lens = tokenize(words, self.clip_bpe).long(), None
        else:
            labels = [_word_label(self.vocab, w, self.eval_include_sos_eos) for w in words]
            word_rows = torch.LongTensor(labels)
            word_lens = torch.tensor([len(l) for l in labels], dtype=torch.long)
        T = len(self.data)
        n = 1 + (len(self.data[0]["foil_categories"]) if T else N_FOILS)
        q_idx, c_idx = np.empty(T, dtype=np.int32), np.empty((T, n), dtype=np.int32)
        for i, t in enumerate(self.data):
            target = t["target_category"]
            target_word = kitty_row if use_kitty_label and target == "cat" else word_row[target]
            target_frame = frame_row[_resolve(self.data_dir, t["target_img_filename"])]
            if eval_type == "image":
                q_idx[i] = target_word
                c_idx[i] = [target_frame] + [frame_row[_resolve(self.data_dir, f)] for f in t["foil_img_filenames"]]
            else:
                q_idx[i] = target_frame
                c_idx[i] = [target_word] + [word_row[w] for w in t["foil_categories"]]
        return {"words": words, "kitty_row": kitty_row, "word_rows": word_rows, "word_lens": word_lens, "q_idx": q_idx, "c_idx": c_idx}


def _get_object_categories(vocab, object_categories_dir):
    """The category folders whose names are vocabulary words (:202-214), sorted."""
    if not os.path.isdir(object_categories_dir):
        raise FileNotFoundError(f"no object-category directory at {object_categories_dir}")
    return sorted(d for d in os.listdir(object_categories_dir)
                  if os.path.isdir(os.path.join(object_categories_dir, d)) and d in vocab)


def _category_images(object_categories_dir, object_category):
    """The sorted .jpg files of one category; an empty folder is refused by name."""
    folder = os.path.join(object_categories_dir, object_category)
    files = sorted(os.path.join(folder, f) for f in os.listdir(folder) if f.endswith(".jpg"))
    if not files:
        raise ValueError(f"object category {object_category!r} has no .jpg file ({folder})")
    return files


def _generate_object_category_eval_trial(idx, target_img_filename, target_category, object_categories, n_foils, rng, images):
    """One evaluation trial (:248-269), the reference's draws in its order from ``rng``: the foil categories without replacement,
    then one image of each.  ``images``: category -> its sorted files."""
    foil_categories = object_categories.copy()
    foil_categories.remove(target_category)
    foil_categories = rng.choice(foil_categories, size=n_foils, replace=False)
    foil_img_filenames = []
    for i in range(n_foils):
        foil_img_filenames.append(str(rng.choice(images[str(foil_categories[i])])))
    return {"trial_num": idx, "target_category": target_category, "target_img_filename": str(target_img_filename),
            "foil_categories": [str(c) for c in foil_categories], "foil_img_filenames": foil_img_filenames}


def _generate_object_category_eval_metadata(object_categories, object_categories_dir, metadata_filename, seed=0):
    """Write the trials of the evaluation (:272-297) unless the file exists: per category (sorted), per image (sorted), 5 trials."""
    if os.path.exists(metadata_filename):
        print("Object categories evaluation metadata files have already been created. Skipping this step.")
        return
    print("Creating metadata files for object categories evaluation.")
    images = {c: _category_images(os.path.abspath(object_categories_dir), c) for c in object_categories}
    rng = np.random.RandomState(seed)
    eval_dataset = []
    for target_category in object_categories:
        for target_img_filename in images[target_category]:
            for i in range(N_EVALUATIONS_PER_EXAMPLE):
                eval_dataset.append(_generate_object_category_eval_trial(i, target_img_filename, target_category, object_categories,
                                                                         N_FOILS, rng, images))
    with open(metadata_filename, "w") as f:
        json.dump({"data": eval_dataset}, f)


def _get_object_category_word_counts(data_dir, object_categories):
    """How often each category word occurs in the training utterances (:300-316; the reference's version reads an undefined name)."""
    counts = Counter(w for d in load_data(os.path.join(data_dir, TRAIN_METADATA_FILENAME)) for w in d["utterance"].split(" "))
    return {c: counts[c] for c in object_categories}
