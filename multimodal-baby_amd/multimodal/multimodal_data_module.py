"""Batch contract of the reference data modules, its evaluation-trial datasets and loaders, + a synthetic data module.

Mirrors the constants, ``read_vocab`` / ``load_data``, ``multiModalDataset_collate_fn``, the two evaluation datasets, setup, the
data loaders and the CLI flags of the reference (multimodal/multimodal_data_module.py:26-69, 98-214, 283-427).  The SAYCam
module on top of it is multimodal_saycam_data_module.py: it reads a dataset directory in the reference's layout, given by
``--data_dir`` / ``$CVCL_DATA_DIR`` (the reference's data is private, its format is not).  The object-categories module is
object_categories_data_module.py; the COCO module is not built; ``SyntheticDataModule`` produces batches of the same shape without any files.

A frame reaches the model by one of three paths (``FrameSource``): decoded and transformed in the loader workers (default),
decoded in the workers and transformed on the device (``--device_frames``), or never decoded at run time at all -- the
datasets return the frame's row in the HBM-resident frame store and the transform kernel reads it through that index
(``--frame_store PATH``, multimodal/frame_store.py)."""
from __future__ import annotations

import json
import os

import numpy as np
import torch
from torch.nn.utils.rnn import pad_sequence

from .lightning import LightningDataModule

BATCH_SIZE = 4
VAL_BATCH_SIZE = 16
NUM_WORKERS = 4
EVAL_INCLUDE_SOS_EOS = False
N_VAL_DATALOADERS_PER_SPLIT = 2
TEST_WHILE_VAL = False
EVAL_TYPE = "image"
MAX_LEN_UTTERANCE = 25
AUGMENT_FRAMES = False
PAD_TOKEN, UNK_TOKEN, SOS_TOKEN, EOS_TOKEN = "<pad>", "<unk>", "<sos>", "<eos>"
PAD_TOKEN_ID, UNK_TOKEN_ID, SOS_TOKEN_ID, EOS_TOKEN_ID = 0, 1, 2, 3
IMAGE_H = IMAGE_W = 224
IMAGENET_MEAN, IMAGENET_STD = (0.485, 0.456, 0.406), (0.229, 0.224, 0.225)
CLIP_MEAN, CLIP_STD = (0.48145466, 0.4578275, 0.40821073), (0.26862954, 0.26130258, 0.27577711)       # reference :262
CLIP_EVAL = False
VOCAB_FILENAME = os.path.join(os.path.dirname(os.path.abspath(__file__)), "vocab.json")


def read_vocab(vocab_filename=VOCAB_FILENAME):
    with open(vocab_filename) as f:
        return json.load(f)


def load_data(filename):
    with open(filename) as f:
        return json.load(f)["data"]


def data_dir_from(args):
    """The dataset root: ``--data_dir``, else $CVCL_DATA_DIR, else None (there is no built-in path)."""
    d = args.get("data_dir") if isinstance(args, dict) else getattr(args, "data_dir", None)
    return d or os.environ.get("CVCL_DATA_DIR") or None


class HostFrameTransform:
    """The reference's per-frame transform on a PIL image in a loader worker (torchvision is not a dependency, so ToTensor and
    Normalize are spelled out): ``augment_frames`` draws the reference's crop / blur / flip per frame in its order
    (``DeviceFrameAugment.sample_params_sequential``) and applies them with Pillow, then (u8 / 255 - mean) / std in fp32,
    CHW.  Without it this is ``base_transform`` (:271-280)."""

    def __init__(self, augment_frames=False, mean=IMAGENET_MEAN, std=IMAGENET_STD, size=(IMAGE_H, IMAGE_W)):
        self.augment_frames = bool(augment_frames)
        self.mean = torch.tensor(mean, dtype=torch.float32).view(3, 1, 1)
        self.std = torch.tensor(std, dtype=torch.float32).view(3, 1, 1)
        self.size = tuple(size)
        self._draws = None

    def __call__(self, img):
        if self.augment_frames:
            from PIL import Image, ImageFilter
            if self._draws is None:
                from .augment import DeviceFrameAugment          # only its host-side draws are used here
                self._draws = DeviceFrameAugment(augment_frames=True, size=self.size)
            p = self._draws.sample_params_sequential(1, img.height, img.width)
            top, left, h, w = (int(v) for v in p.crop[0])
            img = img.crop((left, top, left + w, top + h)).resize((self.size[1], self.size[0]), Image.BILINEAR)
            if float(p.sigma[0]) > 0:
                img = img.filter(ImageFilter.GaussianBlur(radius=float(p.sigma[0])))
            if int(p.flip[0]):
                img = img.transpose(Image.FLIP_LEFT_RIGHT)
        x = torch.from_numpy(np.array(img, dtype=np.uint8)).permute(2, 0, 1).float().div(255.0)
        return x.sub_(self.mean).div_(self.std)


class FrameSource:
    """How a dataset turns a frame key (frame_store.frame_key) into the image of its item:
    ``host``  PIL decode + the dataset's transform -> fp32 [3, H, W]
    ``uint8`` PIL decode -> uint8 [H, W, 3]; the transform runs on the device after the batch transfer
    ``index`` no decode: the frame's row in the frame store as an int64 scalar (``rows``: key -> row)."""

    def __init__(self, data_dir, mode="host", rows=None):
        if mode not in ("host", "uint8", "index"):
            raise ValueError(f"unknown frame mode {mode!r}")
        if mode == "index" and rows is None:
            raise ValueError("frame mode 'index' needs the store's key -> row map")
        self.data_dir, self.mode, self.rows = (str(data_dir) if data_dir is not None else None), mode, rows

    def resolve(self, keys):
        """Every key of a split, checked once when its dataset is built: under ``index`` a frame that is not in the store stops the
        run here (KeyError naming it), not in the middle of an epoch."""
        if self.mode == "index":
            for k in keys:
                if k not in self.rows:
                    raise KeyError(f"frame {k!r} is not in the frame store")

    def path(self, key):
        return key if os.path.isabs(key) or self.data_dir is None else os.path.join(self.data_dir, key)

    def decode(self, key):
        from PIL import Image
        return Image.open(self.path(key)).convert("RGB")

    def __call__(self, key, transform=None):
        if self.mode == "index":
            return torch.tensor(int(self.rows[key]), dtype=torch.int64)
        img = self.decode(key)
        if self.mode == "uint8":
            return torch.from_numpy(np.array(img, dtype=np.uint8))
        return transform(img) if transform is not None else img


def _eval_label(vocab, word, sos_eos):
    label = [vocab[word]]
    return [SOS_TOKEN_ID] + label + [EOS_TOKEN_ID] if sos_eos else label      # [<sos>, label, <eos>] to match LM training


class LabeledSEvalDataset(torch.utils.data.Dataset):
    """One target word and its referents (reference :112-160): item = (imgs [n, 3, H, W] with the target image first, label ids
    [L], L, [raw target category]).  Under the ``uint8`` / ``index`` frame modes imgs is uint8 [n, H, W, 3] / int64 [n].  The CLIP
    branch of the reference is not built."""

    def __init__(self, data, vocab, transform, eval_include_sos_eos=False, frames=None):
        self.data, self.vocab, self.transform, self.eval_include_sos_eos = data, vocab, transform, eval_include_sos_eos
        self.frames = frames if frames is not None else FrameSource(None)
        self.frames.resolve(k for t in data for k in [t["target_img_filename"]] + list(t["foil_img_filenames"]))

    def __getitem__(self, idx):
        trial = self.data[idx]
        names = [trial["target_img_filename"]] + list(trial["foil_img_filenames"])
        imgs = torch.stack([self.frames(n, self.transform) for n in names], 0)
        raw_label = trial["target_category"]
        label = _eval_label(self.vocab, raw_label, self.eval_include_sos_eos)
        return imgs, torch.LongTensor(label), len(label), [raw_label]

    def __len__(self):
        return len(self.data)


class LabeledSTextEvalDataset(torch.utils.data.Dataset):
    """One referent and several words (reference :163-214): item = (img [1, 3, H, W], label ids [n, L] with the target category
    first, [n lengths], [raw target category])."""

    def __init__(self, data, vocab, transform, eval_include_sos_eos=False, frames=None):
        self.data, self.vocab, self.transform, self.eval_include_sos_eos = data, vocab, transform, eval_include_sos_eos
        self.frames = frames if frames is not None else FrameSource(None)
        self.frames.resolve(t["target_img_filename"] for t in data)

    def __getitem__(self, idx):
        trial = self.data[idx]
        img = self.frames(trial["target_img_filename"], self.transform).unsqueeze(0)
        raw_target = trial["target_category"]
        labels = [_eval_label(self.vocab, w, self.eval_include_sos_eos) for w in [raw_target] + list(trial["foil_categories"])]
        return img, torch.LongTensor(labels), [len(l) for l in labels], [raw_target]

    def __len__(self):
        return len(self.data)


def multiModalDataset_collate_fn(batch):
    """(img, idxs, len, raw) items -> (img [B,3,H,W], idxs [B,Lmax<=25] pad 0, len [B] int64, raw list)."""
    img, idxs, length, raw = zip(*batch)
    img = torch.stack(img, 0)
    idxs = pad_sequence(idxs, batch_first=True, padding_value=PAD_TOKEN_ID)
    length = torch.tensor(length, dtype=torch.long)
    if idxs.size(1) > MAX_LEN_UTTERANCE:
        idxs = idxs[:, :MAX_LEN_UTTERANCE]
        length = torch.clamp(length, max=MAX_LEN_UTTERANCE)
    return img, idxs, length, list(raw)


class MultiModalDataModule(LightningDataModule):
    def __init__(self, args=None):
        super().__init__()
        self.args = vars(args) if args is not None else {}
        self.batch_size = self.args.get("batch_size", BATCH_SIZE)
        self.drop_last = self.args.get("drop_last", False)
        self.val_batch_size = self.args.get("val_batch_size", VAL_BATCH_SIZE)
        self.num_workers = self.args.get("num_workers", NUM_WORKERS)
        self.augment_frames = self.args.get("augment_frames", False)
        # --device_frames: the datasets hand over decoded uint8 frames [H, W, 3] and the transform of :244-256 (or the base
        # transform) runs on the device after the batch transfer (multimodal/augment.py) instead of per frame in the workers
        self.device_frames = bool(self.args.get("device_frames", False))
        self._frame_transforms = None
        self.eval_include_sos_eos = self.args.get("eval_include_sos_eos", EVAL_INCLUDE_SOS_EOS)
        self.test_while_val = self.args.get("test_while_val", TEST_WHILE_VAL)
        self.eval_type = self.args.get("eval_type", EVAL_TYPE) or EVAL_TYPE
        self.eval_metadata_filename = self.args.get("eval_metadata_filename", "eval_dev.json")
        self.data_dir = data_dir_from(self.args)
        # --frame_store PATH: the datasets yield frame indices; the store itself is loaded into HBM at setup()
        self.frame_store_path = self.args.get("frame_store") or None
        self.frame_store = None
        # the host path's transforms (:244-280): the training one draws the augmentation when asked to, val / test keep the base one
        self.transform = HostFrameTransform(self.augment_frames)
        self.base_transform = HostFrameTransform(False)

    def on_after_batch_transfer(self, batch, dataloader_idx=0, training=True):
        """Lightning's hook of the same name: uint8 frame batches [B, H, W, 3] (or evaluation trials [B, n, H, W, 3]) become
        normalised fp32 [.., 3, 224, 224] tensors on the device; the training transform only while training (the reference
        keeps ``base_transform`` for val / test, :271-275).  Batches that already hold float images pass through."""
        img = batch[0] if isinstance(batch, (list, tuple)) and len(batch) > 0 else None
        by_index = torch.is_tensor(img) and img.dtype == torch.int64 and self.frame_store is not None
        if not by_index and (not torch.is_tensor(img) or img.dtype != torch.uint8):
            return batch
        from .augment import DeviceFrameAugment
        if self._frame_transforms is None:
            self._frame_transforms = {True: DeviceFrameAugment(augment_frames=self.augment_frames),
                                      False: DeviceFrameAugment(augment_frames=False)}
        tf = self._frame_transforms[self._uses_training_transform(dataloader_idx, bool(training))]
        if by_index:                                       # frame rows [B] or trials [B, n]: read through the index, no gathered copy
            lead = img.shape
            out = self.frame_store._launch(img.reshape(-1).to(self.frame_store.device, non_blocking=True), tf)
        else:
            lead = img.shape[:-3]
            out = tf(img.reshape(-1, *img.shape[-3:]))
        return type(batch)((out.reshape(*lead, *out.shape[1:]),) + tuple(batch[1:]))

    def _uses_training_transform(self, dataloader_idx, training):
        return training

    @staticmethod
    def add_to_argparse(parser):
        parser.add_argument("--batch_size", type=int, default=BATCH_SIZE)
        parser.add_argument("--drop_last", action="store_true")
        parser.add_argument("--val_batch_size", type=int, default=VAL_BATCH_SIZE)
        parser.add_argument("--num_workers", type=int, default=NUM_WORKERS)
        parser.add_argument("--augment_frames", action="store_true")
        parser.add_argument("--device_frames", action="store_true",
                            help="datasets yield uint8 frames; the (augmentation or base) transform runs on the GPU per batch")
        parser.add_argument("--eval_include_sos_eos", action="store_true")
        parser.add_argument("--test_while_val", action="store_true")
        parser.add_argument("--eval_type", type=str, default=EVAL_TYPE, choices=["image", "text"])
        parser.add_argument("--eval_metadata_filename", type=str, default="eval_filtered_dev.json")
        parser.add_argument("--clip_eval", action="store_true")
        parser.add_argument("--data_dir", type=str, default=None, metavar="DIR",
                            help="dataset root in the reference's layout (train.json, val.json, test.json, vocab.json, train_5fps/, "
                                 "eval_*.json); default: $CVCL_DATA_DIR")
        parser.add_argument("--frame_store", type=str, default=None, metavar="PATH",
                            help="a store written by tools/pack_frames.py: loaded into HBM at start-up; batches carry frame indices")
        return parser

    @staticmethod
    def add_additional_to_argparse(parser):
        parser.add_argument("--multiple_frames", action="store_true")
        parser.add_argument("--shuffle_utterances", action="store_true")
        parser.add_argument("--multiple_captions", action="store_true")
        return parser

    def read_vocab(self):
        return read_vocab()

    # ---- the reference's setup and loaders (:318-427), for the modules that read files ----
    def prepare_data(self, *args, **kwargs):
        pass                                               # the reference's download / extraction / filtering steps are not built

    def frame_source(self):
        mode = "index" if self.frame_store_path else ("uint8" if self.device_frames else "host")
        rows = None
        if mode == "index":
            from .frame_store import FrameStore
            if self.frame_store is None:
                device = torch.device("cuda", torch.cuda.current_device()) if torch.cuda.is_available() else torch.device("cpu")
                self.frame_store = FrameStore.load(self.frame_store_path, device)
            rows = self.frame_store.index
        return FrameSource(self.data_dir, mode, rows)

    def setup(self, *args, **kwargs):
        vocab = self.read_vocab()
        self.frames = self.frame_source()
        self.datasets = self.create_datasets(vocab)
        self.eval_datasets = self.create_eval_datasets(vocab)

    def create_datasets(self, vocab):
        raise NotImplementedError

    def create_eval_datasets(self, vocab):
        """:339-360.  The test split's file is the dev file's name with "dev" replaced by "test".  As in the reference the trial
        datasets get ``self.transform`` -- the TRAINING transform, augmentation included when --augment_frames is on -- not
        ``self.base_transform`` (eval.py switches augment_frames off before it builds the module)."""
        eval_datasets = {}
        for split, name in (("val", self.eval_metadata_filename), ("test", self.eval_metadata_filename.replace("dev", "test"))):
            data = load_data(os.path.join(self.data_dir, name))
            cls = LabeledSEvalDataset if self.eval_type == "image" else LabeledSTextEvalDataset
            eval_datasets[split] = cls(data, vocab, self.transform, self.eval_include_sos_eos, frames=self.frames)
        return eval_datasets

    def _loader(self, dataset, batch_size, shuffle=False, drop_last=False):
        workers = 0 if self.frames.mode == "index" else self.num_workers       # an index item is a dictionary lookup: nothing to decode
        return torch.utils.data.DataLoader(dataset, collate_fn=multiModalDataset_collate_fn, shuffle=shuffle, batch_size=batch_size,
                                           drop_last=drop_last, num_workers=workers, pin_memory=False)

    def train_dataloader(self, batch_size=None, shuffle=True, drop_last=None):
        return self._loader(self.datasets["train"], self.batch_size if batch_size is None else batch_size, shuffle,
                            self.drop_last if drop_last is None else drop_last)

    def val_test_dataloader(self, dataset, eval_dataset, batch_size=None, shuffle=False, drop_last=False):
        """[pair batches at val_batch_size, one evaluation trial per batch] (:378-403)"""
        return [self._loader(dataset, self.val_batch_size if batch_size is None else batch_size, shuffle, drop_last),
                self._loader(eval_dataset, 1, shuffle)]

    def val_dataloader(self, batch_size=None, shuffle=False, drop_last=False):
        loaders = self.val_test_dataloader(self.datasets["val"], self.eval_datasets["val"], batch_size, shuffle, drop_last)
        if self.test_while_val:
            loaders += self.test_dataloader(batch_size=batch_size, shuffle=shuffle, drop_last=drop_last)
        return loaders

    def test_dataloader(self, batch_size=None, shuffle=False, drop_last=False):
        return self.val_test_dataloader(self.datasets["test"], self.eval_datasets["test"], batch_size, shuffle, drop_last)


class SyntheticPairs(torch.utils.data.Dataset):
    """``rand -> ImageNet normalise`` frames and ``<sos> w1..wn <eos>`` utterances (reference item shape:
    multimodal_saycam_data_module.py:93-124; image statistics: multimodal_data_module.py:57)."""

    def __init__(self, n_items: int, vocab_size: int, n_words: int = 3, seed: int = 0, raw_frames: bool = False):
        self.n, self.vocab_size, self.n_words, self.seed = n_items, vocab_size, n_words, seed
        self.raw_frames = raw_frames                       # uint8 [H, W, 3] frames for the device transform
        self.mean = torch.tensor(IMAGENET_MEAN).view(3, 1, 1)
        self.std = torch.tensor(IMAGENET_STD).view(3, 1, 1)

    def __len__(self):
        return self.n

    def __getitem__(self, idx):
        g = torch.Generator().manual_seed(self.seed * 1000003 + idx)
        if self.raw_frames:
            img = torch.randint(0, 256, (IMAGE_H, IMAGE_W, 3), dtype=torch.uint8, generator=g)
        else:
            img = (torch.rand(3, IMAGE_H, IMAGE_W, generator=g) - self.mean) / self.std
        words = torch.randint(4, self.vocab_size, (self.n_words,), generator=g)
        idxs = torch.cat([torch.tensor([SOS_TOKEN_ID]), words, torch.tensor([EOS_TOKEN_ID])]).long()
        return img, idxs, int(idxs.numel()), [" ".join(f"w{int(w)}" for w in words)]


class SyntheticEvalTrials(torch.utils.data.Dataset):
    """4-way evaluation trials with the item layout of the reference's LabeledSEvalDataset (``eval_type='image'``:
    (imgs [4,3,H,W] target first, label ids [L], label length, [raw category]); multimodal_data_module.py:112-160) or
    LabeledSTextEvalDataset (``eval_type='text'``: (img [1,3,H,W], label ids [4,L] target first, [4 lengths], [raw target]);
    :163-213).  ``metadata()`` is the list the reference reads from eval_*.json (target_category / foil_categories).
    ``clip_bpe`` (``--clip_eval``, :143-155, 191-202, 256-262): the same frames under CLIP's normalisation -- they are already 224 x 224,
    so the resize and centre crop of CLIP's transform do not apply -- and the raw category names through the CLIP tokenizer:
    label [1, 77] (``image``) or [4, 77] (``text``), lengths counting rows as in the reference."""

    def __init__(self, n_trials, vocab_size, seed=0, eval_include_sos_eos=False, n_images=4, raw_frames=False, eval_type="image",
                 clip_bpe=None):
        self.n, self.v, self.seed, self.sos_eos, self.n_images = n_trials, vocab_size, seed, eval_include_sos_eos, n_images
        self.raw_frames = raw_frames and clip_bpe is None
        self.eval_type = eval_type
        self.clip_bpe = clip_bpe

    def __len__(self):
        return self.n

    def _words(self, idx):
        g = torch.Generator().manual_seed(self.seed * 7919 + idx)
        words = torch.randperm(self.v - 4, generator=g)[: self.n_images] + 4          # target + distinct foil categories
        return g, [int(w) for w in words]

    def metadata(self):
        out = []
        for idx in range(self.n):
            _, words = self._words(idx)
            out.append({"target_category": f"w{words[0]}", "foil_categories": [f"w{w}" for w in words[1:]]})
        return out

    def _wrap(self, word):
        return [SOS_TOKEN_ID, word, EOS_TOKEN_ID] if self.sos_eos else [word]

    def __getitem__(self, idx):
        g, words = self._words(idx)
        n_img = self.n_images if self.eval_type == "image" else 1
        if self.raw_frames:
            imgs = torch.randint(0, 256, (n_img, IMAGE_H, IMAGE_W, 3), dtype=torch.uint8, generator=g)
        else:
            mean = torch.tensor(CLIP_MEAN if self.clip_bpe else IMAGENET_MEAN).view(1, 3, 1, 1)
            std = torch.tensor(CLIP_STD if self.clip_bpe else IMAGENET_STD).view(1, 3, 1, 1)
            imgs = (torch.rand(n_img, 3, IMAGE_H, IMAGE_W, generator=g) - mean) / std
        if self.clip_bpe:
            from .clip_model import tokenize
            names = [f"w{w}" for w in (words[:1] if self.eval_type == "image" else words)]
            label = tokenize(names, self.clip_bpe)
            return imgs, label, (len(label) if self.eval_type == "image" else [1] * len(names)), [f"w{words[0]}"]
        if self.eval_type == "image":
            label = self._wrap(words[0])
            return imgs, torch.tensor(label, dtype=torch.long), len(label), [f"w{words[0]}"]
        labels = [self._wrap(w) for w in words]
        return imgs, torch.tensor(labels, dtype=torch.long), [len(l) for l in labels], [f"w{words[0]}"]


class SyntheticDataModule(MultiModalDataModule):
    """``--dataset synthetic``: same batch contract as the SAYCam module, no files needed."""

    def __init__(self, args=None, n_items: int = 64):
        super().__init__(args)
        world = int(os.environ.get("WORLD_SIZE", "1"))
        self.n_items = max(n_items, 2 * self.batch_size) * max(world, 1)          # the same number of steps per rank
        self.seed = self.args.get("seed", 0)

    def prepare_data(self, *a, **k):
        pass

    def setup(self, *a, **k):
        v = len(self.read_vocab())
        raw = self.device_frames
        self.train_set = SyntheticPairs(self.n_items, v, seed=self.seed, raw_frames=raw)
        self.val_set = SyntheticPairs(self.val_batch_size, v, seed=self.seed + 1, raw_frames=raw)
        self.test_set = SyntheticPairs(self.val_batch_size, v, seed=self.seed + 2, raw_frames=raw)
        sos_eos = bool(self.args.get("eval_include_sos_eos", False))
        et = self.args.get("eval_type", EVAL_TYPE) or EVAL_TYPE
        n_trials = int(self.args.get("n_eval_trials", 4) or 4)
        bpe = None
        if self.args.get("clip_eval", CLIP_EVAL):          # CLIP's frame statistics and tokenizer for the evaluation trials (:143-155, 256-262)
            bpe = self.args.get("clip_bpe")
            if not bpe:
                raise ValueError("clip_eval needs clip_bpe: the path of CLIP's bpe_simple_vocab_16e6.txt(.gz)")
        self.eval_sets = {"val": SyntheticEvalTrials(n_trials, v, seed=self.seed + 3, eval_include_sos_eos=sos_eos, raw_frames=raw,
                                                     eval_type=et, clip_bpe=bpe),
                          "test": SyntheticEvalTrials(n_trials, v, seed=self.seed + 4, eval_include_sos_eos=sos_eos, raw_frames=raw,
                                                      eval_type=et, clip_bpe=bpe)}

    def set_epoch(self, epoch: int):
        self._epoch = int(epoch)

    def train_dataloader(self):
        """One process per GPU: every rank reads its own shard of each global batch (DistributedSampler, as Lightning's DDP
        strategy injects into the reference's loaders) -- identical batches on every rank would make each positive a
        ``world``-fold negative of itself under global negatives."""
        sampler = None
        if torch.distributed.is_available() and torch.distributed.is_initialized() and torch.distributed.get_world_size() > 1:
            sampler = torch.utils.data.distributed.DistributedSampler(
                self.train_set, num_replicas=torch.distributed.get_world_size(), rank=torch.distributed.get_rank(),
                shuffle=False, drop_last=True)
            sampler.set_epoch(getattr(self, "_epoch", 0))
        return torch.utils.data.DataLoader(self.train_set, batch_size=self.batch_size, shuffle=False, sampler=sampler,
                                           collate_fn=multiModalDataset_collate_fn, drop_last=self.drop_last)

    def _val_test(self, pairs, trials):
        """reference val_test_dataloader (:378-403): [pair batches, one evaluation trial per batch]"""
        return [torch.utils.data.DataLoader(pairs, batch_size=self.val_batch_size, shuffle=False,
                                            collate_fn=multiModalDataset_collate_fn),
                torch.utils.data.DataLoader(trials, batch_size=1, shuffle=False, collate_fn=multiModalDataset_collate_fn)]

    def val_dataloader(self):
        return self._val_test(self.val_set, self.eval_sets["val"])

    def test_dataloader(self):
        return self._val_test(self.test_set, self.eval_sets["test"])
