"""The SAYCam-layout data module (reference multimodal_saycam_data_module.py:77-211).

It reads a dataset directory DIR (``--data_dir`` / ``$CVCL_DATA_DIR``; there is no built-in path) laid out as the reference's::

    DIR/train.json, train_shuffled.json, val.json, test.json     {"data": [{"utterance", "frame_filenames", ...}]}
    DIR/vocab.json                                               (optional: the packaged vocabulary otherwise)
    DIR/train_5fps/<frame_filename>                              224 x 224 frames
    DIR/eval_*.json                                              {"data": [{"target_img_filename", "foil_img_filenames",
                                                                            "target_category", "foil_categories"}]}

Frame paths in the evaluation metadata are used as written when absolute and resolve against DIR when relative.  The
reference's dataset preparation (transcript download, frame extraction, CLIP filtering) is not built: ``prepare_data`` does
nothing.  How a frame reaches the model (host transform, ``--device_frames``, ``--frame_store``) is multimodal_data_module's
``FrameSource``."""
import os
import random

import torch

from .frame_store import frame_key
from .multimodal_data_module import (EOS_TOKEN, SOS_TOKEN, UNK_TOKEN_ID, VOCAB_FILENAME, FrameSource, MultiModalDataModule,
                                     load_data, read_vocab)

MULTIPLE_FRAMES = False
SHUFFLE_UTTERANCES = False
TRAIN_METADATA_FILENAME = "train.json"
TRAIN_SHUFFLED_METADATA_FILENAME = "train_shuffled.json"
VAL_METADATA_FILENAME = "val.json"
TEST_METADATA_FILENAME = "test.json"


class MultiModalSAYCamDataset(torch.utils.data.Dataset):
    """Paired frames and child-directed utterances (:77-124): item = (img, token ids [L], L, [utterance]) with
    ``<sos> + utterance.split() + <eos>`` through the vocabulary (unknown words -> <unk>) and the utterance's first frame, or
    ``random.choice`` of its frames under ``multiple_frames`` (Python's generator, as the reference: a seeded run draws the same
    frames).  ``frames`` (a FrameSource) decides what ``img`` is; without one the frame is read from ``train_5fps/`` under the
    current directory and transformed on the host."""

    def __init__(self, data, vocab, multiple_frames, transform, frames=None):
        self.data, self.vocab, self.multiple_frames, self.transform = data, vocab, multiple_frames, transform
        self.frames = frames if frames is not None else FrameSource(None)
        self.frames.resolve(frame_key(n, train=True) for d in data for n in d["frame_filenames"])

    def __len__(self):
        return len(self.data)

    def __getitem__(self, idx):
        utterance = self.data[idx]["utterance"]
        words = [SOS_TOKEN] + utterance.split() + [EOS_TOKEN]
        idxs = torch.tensor([self.vocab.get(w, UNK_TOKEN_ID) for w in words], dtype=torch.long)
        names = self.data[idx]["frame_filenames"]
        name = random.choice(names) if self.multiple_frames else names[0]
        return self.frames(frame_key(name, train=True), self.transform), idxs, len(words), [utterance]


class MultiModalSAYCamDataModule(MultiModalDataModule):
    def __init__(self, args=None):
        super().__init__(args)
        self.multiple_frames = self.args.get("multiple_frames", MULTIPLE_FRAMES)
        self.shuffle_utterances = self.args.get("shuffle_utterances", SHUFFLE_UTTERANCES)
        if not self.data_dir:
            raise ValueError("the SAYCam data module needs a dataset directory: --data_dir DIR or $CVCL_DATA_DIR")

    def read_vocab(self):
        own = os.path.join(self.data_dir, "vocab.json")
        return read_vocab(own if os.path.exists(own) else VOCAB_FILENAME)

    def create_datasets(self, vocab):
        """:181-211: shuffled or matched training utterances; val / test always take the first frame and the base transform"""
        train = TRAIN_SHUFFLED_METADATA_FILENAME if self.shuffle_utterances else TRAIN_METADATA_FILENAME
        print("Training using shuffled utterances!" if self.shuffle_utterances else "Training using matched utterances!")
        datasets = {}
        for split, filename, multiple_frames, transform in (("train", train, self.multiple_frames, self.transform),
                                                            ("val", VAL_METADATA_FILENAME, False, self.base_transform),
                                                            ("test", TEST_METADATA_FILENAME, False, self.base_transform)):
            data = load_data(os.path.join(self.data_dir, filename))
            datasets[split] = MultiModalSAYCamDataset(data, vocab, multiple_frames=multiple_frames, transform=transform,
                                                      frames=self.frames)
        return datasets

    def _uses_training_transform(self, dataloader_idx, training):
        """The device-side counterpart of the transforms the datasets were built with: training batches and the evaluation
        trials (the second loader of each val / test pair) take ``self.transform``, the val / test pair loaders the base one."""
        return training or dataloader_idx % 2 == 1
