"""Write tests/golden/saycam_data.npz and saycam_data.json from the reference's own datasets (CPU, build container only).

    python tools/gen_golden_saycam_data.py [--reference DIR]

The reference's multimodal_data_module.py and multimodal_saycam_data_module.py are imported with stand-ins for the modules they
import but do not use here (torchvision, pytorch_lightning, clip, OpenCV, the Google clients, ...), pointed at a temporary
directory that holds the tiny dataset of tests/saycam_common.py (a dozen 224 x 224 frames; utterances with more than 25
tokens, an out-of-vocabulary word, several frames).  Recorded from the reference's MultiModalSAYCamDataset, LabeledSEvalDataset,
LabeledSTextEvalDataset and multiModalDataset_collate_fn: token ids and lengths of every pair item, the collated (padded,
truncated) batch of each split, the frame each training item picks under multiple_frames after random.seed(0) and
random.seed(1), and the evaluation labels and lengths with and without eval_include_sos_eos for both evaluation types.  The
dataset's metadata is written beside it (saycam_data.json) so that the tests rebuild the same dataset; frames are regenerated
from their names.  Fixed zip timestamps: re-running reproduces the archive byte for byte."""
import argparse
import hashlib
import importlib.util
import io
import json
import os
import random
import sys
import tempfile
import types
import zipfile
from pathlib import Path

import numpy as np
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
GOLDEN = os.path.join(ROOT, "tests", "golden")
sys.path.insert(0, os.path.join(ROOT, "tests"))
import saycam_common as SC  # noqa: E402


class _Anything(types.ModuleType):
    """a module whose every attribute is a do-nothing callable / base class"""

    def __getattr__(self, name):
        if name.startswith("__"):
            raise AttributeError(name)
        return type(name, (), {"__init__": lambda self, *a, **k: None, "__call__": lambda self, *a, **k: None})


def load_reference(ref_dir):
    names = ["torchvision", "torchvision.transforms", "pytorch_lightning", "clip", "cv2", "imageio", "pandas", "gsheets", "spacy",
             "googleapiclient", "googleapiclient.discovery", "google_auth_oauthlib", "google_auth_oauthlib.flow", "google",
             "google.auth", "google.auth.transport", "google.auth.transport.requests", "google.oauth2", "google.oauth2.credentials"]
    for n in names:
        sys.modules[n] = _Anything(n)
    sys.modules["torchvision"].transforms = sys.modules["torchvision.transforms"]
    pkg = types.ModuleType("multimodal")
    pkg.__path__ = []
    utils = types.ModuleType("multimodal.utils")
    utils.GaussianBlur = lambda *a, **k: None
    utils.__all__ = ["GaussianBlur"]
    sys.modules.update({"multimodal": pkg, "multimodal.utils": utils})
    mods = {}
    for name in ("multimodal_data_module", "multimodal_saycam_data_module"):
        spec = importlib.util.spec_from_file_location("multimodal." + name, os.path.join(ref_dir, "multimodal", name + ".py"))
        mod = importlib.util.module_from_spec(spec)
        sys.modules["multimodal." + name] = mod
        spec.loader.exec_module(mod)
        mods[name] = mod
    return mods["multimodal_data_module"], mods["multimodal_saycam_data_module"]


def write_npz(path, arrays):
    with zipfile.ZipFile(path, "w", compression=zipfile.ZIP_DEFLATED) as zf:
        for k in sorted(arrays):
            info = zipfile.ZipInfo(k + ".npy", date_time=(1980, 1, 1, 0, 0, 0))
            info.compress_type = zipfile.ZIP_DEFLATED
            buf = io.BytesIO()
            np.lib.format.write_array(buf, np.ascontiguousarray(arrays[k]), allow_pickle=False)
            zf.writestr(info, buf.getvalue())


def as_pixels(img):
    """the 'transform' handed to the reference: the decoded pixels themselves, CHW float (exact uint8 values)"""
    return torch.from_numpy(np.array(img, dtype=np.uint8)).permute(2, 0, 1).float()


def digest(chw):
    return hashlib.sha256(chw.to(torch.uint8).numpy().tobytes()).hexdigest()


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--reference", default=os.environ.get("CVCL_REFERENCE", "/root/reference"))
    a = ap.parse_args()
    dm, sdm = load_reference(a.reference)
    with open(os.path.join(ROOT, "multimodal-baby_amd", "multimodal", "vocab.json")) as f:
        vocab = json.load(f)
    meta = SC.metadata()
    out = {}
    with tempfile.TemporaryDirectory() as tmp:
        SC.materialize(tmp, meta)
        os.chdir(tmp)                                      # the evaluation metadata names its frames relative to the data directory
        sdm.EXTRACTED_FRAMES_DIRNAME = Path(tmp) / "train_5fps"
        from PIL import Image
        train_names, _ = SC.frame_names(meta)
        by_digest = {digest(as_pixels(Image.open(os.path.join(tmp, "train_5fps", n)).convert("RGB"))): i
                     for i, n in enumerate(train_names)}
        assert len(by_digest) == len(train_names)
        out["train_frame_names"] = np.array(train_names)
        for split in ("train", "train_shuffled", "val", "test"):
            data = dm.load_data(os.path.join(tmp, split + ".json"))
            ds = sdm.MultiModalSAYCamDataset(data, vocab, multiple_frames=False, transform=as_pixels)
            items = [ds[i] for i in range(len(ds))]
            out[f"{split}_lengths"] = np.array([it[2] for it in items], dtype=np.int64)
            out[f"{split}_ids"] = np.concatenate([it[1].numpy() for it in items]).astype(np.int64)
            out[f"{split}_frame"] = np.array([by_digest[digest(it[0])] for it in items], dtype=np.int64)
            img, idxs, length, raw = dm.multiModalDataset_collate_fn(items)
            out[f"{split}_batch_ids"], out[f"{split}_batch_lengths"] = idxs.numpy(), length.numpy()
            assert [r[0] for r in raw] == [d["utterance"] for d in data] and tuple(img.shape) == (len(ds), 3, SC.H, SC.W)
        data = dm.load_data(os.path.join(tmp, "train.json"))
        for seed in (0, 1):
            ds = sdm.MultiModalSAYCamDataset(data, vocab, multiple_frames=True, transform=as_pixels)
            random.seed(seed)
            out[f"train_multiple_frames_seed_{seed}"] = np.array([by_digest[digest(ds[i][0])] for i in range(len(ds))], dtype=np.int64)
        for stage in ("dev", "test"):
            trials = dm.load_data(os.path.join(tmp, f"eval_{stage}.json"))
            for sos_eos in (False, True):
                tag = f"eval_{stage}_sos_eos_{int(sos_eos)}"
                ds = dm.LabeledSEvalDataset(trials, vocab, as_pixels, eval_include_sos_eos=sos_eos)
                items = [ds[i] for i in range(len(ds))]
                out[f"{tag}_image_labels"] = np.stack([it[1].numpy() for it in items]).astype(np.int64)
                out[f"{tag}_image_lengths"] = np.array([it[2] for it in items], dtype=np.int64)
                for i, (it, t) in enumerate(zip(items, trials)):      # the target image first, then the foils in order
                    want = [t["target_img_filename"]] + t["foil_img_filenames"]
                    assert [digest(x) for x in it[0]] == [digest(as_pixels(Image.open(w).convert("RGB"))) for w in want]
                    assert it[3] == [t["target_category"]]
                b = dm.multiModalDataset_collate_fn(items[:1])
                out[f"{tag}_image_batch_labels"], out[f"{tag}_image_batch_lengths"] = b[1].numpy(), b[2].numpy()
                ds = dm.LabeledSTextEvalDataset(trials, vocab, as_pixels, eval_include_sos_eos=sos_eos)
                items = [ds[i] for i in range(len(ds))]
                out[f"{tag}_text_labels"] = np.stack([it[1].numpy() for it in items]).astype(np.int64)
                out[f"{tag}_text_lengths"] = np.array([it[2] for it in items], dtype=np.int64)
                b = dm.multiModalDataset_collate_fn(items[:1])
                out[f"{tag}_text_batch_labels"], out[f"{tag}_text_batch_lengths"] = b[1].numpy(), b[2].numpy()
        os.chdir(ROOT)
    write_npz(os.path.join(GOLDEN, "saycam_data.npz"), out)
    with open(os.path.join(GOLDEN, "saycam_data.json"), "w") as f:
        json.dump(meta, f, indent=1, sort_keys=True)
    print(f"wrote {os.path.join(GOLDEN, 'saycam_data.npz')}: {len(out)} arrays, and saycam_data.json")


if __name__ == "__main__":
    main()
