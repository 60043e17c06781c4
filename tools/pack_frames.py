"""Decode every frame of a SAYCam-layout dataset once into a frame store (multimodal/frame_store.py).

    python tools/pack_frames.py --data_dir DIR --out PATH [--eval_metadata eval_dev.json eval_test.json ...] [--workers 16]

Reads the frames named by DIR/train.json, train_shuffled.json, val.json and test.json (those that exist) and by the given
evaluation metadata files, decodes each distinct frame once with Pillow (``convert("RGB")``) and writes them into one C-ordered
uint8 [N, H, W, 3] ``.npy`` through ``numpy.lib.format.open_memmap`` -- the array is never held in RAM -- plus the sidecar
``PATH.json`` with the key -> row map and H, W.  Every frame must have the size of the first one (the reference's extractor
writes 224 x 224, multimodal_saycam_data_module.py:511-542): a frame of another size is an error that names the file."""
import argparse
import json
import multiprocessing
import os
import sys

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(ROOT, "multimodal-baby_amd"))
from multimodal.frame_store import frame_key, frame_path, sidecar_path  # noqa: E402

PAIR_FILES = ("train.json", "train_shuffled.json", "val.json", "test.json")
MAX_WORKERS = 16


def collect_keys(data_dir, eval_metadata=()):
    """The distinct frame keys of the dataset, in first-seen order."""
    keys = {}
    for name in PAIR_FILES:
        path = os.path.join(data_dir, name)
        if not os.path.exists(path):
            continue
        with open(path) as f:
            for item in json.load(f)["data"]:
                for n in item["frame_filenames"]:
                    keys.setdefault(frame_key(n, train=True))
    for name in eval_metadata:
        with open(name if os.path.isabs(name) else os.path.join(data_dir, name)) as f:
            for trial in json.load(f)["data"]:
                for n in [trial["target_img_filename"]] + list(trial["foil_img_filenames"]):
                    keys.setdefault(frame_key(n))
    return list(keys)


def decode(path):
    from PIL import Image
    with Image.open(path) as im:
        return np.array(im.convert("RGB"), dtype=np.uint8)


def _pack_rows(job):
    """one worker's share: decode rows lo..hi straight into the memory-mapped array"""
    out, paths, lo, shape = job
    arr = np.load(out, mmap_mode="r+")
    for i, path in enumerate(paths):
        a = decode(path)
        if a.shape != shape:
            return f"{path}: frame is {a.shape[0]} x {a.shape[1]}, the store holds {shape[0]} x {shape[1]} frames"
        arr[lo + i] = a
    arr.flush()
    return None


def pack(data_dir, out, eval_metadata=(), workers=MAX_WORKERS):
    keys = collect_keys(data_dir, eval_metadata)
    if not keys:
        raise SystemExit(f"{data_dir}: no frames named by {', '.join(PAIR_FILES)} or the evaluation metadata")
    paths = [frame_path(data_dir, k) for k in keys]
    shape = decode(paths[0]).shape
    n = len(keys)
    arr = np.lib.format.open_memmap(out, mode="w+", dtype=np.uint8, shape=(n,) + shape)
    arr.flush()
    del arr
    workers = max(1, min(int(workers), MAX_WORKERS, n))
    step = max(1, min(1024, -(-n // workers)))
    jobs = [(out, paths[lo:lo + step], lo, shape) for lo in range(0, n, step)]
    if workers == 1:
        errors = [_pack_rows(j) for j in jobs]
    else:
        with multiprocessing.get_context("spawn").Pool(workers) as pool:
            errors = pool.map(_pack_rows, jobs)
    errors = [e for e in errors if e]
    if errors:
        os.remove(out)
        raise SystemExit(errors[0])
    with open(sidecar_path(out), "w") as f:
        json.dump({"H": int(shape[0]), "W": int(shape[1]), "index": {k: i for i, k in enumerate(keys)}}, f)
    return n, shape


def main(argv=None):
    ap = argparse.ArgumentParser(description=__doc__.split("\n")[0])
    ap.add_argument("--data_dir", default=os.environ.get("CVCL_DATA_DIR"), required="CVCL_DATA_DIR" not in os.environ)
    ap.add_argument("--out", required=True, metavar="PATH", help="the .npy to write (its sidecar is PATH.json)")
    ap.add_argument("--eval_metadata", nargs="*", default=[], help="evaluation metadata files (relative to the data directory)")
    ap.add_argument("--workers", type=int, default=MAX_WORKERS, help=f"decoding processes (at most {MAX_WORKERS})")
    a = ap.parse_args(argv)
    n, shape = pack(a.data_dir, a.out, a.eval_metadata, a.workers)
    print(f"wrote {a.out}: {n} frames of {shape[0]} x {shape[1]} ({n * shape[0] * shape[1] * 3 / 1e9:.2f} GB) and {sidecar_path(a.out)}")


if __name__ == "__main__":
    main()
