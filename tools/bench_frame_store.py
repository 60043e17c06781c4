"""Real-data input path probe: frames/s into a ready [256, 3, 224, 224] device batch by each of the three frame paths, and the
indexed transform launch against the plain one.

    python tools/bench_frame_store.py [--files 2048] [--steps 24] [--warmup 4] [--workers 16] [--json OUT]

Needs nothing from outside: it synthesises JPEG frames into a temporary directory with Pillow, builds the SAYCam dataset over
them and packs them into a frame store (tools/pack_frames.py).  Measured, each over ``steps`` batches of 256 after ``warmup``:
  (a) host     workers decode + transform on the host (fp32 batch), then the copy to the device
  (b) device   --device_frames: workers decode (uint8 batch), copy, cvcl_augment_frames on the device
  (c) store    --frame_store: the loader yields indices, cvcl_augment_frames_indexed reads the HBM-resident store
and, as single launches alternated by tools/timing.py, cvcl_augment_frames_indexed on 256 scattered rows of the store against
cvcl_augment_frames on the same 256 frames gathered into a contiguous batch, for the identity transform and the
--augment_frames draws.  Worker processes are spawned, not forked, so none of them holds the GPU open."""
import argparse
import json
import os
import random
import sys
import tempfile
import time

import numpy as np
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(ROOT, "multimodal-baby_amd"))
sys.path.insert(0, os.path.join(ROOT, "tools"))
import pack_frames  # noqa: E402
import timing  # noqa: E402
from multimodal.augment import DeviceFrameAugment  # noqa: E402
from multimodal.frame_store import FrameStore  # noqa: E402
from multimodal.multimodal_data_module import FrameSource, HostFrameTransform, multiModalDataset_collate_fn, read_vocab  # noqa: E402
from multimodal.multimodal_saycam_data_module import MultiModalSAYCamDataset  # noqa: E402

BATCH = 256


def synthesise(root, n_files, seed=0):
    """n_files JPEG frames of 224 x 224 (smooth colour fields plus noise, so that they compress like camera frames rather than
    like noise) and a train.json naming each once"""
    from PIL import Image
    rng = np.random.default_rng(seed)
    os.makedirs(os.path.join(root, "train_5fps"))
    yy, xx = np.mgrid[0:224, 0:224].astype(np.float32) / 224.0
    names = []
    for i in range(n_files):
        c = rng.uniform(0, 255, (3, 3)).astype(np.float32)
        img = c[:, 0, None, None] * yy + c[:, 1, None, None] * xx + c[:, 2, None, None] * (1 - yy * xx)
        img = np.clip(img.transpose(1, 2, 0) / 1.5 + rng.normal(0, 6, (224, 224, 3)), 0, 255).astype(np.uint8)
        names.append(f"f{i:06d}.jpg")
        Image.fromarray(img).save(os.path.join(root, "train_5fps", names[-1]), quality=90)
    with open(os.path.join(root, "train.json"), "w") as f:
        json.dump({"data": [{"utterance": "look at the ball", "frame_filenames": [n]} for n in names]}, f)
    return names


def loader(dataset, workers):
    return torch.utils.data.DataLoader(dataset, batch_size=BATCH, shuffle=True, drop_last=True, num_workers=workers,
                                       collate_fn=multiModalDataset_collate_fn, pin_memory=False,
                                       multiprocessing_context="spawn" if workers else None)


def feed_rate(dl, to_batch, warmup, steps, dev):
    """frames/s over ``steps`` batches once ``warmup`` batches have passed; every batch ends as fp32 [256, 3, 224, 224] on the device"""
    n, t0 = 0, None
    for i, batch in enumerate(dl):
        out = to_batch(batch[0])
        assert out.shape == (BATCH, 3, 224, 224) and out.dtype == torch.float32 and out.is_cuda
        if i + 1 == warmup:
            torch.cuda.synchronize(dev)
            t0 = time.perf_counter()
        elif i + 1 > warmup:
            n += BATCH
        if i + 1 == warmup + steps:
            break
    torch.cuda.synchronize(dev)
    return n / (time.perf_counter() - t0)


def launch_pair(store, aug, params, index, gathered, reps):
    """device time (us) of the indexed and the plain launch: single launches, alternated"""
    idx_d = index.to(store.device)
    t = timing.measure({"indexed": lambda: store._launch(idx_d, aug, params), "plain": lambda: aug(gathered, params)},
                       calls=1, repeats=reps, warmup=5)
    return {k: {"median_us": r["ms"] * 1e3, "min_us": r["min_ms"] * 1e3, "max_us": r["max_ms"] * 1e3,
                "p90_us": sorted(r["samples"])[int(0.9 * reps)] * 1e3} for k, r in t.items()}


def main(argv=None):
    ap = argparse.ArgumentParser()
    ap.add_argument("--files", type=int, default=2048, help="distinct JPEG frames synthesised (the datasets cycle over them)")
    ap.add_argument("--steps", type=int, default=24)
    ap.add_argument("--warmup", type=int, default=4)
    ap.add_argument("--workers", type=int, default=16)
    ap.add_argument("--reps", type=int, default=200, help="alternations of the two launches")
    ap.add_argument("--json", default=None, help="also write the result here")
    a = ap.parse_args(argv)
    if not torch.cuda.is_available():
        raise SystemExit("bench_frame_store.py measures on the GPU; none is visible")
    dev = torch.device("cuda:0")
    res = {"batch": BATCH, "files": a.files, "steps": a.steps, "warmup": a.warmup, "workers": a.workers}
    with tempfile.TemporaryDirectory() as root:
        t0 = time.perf_counter()
        names = synthesise(root, a.files)
        res["synthesise_s"] = time.perf_counter() - t0
        items = (a.warmup + a.steps) * BATCH
        data = [{"utterance": "look at the ball", "frame_filenames": [names[i % len(names)]]} for i in range(items)]
        vocab = read_vocab()
        t0 = time.perf_counter()
        store_path = os.path.join(root, "frames.npy")
        pack_frames.pack(root, store_path, [], workers=a.workers)
        res["pack_s"] = time.perf_counter() - t0
        t0 = time.perf_counter()
        store = FrameStore.load(store_path, dev)
        torch.cuda.synchronize(dev)
        res["load_s"], res["store_bytes"] = time.perf_counter() - t0, store.frames.numel()
        base = DeviceFrameAugment(augment_frames=False)

        host = MultiModalSAYCamDataset(data, vocab, False, HostFrameTransform(False), frames=FrameSource(root, "host"))
        res["host_frames_per_s"] = feed_rate(loader(host, a.workers), lambda x: x.to(dev, non_blocking=True), a.warmup, a.steps, dev)
        u8 = MultiModalSAYCamDataset(data, vocab, False, None, frames=FrameSource(root, "uint8"))
        res["device_frames_frames_per_s"] = feed_rate(loader(u8, a.workers), lambda x: base(x.to(dev, non_blocking=True)),
                                                      a.warmup, a.steps, dev)
        idx = MultiModalSAYCamDataset(data, vocab, False, None, frames=FrameSource(root, "index", store.index))
        res["frame_store_frames_per_s"] = feed_rate(loader(idx, 0), lambda x: store._launch(x.to(dev, non_blocking=True), base),
                                                    a.warmup, a.steps, dev)

        g = torch.Generator().manual_seed(0)
        index = torch.randperm(len(store), generator=g)[:BATCH].contiguous()           # 256 scattered rows of the store
        gathered = store.frames.index_select(0, index.to(dev)).contiguous()
        random.seed(0)
        aug = DeviceFrameAugment(augment_frames=True, generator=torch.Generator().manual_seed(0))
        for name, tf, params in (("identity", base, base.sample_params(BATCH, 224, 224)), ("augment", aug, aug.sample_params(BATCH, 224, 224))):
            assert torch.equal(store._launch(index.to(dev), tf, params), tf(gathered, params))
            res[f"launch_{name}"] = launch_pair(store, tf, params, index, gathered, a.reps)
    line = json.dumps(res)
    print(line)
    if a.json:
        os.makedirs(os.path.dirname(os.path.abspath(a.json)), exist_ok=True)
        with open(a.json, "w") as f:
            f.write(line + "\n")


if __name__ == "__main__":
    main()
