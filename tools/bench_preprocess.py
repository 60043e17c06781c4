"""The evaluation-time transform on the device (cvcl_preprocess_frames) at 256 frames of 480 x 640 and at a mixed-size batch, in both
modes, vs Pillow on one host core.      python tools/bench_preprocess.py [--batch 256] [--cpu-frames 32] [--repeats 7] [--window-ms 200]"""
import argparse
import os
import sys
import time

import numpy as np
import torch

import timing

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(ROOT, "multimodal-baby_amd"))
from multimodal.preprocess import MODES, DevicePreprocess, resize_geometry  # noqa: E402

MIXED = [(480, 640), (640, 480), (224, 224), (240, 320), (720, 1280), (1080, 1920), (100, 75), (333, 500)]      # H x W, cycled

ap = argparse.ArgumentParser()
ap.add_argument("--batch", type=int, default=256)
ap.add_argument("--cpu-frames", type=int, default=32)
timing.add_arguments(ap)
a = ap.parse_args()
dev = torch.device("cuda:0")
g = torch.Generator().manual_seed(0)
try:
    from PIL import Image
except ImportError:
    Image = None
    print("Pillow not importable: no host column")


def pillow_ms_per_frame(frames, mode):
    """Image.resize + crop + ToTensor + Normalize per frame on one host core, as a DataLoader worker runs them"""
    torch.set_num_threads(1)
    mean, std = torch.tensor(pre.mean[:]).view(3, 1, 1), torch.tensor(pre.std[:]).view(3, 1, 1)
    t0 = time.perf_counter()
    for f in frames:
        h, w = f.shape[:2]
        rh, rw, ct, cl = resize_geometry(h, w, 224, mode)
        im = Image.fromarray(f)
        im = im if (rw, rh) == im.size else im.resize((rw, rh), Image.BICUBIC)
        im = im.crop((cl, ct, cl + 224, ct + 224))
        torch.from_numpy(np.asarray(im).copy()).permute(2, 0, 1).float().div(255).sub_(mean).div_(std)
    return (time.perf_counter() - t0) / len(frames) * 1e3


for name, sizes in (("480 x 640", [(480, 640)] * a.batch), ("mixed sizes", [MIXED[i % len(MIXED)] for i in range(a.batch)])):
    host = [torch.randint(0, 256, (h, w, 3), dtype=torch.uint8, generator=g) for h, w in sizes]
    frames = [f.to(dev) for f in host]
    src_bytes = sum(h * w * 3 for h, w in sizes)
    out_bytes = a.batch * 3 * 224 * 224 * 4
    for mode in MODES:
        pre = DevicePreprocess(mode=mode)
        plan = pre.plan(frames)
        t = timing.measure({"run": lambda: pre.run(*plan)}, **timing.keywords(a))["run"]
        ms = t["ms"]
        t0 = time.perf_counter()
        for _ in range(5):
            pre(frames)
        torch.cuda.synchronize()
        call_ms = (time.perf_counter() - t0) / 5 * 1e3
        line = (f"{name:12s} {mode:26s} {timing.text(t, 1e3, '.0f'):>20s} us per batch of {a.batch} ({(src_bytes + out_bytes) / ms / 1e6:6.0f} GB/s of source + "
                f"output bytes); whole call with packing {a.batch} device frames and the table {call_ms:.2f} ms")
        if Image is not None:
            line += f"; Pillow + torch on one host core {pillow_ms_per_frame([f.numpy() for f in host[:a.cpu_frames]], mode):.2f} ms per frame"
        print(line, flush=True)
