"""Generates tests/golden/preprocess_pil.npz: outputs of Pillow itself (the library the reference's evaluation transform runs on,
multimodal_lit.py:143-147 and multimodal_data_module.py:259-266) for fixed frames.  TEST INFRASTRUCTURE; the fixture holds data only.

    python tools/gen_golden_preprocess.py

Each case applies ``Image.resize((rw, rh), BICUBIC)`` and ``Image.crop`` of the size x size window, with the geometry of
``multimodal.preprocess.resize_geometry`` (Resize((224, 224)) for the stretch; Resize(224) + CenterCrop(224) for the crop).  The
inputs are rebuilt from their seed (tests/preprocess_common.case_frame: oracle/augment_oracle.synthetic_frame, thresholded on a
block grid for the hard-edged kind), the outputs are stored as CRC-32 for all cases, in full for two small ones, and one case carries
the first 16 rows of ToTensor + Normalize computed with torch's own fp32 operations.  The zip members carry a fixed timestamp, so a
re-run reproduces the file byte for byte."""
import io
import os
import sys
import zipfile
import zlib

import numpy as np
import PIL
import torch
from PIL import Image

ROOT = os.path.join(os.path.dirname(os.path.abspath(__file__)), "..")
for p in ("tests", "oracle", "multimodal-baby_amd"):
    sys.path.insert(0, os.path.join(ROOT, p))
import preprocess_common as P  # noqa: E402  (only for the test inputs)
from multimodal.preprocess import MODES, resize_geometry  # noqa: E402

OUT = os.path.join(ROOT, "tests", "golden", "preprocess_pil.npz")
SIZE = 224
# (H, W, mode, cell: 0 = smooth frame, n = hard-edged 0 / 255 blocks of n x n pixels)
CASES = [
    (224, 224, "stretch", 0),                    # identity: both passes skipped
    (224, 224, "shorter_side_center_crop", 1),
    (240, 320, "stretch", 0),
    (240, 320, "shorter_side_center_crop", 6),   # vertical pass only just down, horizontal crop window
    (100, 75, "stretch", 1),                     # up-scaling of single-pixel noise
    (100, 75, "shorter_side_center_crop", 0),
    (225, 223, "stretch", 0),                    # one pass barely down, one barely up
    (225, 223, "shorter_side_center_crop", 3),
    (7, 5, "stretch", 1),
    (7, 5, "shorter_side_center_crop", 0),
    (300, 60, "stretch", 0),
    (300, 60, "shorter_side_center_crop", 2),    # window far inside a 1120-row resized image
    (224, 301, "shorter_side_center_crop", 0),   # no resize, crop origin 38 (half to even)
    (480, 640, "stretch", 0),
    (480, 640, "shorter_side_center_crop", 12),
    (640, 480, "shorter_side_center_crop", 0),
    (1080, 1920, "stretch", 40),                 # 35 / 21 taps, many bands
    (1080, 1920, "shorter_side_center_crop", 0),
]
FULL = (4, 8)                                    # cases stored in full
TENSOR = 15                                      # case whose normalised tensor is stored (first 16 rows)


def main():
    out = {"pillow_version": np.array(PIL.__version__), "n_cases": np.array(len(CASES)), "size": np.array(SIZE)}
    saturated = 0
    for i, (H, W, mode, cell) in enumerate(CASES):
        img = P.case_frame(2000 + i, H, W, cell)
        rh, rw, ct, cl = resize_geometry(H, W, SIZE, mode)
        pil = Image.fromarray(img)
        if (rw, rh) != pil.size:
            pil = pil.resize((rw, rh), Image.BICUBIC)
        u8 = np.asarray(pil.crop((cl, ct, cl + SIZE, ct + SIZE))).copy()
        assert u8.shape == (SIZE, SIZE, 3)
        if cell:
            assert (u8 == 0).any() and (u8 == 255).any(), f"case {i}: hard-edged frame without pixels saturated at both ends"
            saturated += int(((u8 == 0) | (u8 == 255)).sum())
        out[f"case{i}"] = np.array([H, W, MODES.index(mode), cell, 2000 + i], dtype=np.int32)
        out[f"frame_crc{i}"] = np.array(zlib.crc32(img.tobytes()), dtype=np.uint32)
        out[f"geometry{i}"] = np.array([rh, rw, ct, cl], dtype=np.int32)
        out[f"u8_crc{i}"] = np.array(zlib.crc32(u8.tobytes()), dtype=np.uint32)
        if i in FULL:
            out[f"u8_{i}"] = u8
        if i == TENSOR:     # ToTensor (uint8 -> float / 255, CHW) + Normalize (sub mean, div std) with torch's fp32 arithmetic
            mean, std = P.mode_stats(mode)
            t = torch.from_numpy(u8).permute(2, 0, 1).contiguous().to(torch.float32).div(255)
            t = t.sub_(torch.tensor(mean).view(3, 1, 1)).div_(torch.tensor(std).view(3, 1, 1))
            out[f"tensor{i}_rows0_16"] = t[:, :16].contiguous().numpy()
    with zipfile.ZipFile(OUT, "w", zipfile.ZIP_DEFLATED, compresslevel=9) as z:
        for name, a in out.items():
            buf = io.BytesIO()
            np.lib.format.write_array(buf, np.asanyarray(a), allow_pickle=False)
            z.writestr(zipfile.ZipInfo(name + ".npy", date_time=(1980, 1, 1, 0, 0, 0)), buf.getvalue(), zipfile.ZIP_DEFLATED, 9)
    print("wrote", OUT, os.path.getsize(OUT) // 1024, "KiB;", saturated, "saturated pixels in the hard-edged cases")


if __name__ == "__main__":
    main()
