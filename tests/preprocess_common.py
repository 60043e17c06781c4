"""Numpy restatement of the evaluation-time transform (Pillow's bicubic resize, the crop window, ToTensor + Normalize), shared by the
preprocess tests -- TEST INFRASTRUCTURE ONLY; the product path is csrc/preprocess.hip behind cvcl_preprocess_frames.

Written from Pillow's published algorithm (libImaging/Resample.c): ``precompute_coeffs`` with the bicubic filter (Keys, a = -0.5,
support 2, widened by the down-scale factor), ``normalize_coeffs_8bpc`` (coefficients normalised in double, rounded to 22 fractional
bits, -0.5 for negative weights), a horizontal pass then a vertical pass, each started at 1 << 21, shifted right by 22 and clamped to
uint8; a pass whose size does not change is skipped.  Pinned against Pillow itself by tests/golden/preprocess_pil.npz
(tools/gen_golden_preprocess.py) and, where Pillow is importable, against the live library (tests/test_preprocess_oracle.py)."""
import math

import numpy as np

PRECISION_BITS = 32 - 8 - 2
IMAGENET_MEAN, IMAGENET_STD = (0.485, 0.456, 0.406), (0.229, 0.224, 0.225)
CLIP_MEAN, CLIP_STD = (0.48145466, 0.4578275, 0.40821073), (0.26862954, 0.26130258, 0.27577711)


def bicubic_filter(x):
    a = -0.5
    x = abs(x)
    if x < 1.0:
        return ((a + 2.0) * x - (a + 3.0)) * x * x + 1
    if x < 2.0:
        return (((x - 5) * x + 8) * x - 4) * a
    return 0.0


def bicubic_coeffs(in_size, out_size, first=0, count=None):
    """Output indices first .. first + count of an in_size -> out_size pass: (bounds [count][2] = (first tap, tap count),
    coefficients [count][ksize] int32 with 22 fractional bits)."""
    count = out_size - first if count is None else count
    scale = in_size / out_size
    filterscale = max(scale, 1.0)
    support = 2.0 * filterscale
    ksize = int(math.ceil(support)) * 2 + 1
    ss = 1.0 / filterscale
    bounds = np.zeros((count, 2), dtype=np.int32)
    kk = np.zeros((count, ksize), dtype=np.int32)
    for i in range(count):
        center = (first + i + 0.5) * scale
        xmin = max(int(center - support + 0.5), 0)
        xmax = min(int(center + support + 0.5), in_size) - xmin
        k = [bicubic_filter((x + xmin - center + 0.5) * ss) for x in range(xmax)]
        ww = 0.0
        for w in k:
            ww += w
        for x in range(xmax):
            w = k[x] / ww if ww != 0.0 else k[x]
            kk[i, x] = int(w * (1 << PRECISION_BITS) + (-0.5 if w < 0 else 0.5))     # C cast truncates toward zero
        bounds[i] = (xmin, xmax)
    return bounds, kk


def _resample_axis0(img, out_size, first, count):
    """Rows first .. first + count of the bicubic pass along axis 0 of a [n][...] uint8 array"""
    bounds, kk = bicubic_coeffs(img.shape[0], out_size, first, count)
    out = np.empty((count,) + img.shape[1:], dtype=np.uint8)
    src = img.astype(np.int64)
    for i in range(count):
        xmin, xmax = (int(v) for v in bounds[i])
        acc = np.tensordot(kk[i, :xmax].astype(np.int64), src[xmin:xmin + xmax], axes=1) + (1 << (PRECISION_BITS - 1))
        out[i] = np.clip(acc >> PRECISION_BITS, 0, 255).astype(np.uint8)
    return out


def resize_window_u8(img, rh, rw, ct, cl, out_h, out_w):
    """The out_h x out_w window at (ct, cl) of Image.resize((rw, rh), BICUBIC) of img (uint8 [H][W][3]): horizontal pass, then
    vertical pass.  Output pixels are independent, so computing the window alone is resize-then-crop."""
    H, W = img.shape[:2]
    assert 0 <= ct and ct + out_h <= rh and 0 <= cl and cl + out_w <= rw
    if rw != W:
        img = _resample_axis0(img.transpose(1, 0, 2), rw, cl, out_w).transpose(1, 0, 2)
    else:
        img = img[:, cl:cl + out_w]
    if rh != H:
        img = _resample_axis0(img, rh, ct, out_h)
    else:
        img = img[ct:ct + out_h]
    return np.ascontiguousarray(img)


def to_tensor_normalize(img_u8, mean=IMAGENET_MEAN, std=IMAGENET_STD):
    """ToTensor + Normalize: uint8 [H][W][3] -> fp32 [3][H][W], (x / 255 - mean) / std with every operation in fp32"""
    x = img_u8.transpose(2, 0, 1).astype(np.float32) / np.float32(255.0)
    mean, std = np.asarray(mean, dtype=np.float32), np.asarray(std, dtype=np.float32)
    return ((x - mean[:, None, None]) / std[:, None, None]).astype(np.float32)


def hard_frame(seed, height, width, cell=1):
    """Hard-edged 0 / 255 frame: augment_oracle.synthetic_frame's uniform noise on a grid of cell x cell blocks, thresholded at 127.
    Blocks wider than the filter keep flat 0 and 255 areas through a down-scale, and the cubic's overshoot at their edges runs
    into the clamp of both passes on both sides."""
    import augment_oracle as A
    ch, cw = -(-height // cell), -(-width // cell)
    coarse = np.where(A.synthetic_frame(seed, ch, cw, smooth=False) > 127, 255, 0).astype(np.uint8)
    return np.ascontiguousarray(np.repeat(np.repeat(coarse, cell, axis=0), cell, axis=1)[:height, :width])


def case_frame(seed, height, width, cell):
    """the input of a golden case: cell == 0 is a smooth frame, otherwise a hard-edged one of that block size"""
    import augment_oracle as A
    return A.synthetic_frame(seed, height, width, smooth=True) if cell == 0 else hard_frame(seed, height, width, cell)


def mode_stats(mode):
    """the normalisation each mode is used with in the reference: ImageNet's for the stretch, CLIP's for the centre crop"""
    return (IMAGENET_MEAN, IMAGENET_STD) if mode == "stretch" else (CLIP_MEAN, CLIP_STD)
