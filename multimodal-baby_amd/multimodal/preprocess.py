"""Evaluation-time image preprocessing on the device.

Host-side mirror of the PIL transform every evaluation entry point of the reference applies to an image before the encoder::

    transforms.Compose([                                                   # multimodal_lit.py:143-147 (load_model's `preprocess`),
        transforms.Resize((224, 224), interpolation=BICUBIC),              # analysis_cvcl/alignment.py, embeddings.py:32-37,
        transforms.ToTensor(),                                             # generate_attention_maps.py:63-67,
        transforms.Normalize(IMAGENET_MEAN, IMAGENET_STD)])                # object_categories_data_module.py:49-52, 106-109

    transforms.Compose([                                                   # CLIP's: multimodal_data_module.py:259-266,
        transforms.Resize(224, interpolation=BICUBIC),                     # object_categories_data_module.py:38-45
        transforms.CenterCrop(224),
        transforms.ToTensor(),
        transforms.Normalize(CLIP_MEAN, CLIP_STD)])

The first is ``mode="stretch"``, the second ``mode="shorter_side_center_crop"``.  Decoding (and ``convert("RGB")``) stays on the
host; the host also works out each frame's geometry (``resize_geometry``: a few integers per frame, torchvision's rules).  Every
pixel operation runs in one launch of ``cvcl_preprocess_frames`` (csrc/preprocess.hip) over the whole, possibly mixed-size, batch,
bit-identical to Pillow's bicubic resize and torch's ToTensor / Normalize.  There is no CPU pixel path: without the HIP library
the call fails.
"""
import ctypes

import numpy as np
import torch

from . import _hip as H
from .augment import IMAGENET_MEAN, IMAGENET_STD

MODES = ("stretch", "shorter_side_center_crop")
TABLE_COLS = H.PREPROCESS_TABLE_COLS                 # offset, H, W, rh, rw, ct, cl


def resize_geometry(height, width, size, mode):
    """(rh, rw, ct, cl): the size the frame is resized to and the origin of the size x size window inside it.

    ``stretch``: Resize((size, size)), the whole image.  ``shorter_side_center_crop``: torchvision's Resize(size) -- the shorter
    side becomes ``size``, the longer ``int(size * long / short)``, nothing is resized when the shorter side is ``size`` already --
    then CenterCrop(size), whose origin is ``int(round((dim - size) / 2.0))`` (Python's round: halves go to the even integer)."""
    if mode == "stretch":
        return size, size, 0, 0
    if mode != "shorter_side_center_crop":
        raise ValueError(f"mode {mode!r}: one of {MODES}")
    short, long = (width, height) if width <= height else (height, width)
    new_long = long if short == size else int(size * long / short)
    rw, rh = (size, new_long) if width <= height else (new_long, size)
    return rh, rw, int(round((rh - size) / 2.0)), int(round((rw - size) / 2.0))


def _as_hwc_u8(img):
    """one image -> a contiguous uint8 [H, W, 3] tensor where it lives (a PIL image is decoded to RGB on the host)"""
    if hasattr(img, "convert") and not torch.is_tensor(img):
        img = np.array(img.convert("RGB"), dtype=np.uint8)            # (a copy: PIL hands out a read-only view)
    if isinstance(img, np.ndarray):
        img = torch.from_numpy(np.ascontiguousarray(img))
    if not torch.is_tensor(img) or img.dtype != torch.uint8 or img.dim() != 3 or img.shape[-1] != 3:
        what = f"{tuple(img.shape)} {img.dtype}" if torch.is_tensor(img) else type(img).__name__
        raise H.CvclError(f"expected a PIL image or a uint8 [H, W, 3] array / tensor, got {what}")
    return img.contiguous()


class DevicePreprocess:
    """``preprocess(images)``: a PIL image, a uint8 HWC numpy array or tensor, a list of these (sizes may differ) or a uint8
    [B, H, W, 3] tensor -> normalised fp32 frames on the device: [3, size, size] for a single image (so the reference's
    ``preprocess(img).unsqueeze(0)`` works), [B, 3, size, size] for a batch.  ``return_uint8=True`` adds the uint8
    [.., size, size, 3] image before ToTensor."""

    def __init__(self, size=224, mode="stretch", mean=IMAGENET_MEAN, std=IMAGENET_STD, device=None):
        if mode not in MODES:
            raise ValueError(f"mode {mode!r}: one of {MODES}")
        self.size, self.mode = int(size), mode
        self.mean = (ctypes.c_float * 3)(*mean)
        self.std = (ctypes.c_float * 3)(*std)
        self.device = device

    def _pack(self, frames):
        """-> (one flat uint8 device buffer, [(H, W)] per frame); host frames are joined first and uploaded once"""
        sizes = [(int(f.shape[0]), int(f.shape[1])) for f in frames]
        dev = next((f.device for f in frames if f.is_cuda), None) or torch.device(self.device or "cuda")
        if all(not f.is_cuda for f in frames):
            return torch.cat([f.reshape(-1) for f in frames]).to(dev), sizes
        return torch.cat([f.to(dev).reshape(-1) for f in frames]), sizes

    def plan(self, images):
        """-> (packed uint8 device buffer, host table int64 [n, TABLE_COLS], its device copy): everything but the launch"""
        if torch.is_tensor(images):
            if images.dtype != torch.uint8 or images.dim() != 4 or images.shape[-1] != 3:
                raise H.CvclError(f"expected uint8 [B, H, W, 3] frames, got {tuple(images.shape)} {images.dtype}")
            sizes = [(int(images.shape[1]), int(images.shape[2]))] * images.shape[0]
            packed = images.contiguous().reshape(-1)
            packed = packed if packed.is_cuda else packed.to(torch.device(self.device or "cuda"))
        else:
            packed, sizes = self._pack([_as_hwc_u8(im) for im in images]) if len(images) else (None, [])
        if not sizes:
            raise H.CvclError("no frames to preprocess")
        table = np.empty((len(sizes), TABLE_COLS), dtype=np.int64)
        offset = 0
        for i, (h, w) in enumerate(sizes):
            table[i] = (offset, h, w) + resize_geometry(h, w, self.size, self.mode)
            offset += h * w * 3
        return packed, table, torch.from_numpy(table).to(packed.device)

    def run(self, packed, table, table_dev, return_uint8=False):
        """the launch: -> fp32 [n, 3, size, size] (and uint8 [n, size, size, 3])"""
        n, s, dev = table.shape[0], self.size, packed.device
        with torch.cuda.device(dev):
            out = torch.empty(n, 3, s, s, dtype=torch.float32, device=dev)
            out8 = torch.empty(n, s, s, 3, dtype=torch.uint8, device=dev) if return_uint8 else None
            H.check(H.lib().cvcl_preprocess_frames(H.ptr(packed), packed.numel(), table.ctypes.data, H.ptr(table_dev), n,
                                                   ctypes.cast(self.mean, ctypes.c_void_p), ctypes.cast(self.std, ctypes.c_void_p),
                                                   H.ptr(out), s, s, H.ptr(out8), H.stream_ptr()), "cvcl_preprocess_frames")
        return (out, out8) if return_uint8 else out

    def __call__(self, images, return_uint8=False):
        H.lib()
        single = not isinstance(images, (list, tuple)) and not (torch.is_tensor(images) and images.dim() == 4)
        res = self.run(*self.plan([images] if single else images), return_uint8=return_uint8)
        if single:
            return (res[0][0], res[1][0]) if return_uint8 else res[0]
        return res
