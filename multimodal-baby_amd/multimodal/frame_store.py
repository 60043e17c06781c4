"""The HBM-resident frame store: every decoded frame of a dataset as one uint8 [N, H, W, 3] device array.

The reference opens and decodes one image file per item inside its DataLoader workers (multimodal_saycam_data_module.py:107-122,
multimodal_data_module.py:130-138).  Here the dataset is decoded once, offline (tools/pack_frames.py), into one C-ordered
``.npy`` plus a sidecar ``PATH.json`` (``{"H", "W", "index": {key: row}}``); ``FrameStore.load`` copies the array to the device
at start-up and batches then travel as frame *indices*: ``cvcl_augment_frames_indexed`` (csrc/augment.hip) reads frame b of
a batch at ``store + index[b] * H * W * 3``, so no gathered copy of the frames is ever made.

The keys are the names the metadata files use: a training frame's name under ``train_5fps/`` is keyed ``train_5fps/<name>``;
an evaluation frame by its path as written in the metadata (``frame_key``).  There is no host-resident fallback: a store that
does not fit the free device memory is an error."""
import ctypes
import json
import os

import numpy as np
import torch

from . import _hip as H

CHUNK_BYTES = 256 << 20                      # host -> device copy granularity of load(): the only host staging there is
TRAIN_FRAMES_DIRNAME = "train_5fps"


def frame_key(name, train=False):
    """The store key of a frame named in a metadata file: train frames live under train_5fps/, evaluation frames are keyed by
    their path as written (absolute, or relative to the data directory)."""
    return f"{TRAIN_FRAMES_DIRNAME}/{name}" if train else str(name)


def frame_path(data_dir, key):
    """Where the frame of ``key`` is on disk: absolute paths as written, relative ones against the data directory."""
    return key if os.path.isabs(key) else os.path.join(str(data_dir), key)


def sidecar_path(path):
    return str(path) + ".json"


class FrameStore:
    def __init__(self, frames, index, path=None):
        if frames.dtype != torch.uint8 or frames.dim() != 4 or frames.shape[-1] != 3:
            raise H.CvclError(f"a frame store is uint8 [N, H, W, 3], got {tuple(frames.shape)} {frames.dtype}")
        self.frames = frames
        self.index = index
        self.path = path
        self.n, self.height, self.width = int(frames.shape[0]), int(frames.shape[1]), int(frames.shape[2])

    def __len__(self):
        return self.n

    @property
    def device(self):
        return self.frames.device

    @staticmethod
    def open_memmap(path):
        """(memory-mapped uint8 [N, H, W, 3] array, key -> row map) of a packed store, checked against its sidecar."""
        with open(sidecar_path(path)) as f:
            meta = json.load(f)
        arr = np.load(str(path), mmap_mode="r")
        if arr.dtype != np.uint8 or arr.ndim != 4 or arr.shape[3] != 3 or not arr.flags["C_CONTIGUOUS"]:
            raise H.CvclError(f"{path}: expected a C-ordered uint8 [N, H, W, 3] array, got {arr.dtype} {arr.shape}")
        if (arr.shape[1], arr.shape[2]) != (int(meta["H"]), int(meta["W"])) or len(meta["index"]) != arr.shape[0]:
            raise H.CvclError(f"{path}: the array {arr.shape} does not match its sidecar ({len(meta['index'])} frames of "
                              f"{meta['H']} x {meta['W']})")
        return arr, meta["index"]

    @classmethod
    def load(cls, path, device):
        """Memory-map PATH and copy it to ``device`` in chunks of at most CHUNK_BYTES: the array is never pinned or staged whole
        on the host.  A device that reports less free memory than the array needs is refused before anything is allocated."""
        arr, index = cls.open_memmap(path)
        device = torch.device(device)
        n, per = arr.shape[0], int(arr.shape[1]) * int(arr.shape[2]) * 3
        if device.type == "cuda":
            free, _total = torch.cuda.mem_get_info(device)
            if n * per > free:
                raise H.CvclError(f"{path}: the frame store needs {n * per} bytes but device {device} reports {free} free; there "
                                  "is no host-resident fallback")
        frames = torch.empty(arr.shape, dtype=torch.uint8, device=device)
        step = max(1, CHUNK_BYTES // per)
        for lo in range(0, n, step):
            hi = min(n, lo + step)
            frames[lo:hi].copy_(torch.from_numpy(np.array(arr[lo:hi])))          # one chunk read from the map into host memory
        return cls(frames, index, path=str(path))

    def index_of(self, key):
        try:
            return int(self.index[key])
        except KeyError:
            raise KeyError(f"frame {key!r} is not in the frame store{' ' + self.path if self.path else ''}") from None

    def check_index(self, index):
        """Host check of an index tensor: int64, every value in 0..N-1 (IndexError otherwise).  A device tensor is read back."""
        if not torch.is_tensor(index) or index.dtype != torch.int64:
            raise H.CvclError(f"a frame index is an int64 tensor, got {getattr(index, 'dtype', type(index))}")
        host = index.detach().cpu()
        if host.numel() and (int(host.min()) < 0 or int(host.max()) >= self.n):
            bad = host[(host < 0) | (host >= self.n)]
            raise IndexError(f"frame index {int(bad.reshape(-1)[0])} outside the store's 0..{self.n - 1}")

    def transform(self, index, augment, params=None, return_uint8=False):
        """int64 index [B] -> fp32 [B, 3, oh, ow] (and the uint8 [B, oh, ow, 3] image before ToTensor with ``return_uint8``): the
        frames ``store[index]`` through ``augment`` (a DeviceFrameAugment: its draws, sizes and statistics) in one launch.  The
        index is checked on the host before it is uploaded; no kernel is launched for a bad one."""
        self.check_index(index)
        return self._launch(index.reshape(-1).to(self.device, non_blocking=True), augment, params, return_uint8)

    def _launch(self, index_d, augment, params=None, return_uint8=False):
        """``transform`` for an index already on the device whose values the caller vouches for (the data module: every index
        its datasets emit came from ``index_of`` at setup).  No read-back, so the host keeps its lead over the device; the
        kernel clamps the index into the store whatever it holds."""
        if not self.frames.is_cuda:
            raise H.CvclError("the frame store is not on a GPU; there is no CPU pixel path")
        B = int(index_d.numel())
        if params is None:
            params = augment.sample_params(B, self.height, self.width)
        max_h = augment.check_params(params, B, self.height, self.width)
        dev = self.device
        index_d = index_d.contiguous()
        crop_d, sigma_d, flip_d = (t.to(dev, non_blocking=True) for t in (params.crop, params.sigma, params.flip))
        oh, ow = augment.size
        out = torch.empty(B, 3, oh, ow, dtype=torch.float32, device=dev)
        out8 = torch.empty(B, oh, ow, 3, dtype=torch.uint8, device=dev) if return_uint8 else None
        H.check(H.lib().cvcl_augment_frames_indexed(
            H.ptr(self.frames), self.n, H.ptr(index_d, torch.int64), B, self.height, self.width, H.ptr(crop_d), H.ptr(sigma_d),
            H.ptr(flip_d), ctypes.cast(augment.mean, ctypes.c_void_p), ctypes.cast(augment.std, ctypes.c_void_p), H.ptr(out), oh, ow,
            H.ptr(out8), max_h, H.stream_ptr()), "cvcl_augment_frames_indexed")
        return (out, out8) if return_uint8 else out
