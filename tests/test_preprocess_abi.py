"""CPU: cvcl_preprocess_frames is declared, bound and exported with the ABI at 7, refuses every invalid argument with CVCL_EINVAL and
its message on dummy pointers without touching a GPU, and MultiModalLitModel.load_model hands out a DevicePreprocess."""
import ctypes
import gzip
import os
import re
import shutil

import numpy as np
import pytest

from conftest import GOLDEN, ROOT

FAKE = 0x10000                                          # never dereferenced: validation fails first
MEAN = (ctypes.c_float * 3)(0.485, 0.456, 0.406)
STD = (ctypes.c_float * 3)(0.229, 0.224, 0.225)


@pytest.fixture(scope="module")
def H():
    import importlib.util
    spec = importlib.util.spec_from_file_location("cvcl_build", os.path.join(ROOT, "multimodal-baby_amd", "build.py"))
    b = importlib.util.module_from_spec(spec)
    spec.loader.exec_module(b)
    b.build(verbose=False)
    from multimodal import _hip
    _hip.load()
    return _hip


def test_entry_declared_bound_exported(H):
    txt = open(os.path.join(ROOT, "include", "cvcl_hip.h")).read()
    assert re.search(r"\bcvcl_preprocess_frames\s*\(", txt)
    assert "cvcl_preprocess_frames" in H.SIGNATURES and hasattr(H.lib(), "cvcl_preprocess_frames")
    assert re.search(r"#define\s+CVCL_ABI_VERSION\s+7\b", txt) and H.ABI_VERSION == 7 and H.lib().cvcl_abi_version() == 7
    m = re.search(r"#define\s+CVCL_PREPROCESS_TABLE_COLS\s+(\d+)", txt)
    from multimodal.preprocess import TABLE_COLS
    assert m and int(m.group(1)) == TABLE_COLS
    for cite in ("multimodal_lit.py:143-147", "embeddings.py:32-37", "generate_attention_maps.py:63-67",
                 "object_categories_data_module.py:49-52, 106-109", "multimodal_data_module.py:259-266",
                 "object_categories_data_module.py:38-45"):
        assert cite in txt, cite


def _call(H, rows=((0, 480, 640, 224, 224, 0, 0),), frames=FAKE, frames_bytes=1 << 40, table=True, table_dev=FAKE, B=None, mean=MEAN,
          std=STD, out=FAKE, out_h=224, out_w=224):
    t = np.array(rows, dtype=np.int64).reshape(-1, 7)
    return H.lib().cvcl_preprocess_frames(frames, frames_bytes, t.ctypes.data if table else None, table_dev, len(t) if B is None else B,
                                          ctypes.cast(mean, ctypes.c_void_p) if mean else None,
                                          ctypes.cast(std, ctypes.c_void_p) if std else None, out, out_h, out_w, None, None)


@pytest.mark.parametrize("kw,msg", [
    (dict(frames=None), b"null pointer (frames / table / table_dev)"),
    (dict(table=False), b"null pointer (frames / table / table_dev)"),
    (dict(table_dev=None), b"null pointer (frames / table / table_dev)"),
    (dict(mean=None), b"null pointer (mean / std)"),
    (dict(std=None), b"null pointer (mean / std)"),
    (dict(out=None), b"null pointer (out)"),
    (dict(B=0), b"B 0 outside 1..65535"),
    (dict(B=-3), b"B -3 outside 1..65535"),
    (dict(out_h=0), b"output 0 x 224 outside 1..1024"),
    (dict(out_w=1025), b"output 224 x 1025 outside 1..1024"),
    (dict(rows=[(0, 0, 640, 224, 224, 0, 0)]), b"frame 0: source 0 x 640 outside 1..4096"),
    (dict(rows=[(0, 480, 640, 224, 224, 0, 0), (921600, 480, 4097, 224, 224, 0, 0)]), b"frame 1: source 480 x 4097 outside 1..4096"),
    (dict(rows=[(0, 480, 640, 0, 224, 0, 0)]), b"frame 0: resized 0 x 224 outside 1..65536"),
    (dict(rows=[(0, 480, 640, 224, 65537, 0, 0)]), b"frame 0: resized 224 x 65537 outside 1..65536"),
    (dict(rows=[(0, 480, 640, 224, 298, 0, 75)]), b"frame 0: the 224 x 224 window at (0, 75) leaves the 224 x 298 resized image"),
    (dict(rows=[(0, 480, 640, 224, 298, -1, 37)]), b"window at (-1, 37) leaves"),
    (dict(rows=[(0, 480, 640, 223, 298, 0, 37)]), b"window at (0, 37) leaves the 223 x 298"),
    (dict(rows=[(-1, 480, 640, 224, 224, 0, 0)]), b"frame 0: bytes -1..921599 outside"),
    (dict(rows=[(0, 480, 640, 224, 224, 0, 0)], frames_bytes=921599), b"frame 0: bytes 0..921600 outside the 921599-byte buffer"),
    (dict(rows=[(0, 4096, 4096, 1, 1024, 0, 0)], out_h=1, out_w=1024), b"a 16385-tap filter at output width 1024 needs"),
])
def test_refusals(H, kw, msg):
    assert _call(H, **kw) == -1
    assert msg in H.lib().cvcl_last_error(), H.lib().cvcl_last_error()


def test_python_layer_refusals(H):
    import torch
    from multimodal.preprocess import DevicePreprocess
    pre = DevicePreprocess()
    for bad in (np.zeros((4, 4), dtype=np.uint8), np.zeros((4, 4, 3), dtype=np.float32), torch.zeros(4, 4, 4, dtype=torch.uint8), "x"):
        with pytest.raises(H.CvclError, match="uint8"):
            pre(bad)
    with pytest.raises(H.CvclError, match="uint8"):
        pre(torch.zeros(2, 8, 8, 3))
    with pytest.raises(H.CvclError, match="no frames"):
        pre([])


def test_load_model_returns_device_preprocess(tmp_path):
    from multimodal.clip_model import CLIP_MEAN, clip_preprocess
    from multimodal.multimodal_lit import MultiModalLitModel
    from multimodal.preprocess import DevicePreprocess
    dst = tmp_path / "ref_lit_vit.ckpt"
    with gzip.open(os.path.join(GOLDEN, "ref_lit_vit.ckpt.gz"), "rb") as fi, open(dst, "wb") as fo:
        shutil.copyfileobj(fi, fo)
    _lit, pre = MultiModalLitModel.load_model("cvcl", checkpoint_path=str(dst))
    assert isinstance(pre, DevicePreprocess) and pre.size == 224 and pre.mode == "stretch"
    assert [round(float(v), 3) for v in pre.mean] == [0.485, 0.456, 0.406] and [round(float(v), 3) for v in pre.std] == [0.229, 0.224, 0.225]
    clip = clip_preprocess()
    assert isinstance(clip, DevicePreprocess) and clip.mode == "shorter_side_center_crop"
    assert [float(v) for v in clip.mean] == [float(np.float32(v)) for v in CLIP_MEAN]
