"""CPU: cvcl_augment_frames_indexed is declared, bound and exported with the ABI at 7, and refuses every invalid argument with
CVCL_EINVAL and its message on dummy pointers, before anything is enqueued (no GPU is touched)."""
import ctypes
import os
import re

import pytest

from conftest import ROOT

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
    assert re.search(r"\bcvcl_augment_frames_indexed\s*\(", txt)
    assert "cvcl_augment_frames_indexed" in H.SIGNATURES and hasattr(H.lib(), "cvcl_augment_frames_indexed")
    assert re.search(r"#define\s+CVCL_ABI_VERSION\s+7\b", txt) and H.ABI_VERSION == 7 and H.lib().cvcl_abi_version() == 7
    assert "multimodal_saycam_data_module.py:107-122" in txt
    # the indexed entry is the plain entry's arguments with (store, n_frames, index) in place of frames
    plain, indexed = H.SIGNATURES["cvcl_augment_frames"][1], H.SIGNATURES["cvcl_augment_frames_indexed"][1]
    assert indexed[3:] == plain[1:] and indexed[1] is ctypes.c_int64
    src = open(os.path.join(ROOT, "multimodal-baby_amd", "csrc", "augment.hip")).read()
    assert len(re.findall(r"__global__", src)) == 1     # one kernel body serves both entries


def _call(H, store=FAKE, n_frames=7, index=FAKE, B=5, Hh=224, W=224, crop=FAKE, sigma=FAKE, flip=FAKE, mean=MEAN, std=STD, out=FAKE,
          out_h=224, out_w=224, max_crop_h=224):
    return H.lib().cvcl_augment_frames_indexed(store, n_frames, index, B, Hh, W, crop, sigma, flip,
                                               ctypes.cast(mean, ctypes.c_void_p) if mean else None,
                                               ctypes.cast(std, ctypes.c_void_p) if std else None, out, out_h, out_w, None, max_crop_h, None)


@pytest.mark.parametrize("kw,msg", [
    (dict(store=None), b"cvcl_augment_frames_indexed: null store / index"),
    (dict(index=None), b"cvcl_augment_frames_indexed: null store / index"),
    (dict(n_frames=0), b"cvcl_augment_frames_indexed: n_frames 0 < 1"),
    (dict(n_frames=-4), b"cvcl_augment_frames_indexed: n_frames -4 < 1"),
    (dict(crop=None), b"cvcl_augment_frames_indexed: null operand"),
    (dict(sigma=None), b"cvcl_augment_frames_indexed: null operand"),
    (dict(flip=None), b"cvcl_augment_frames_indexed: null operand"),
    (dict(mean=None), b"cvcl_augment_frames_indexed: null operand"),
    (dict(std=None), b"cvcl_augment_frames_indexed: null operand"),
    (dict(out=None), b"cvcl_augment_frames_indexed: null operand"),
    (dict(B=0), b"cvcl_augment_frames_indexed: bad sizes (B 0,"),
    (dict(B=-2), b"cvcl_augment_frames_indexed: bad sizes (B -2,"),
    (dict(Hh=0, max_crop_h=0), b"bad sizes (B 5, frame 0 x 224"),
    (dict(W=0), b"bad sizes (B 5, frame 224 x 0"),
    (dict(out_h=0), b"output 0 x 224"),
    (dict(out_w=-1), b"output 224 x -1"),
    (dict(max_crop_h=0), b"max crop height 0"),
    (dict(max_crop_h=225), b"max crop height 225"),
    (dict(Hh=4096, W=224, max_crop_h=4096), b"cvcl_augment_frames_indexed: a 4096-row crop resampled to 224 x 224 needs"),
    (dict(W=100000, out_h=8, out_w=8), b"tap horizontal filter table does not fit the plane buffer"),
])
def test_refusals(H, kw, msg):
    assert _call(H, **kw) == -1
    assert msg in H.lib().cvcl_last_error(), H.lib().cvcl_last_error()


def test_plain_entry_keeps_its_refusals(H):
    """the shared validation names the entry that was called"""
    rc = H.lib().cvcl_augment_frames(None, 5, 224, 224, FAKE, FAKE, FAKE, ctypes.cast(MEAN, ctypes.c_void_p),
                                     ctypes.cast(STD, ctypes.c_void_p), FAKE, 224, 224, None, 224, None)
    assert rc == -1 and b"cvcl_augment_frames: null operand" in H.lib().cvcl_last_error()
    rc = H.lib().cvcl_augment_frames(FAKE, 0, 224, 224, FAKE, FAKE, FAKE, ctypes.cast(MEAN, ctypes.c_void_p),
                                     ctypes.cast(STD, ctypes.c_void_p), FAKE, 224, 224, None, 224, None)
    assert rc == -1 and b"cvcl_augment_frames: bad sizes (B 0," in H.lib().cvcl_last_error()
