"""CPU: the map-faithfulness entries (csrc/faithfulness.hip) are declared, bound and exported at ABI 7 without a new struct, refuse
every invalid argument with CVCL_EINVAL on dummy pointers before anything reaches a GPU, and the wrappers of
multimodal/map_faithfulness.py refuse CPU tensors."""
import os
import re

import numpy as np
import pytest
import torch

from conftest import ROOT

ENTRIES = {"cvcl_map_ranks_scratch_bytes": 2, "cvcl_map_ranks": 7, "cvcl_map_perturb": 15, "cvcl_gaussian_blur_f32": 9,
           "cvcl_pair_dot": 8, "cvcl_curve_auc": 7}
FAKE = 0x10000                                          # 16-byte aligned, never dereferenced: validation fails first


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


def test_entries_declared_bound_exported_at_abi_7(H):
    txt = open(os.path.join(ROOT, "include", "cvcl_hip.h")).read()
    assert re.search(r"#define CVCL_ABI_VERSION 7\b", txt)
    lib = H.lib()
    assert lib.cvcl_abi_version() == 7 == H.ABI_VERSION and len(H.STRUCTS) == 3
    for name, n_args in ENTRIES.items():
        assert re.search(rf"\b{name}\s*\(", txt), name
        assert name in H.SIGNATURES and len(H.SIGNATURES[name][1]) == n_args, name
        assert hasattr(lib, name), name


def _last(H, entry, msg, rc):
    assert rc == -1 == H.EINVAL
    err = H.lib().cvcl_last_error()
    assert err.startswith(entry.encode() + b": ") and msg in err, err


def _ranks(H, maps=FAKE, ranks=FAKE, M=2, HW=49, scratch=FAKE, scratch_bytes=1 << 30):
    return H.lib().cvcl_map_ranks(maps, ranks, M, HW, scratch, scratch_bytes, None)


@pytest.mark.parametrize("kw,msg", [
    (dict(maps=None), b"null pointer (maps / ranks)"),
    (dict(ranks=None), b"null pointer (maps / ranks)"),
    (dict(scratch=None), b"null pointer (scratch)"),
    (dict(HW=0), b"HW 0 is outside 1 .. 65536"),
    (dict(HW=65537), b"HW 65537 is outside 1 .. 65536"),
    (dict(M=0), b"M 0 < 1"),
    (dict(M=-2), b"M -2 < 1"),
    (dict(scratch_bytes=16), b"scratch_bytes 16 <"),
    (dict(scratch=FAKE + 4), b"not 16-byte aligned"),
])
def test_rank_refusals(H, kw, msg):
    """each returns before the launch: on a machine without a GPU a launch would fail with a runtime error instead"""
    _last(H, "cvcl_map_ranks", msg, _ranks(H, **kw))


def test_rank_scratch_query(H):
    q = H.lib().cvcl_map_ranks_scratch_bytes
    assert q(0, 49) == 0 and q(1, 0) == 0 and q(1, 65537) == 0 and q(-1, 5) == 0
    assert q(1, 1) >= 2 * (4 + 2) and q(3, 49) % 16 == 0 and q(1, 65536) == 2 * 65536 * 6
    assert 2 * 6 * 256 * 50176 <= q(256, 50176) < 2 * 8 * 256 * 50176          # two (key, 16-bit index) buffers
    _last(H, "cvcl_map_ranks", b"scratch_bytes", _ranks(H, scratch_bytes=q(2, 49) - 1))
    _last(H, "cvcl_map_ranks", b"not 16-byte aligned", _ranks(H, scratch_bytes=q(2, 49), scratch=FAKE + 8))


def _perturb(H, images=FAKE, baseline=None, ranks=FAKE, iom=(1, 0, 1), item_map=(0, 1, 2), item_count=(0, 10, 63), item_mode=(0, 1, 0),
             n_items=None, N=2, M=3, C=3, Hh=7, Ww=9, out=FAKE):
    arr = [None if v is None else np.asarray(v, dtype=np.int32) for v in (iom, item_map, item_count, item_mode)]
    p = [None if a is None else a.ctypes.data for a in arr]
    n = len(item_map) if n_items is None else n_items
    return H.lib().cvcl_map_perturb(images, baseline, ranks, p[0], p[1], p[2], p[3], n, N, M, C, Hh, Ww, out, None)


@pytest.mark.parametrize("kw,msg", [
    (dict(images=None), b"null pointer (images / ranks / out)"),
    (dict(ranks=None), b"null pointer (images / ranks / out)"),
    (dict(out=None), b"null pointer (images / ranks / out)"),
    (dict(item_map=None, n_items=3), b"null pointer (item_map / item_count / item_mode)"),
    (dict(item_count=None), b"null pointer (item_map / item_count / item_mode)"),
    (dict(item_mode=None), b"null pointer (item_map / item_count / item_mode)"),
    (dict(n_items=0), b"must be positive"),
    (dict(M=0), b"must be positive"),
    (dict(Hh=0), b"is outside 1 .. 65536 pixels"),
    (dict(Hh=257, Ww=256), b"is outside 1 .. 65536 pixels"),
    (dict(iom=None), b"without image_of_map map m lies over image m, but M 3 > N 2"),
    (dict(iom=(1, 2, 0)), b"image_of_map[1] = 2 is outside 0 .. 1"),
    (dict(iom=(-1, 0, 0)), b"image_of_map[0] = -1 is outside 0 .. 1"),
    (dict(item_map=(0, 3, 2)), b"item_map[1] = 3 is outside 0 .. 2"),
    (dict(item_map=(0, 1, -1)), b"item_map[2] = -1 is outside 0 .. 2"),
    (dict(item_count=(0, 10, 64)), b"item_count[2] = 64 is outside 0 .. 63"),
    (dict(item_count=(-1, 10, 63)), b"item_count[0] = -1 is outside 0 .. 63"),
    (dict(item_mode=(0, 2, 0)), b"item_mode[1] = 2 outside {0, 1}"),
])
def test_perturb_refusals(H, kw, msg):
    _last(H, "cvcl_map_perturb", msg, _perturb(H, **kw))


def _blur(H, x=FAKE, y=FAKE + 64, w=(0.25, 0.5, 0.25), k=None, planes=2, Hh=7, Ww=9, scratch=FAKE + 128):
    wa = None if w is None else np.asarray(w, dtype=np.float32)
    return H.lib().cvcl_gaussian_blur_f32(x, y, None if wa is None else wa.ctypes.data, len(w) if k is None else k, planes, Hh, Ww,
                                          scratch, None)


@pytest.mark.parametrize("kw,msg", [
    (dict(x=None), b"null pointer"),
    (dict(y=None), b"null pointer"),
    (dict(w=None, k=3), b"null pointer"),
    (dict(scratch=None), b"null pointer"),
    (dict(planes=0), b"must be positive"),
    (dict(w=(0.5, 0.5)), b"k 2 is not a positive odd number"),
    (dict(w=(0.25,) * 4), b"k 4 is not a positive odd number"),
    (dict(k=0), b"k 0 is not a positive odd number"),
    (dict(w=(1 / 131,) * 131), b"k 131 > 129"),
    (dict(w=(1 / 15,) * 15), b"the radius k / 2 = 7 does not lie below min(H, W) = 7"),
    (dict(w=(0.2,) * 5, Hh=9, Ww=2), b"the radius k / 2 = 2 does not lie below min(H, W) = 2"),
    (dict(y=FAKE), b"must be distinct"),
    (dict(scratch=FAKE), b"must be distinct"),
])
def test_blur_refusals(H, kw, msg):
    _last(H, "cvcl_gaussian_blur_f32", msg, _blur(H, **kw))


def test_pair_dot_and_auc_refusals(H):
    lib = H.lib()
    for args in ((None, FAKE, FAKE, FAKE, 4, 2, 8), (FAKE, None, FAKE, FAKE, 4, 2, 8), (FAKE, FAKE, None, FAKE, 4, 2, 8),
                 (FAKE, FAKE, FAKE, None, 4, 2, 8)):
        _last(H, "cvcl_pair_dot", b"null pointer", lib.cvcl_pair_dot(*args, None))
    for args in ((FAKE, FAKE, FAKE, FAKE, 0, 2, 8), (FAKE, FAKE, FAKE, FAKE, 4, 0, 8), (FAKE, FAKE, FAKE, FAKE, 4, 2, 0)):
        _last(H, "cvcl_pair_dot", b"must be positive", lib.cvcl_pair_dot(*args, None))
    for args in ((None, FAKE, FAKE, 2, 4, 3), (FAKE, None, FAKE, 2, 4, 3), (FAKE, FAKE, None, 2, 4, 3)):
        _last(H, "cvcl_curve_auc", b"null pointer", lib.cvcl_curve_auc(*args, None))
    for args in ((FAKE, FAKE, FAKE, 0, 4, 3), (FAKE, FAKE, FAKE, 2, 0, 3), (FAKE, FAKE, FAKE, 2, 4, 0)):
        _last(H, "cvcl_curve_auc", b"must be positive", lib.cvcl_curve_auc(*args, None))


def test_every_wrapper_refuses_cpu_tensors(H):
    from multimodal import map_faithfulness as F
    img, maps = torch.randn(2, 3, 7, 9), torch.rand(2, 7, 9)
    rk = torch.zeros(2, 7, 9, dtype=torch.int32)
    calls = [lambda: F.pixel_ranks(maps), lambda: F.perturb(img, None, rk, None, [0], [3], [0]), lambda: F.gaussian_blur(img, 5, 1.0),
             lambda: F.pair_dot(torch.randn(4, 8), torch.randn(2, 8), torch.zeros(4, dtype=torch.int32)),
             lambda: F.curve_auc(torch.randn(2, 5, 3), torch.linspace(0, 1, 5)),
             lambda: F.deletion_insertion(None, img, torch.randn(2, 8), maps),
             lambda: F.maps_of(None, img, None, None, "random")]
    for call in calls:
        with pytest.raises(H.CvclError, match="no CPU fallback"):
            call()
    assert np.isclose(F.gaussian_weights(11, 5.0).astype(np.float64).sum(), 1.0, atol=1e-6) and F.gaussian_weights(11, 5.0).dtype == np.float32
