"""CPU: tests/golden/caption_gradcam.npz (tools/gen_golden_caption_gradcam.py: the reference's gradCAM_for_captioning_lm on a stub
model) loads, has the documented shapes and step convention, holds exact zeros behind every caption's last word, exercises the ReLU
on both sides, and equals the closed form -- relu(sum_c alpha_c A_c), alpha = -(d loss / d f @ W_fc) / hw -- evaluated with plain
torch autograd in float64 on the weights rebuilt from the formula."""
import numpy as np
import pytest
import torch

import caption_gradcam_common as K
from conftest import load_golden

CASES = ("plain", "normalized")


@pytest.fixture(scope="module")
def fx():
    return load_golden("caption_gradcam")


def test_shapes_and_step_convention(fx):
    assert list(fx["cases"]) == list(CASES)
    assert fx["map"].shape == (K.B, K.C, K.HW, K.HW) and fx["map"].dtype == torch.float32
    assert fx["y"].shape == (K.B, K.L) and fx["y_len"].shape == (K.B,)
    y, n = fx["y"], fx["y_len"]
    assert int(n.max()) == K.L and int(n.min()) >= 3 and len(set(n.tolist())) > 1
    for b in range(K.B):
        assert int(y[b, 0]) == 2 and int(y[b, int(n[b]) - 1]) == 3 and bool((y[b, int(n[b]):] == 0).all())
    for c in CASES:
        # no entry for step 0 (the reference returns None there): index p is the map of predicting word p + 1
        assert fx[f"{c}.cam64"].shape == (K.B, K.L - 1, K.HW, K.HW) and fx[f"{c}.cam64"].dtype == torch.float64
        assert fx[f"{c}.cam32"].shape == (K.B, K.L - 1, K.HW, K.HW) and fx[f"{c}.cam32"].dtype == torch.float32
        dev = float(fx[f"{c}.ref32_dev"])
        assert dev == K.err(fx[f"{c}.cam32"], fx[f"{c}.cam64"]) and 0 < dev < 1e-5


def test_pad_positions_are_zero_and_relu_is_exercised(fx):
    n = fx["y_len"]
    for c in CASES:
        for key in (f"{c}.cam64", f"{c}.cam32"):
            cam = fx[key]
            inside = []
            for b in range(K.B):
                assert bool((cam[b, int(n[b]) - 1:] == 0).all()), (key, b)
                inside.append(cam[b, :int(n[b]) - 1].reshape(-1))
                for p in range(int(n[b]) - 1):
                    assert float(cam[b, p].max()) > 0, (key, b, p)          # every word of a caption has a map
            inside = torch.cat(inside)
            assert bool((inside >= 0).all())
            pos, zero = float((inside > 0).double().mean()), float((inside == 0).double().mean())
            print(f"{key}: in-caption entries positive {pos:.1%}, zero {zero:.1%}")
            assert pos >= 0.30 and zero >= 0.30, (key, pos, zero)


@pytest.mark.parametrize("case", CASES)
def test_closed_form_reproduces_the_reference(fx, case):
    w = K.toy_weights()
    A = fx["map"]
    f = A.double().mean(dim=(2, 3)) @ w["fc.weight"].double().t() + w["fc.bias"].double()
    g = K.reference_grads(f, w, fx["y"], case == "normalized")
    cams = K.reference_cams(A, g, w["fc.weight"])
    e = K.err(cams, fx[f"{case}.cam64"])
    print(f"{case}: closed form vs the reference's float64 maps {e:.2e}")
    assert e < 1e-12
    assert np.isfinite(e)
