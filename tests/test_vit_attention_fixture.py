"""CPU: the float64 restatement of VisionTransformer.get_last_selfattention / get_intermediate_layers that the GPU tests use as their
reference (tests/vit_attention_common.py) against the reference's own fp32 outputs (tests/golden/vit_attention.npz, written by
tools/gen_golden_vit_attention.py from the weights and inputs of vit_tiny.npz / vit_tiny_interp.npz), at the 5e-6 relative bound
oracle/gen_golden.py holds every restatement to."""
import pytest
import torch

import vit_attention_common as VC
from conftest import load_golden, maxrel

PATCH, HEADS = 8, 2
CASES = [("", "vit_tiny", "x"), ("_a", "vit_tiny_interp", "x_a"), ("_b", "vit_tiny_interp", "x_b")]


def _weights():
    return {k[2:]: v for k, v in load_golden("vit_tiny").items() if k.startswith("w.")}


@pytest.mark.parametrize("tag,src,key", CASES)
def test_restatement_reproduces_reference_outputs(tag, src, key):
    g = load_golden("vit_attention")
    x = load_golden(src)[key]
    sd64 = VC.to_dtype(_weights(), torch.float64)
    attn = VC.last_selfattention(sd64, x.double(), PATCH, HEADS)
    want = g["attn" + tag]
    T = (x.shape[2] // PATCH) * (x.shape[3] // PATCH) + 1
    assert want.shape == (x.shape[0], HEADS, T, T) and attn.shape == want.shape
    assert maxrel(attn, want) <= 5e-6
    assert float((want.double().sum(-1) - 1).abs().max()) <= T * 2.0 ** -23
    layers = VC.intermediate_layers(sd64, x.double(), PATCH, HEADS, 2)
    assert g["layers" + tag].shape == (2, x.shape[0], T, 32) and len(layers) == 2
    for got, w in zip(layers, g["layers" + tag]):
        assert maxrel(got, w) <= 5e-6
    # n = 1 is the last entry, and its CLS rows are what forward() returns (the cls outputs stored beside the inputs)
    last = VC.intermediate_layers(sd64, x.double(), PATCH, HEADS, 1)
    assert len(last) == 1 and torch.equal(last[0], layers[-1])
    assert maxrel(last[0][:, 0], load_golden(src)["cls" + tag]) <= 5e-6


def test_fixture_holds_outputs_only():
    g = load_golden("vit_attention")
    assert sorted(g) == ["attn", "attn_a", "attn_b", "layers", "layers_a", "layers_b"]


def test_tau_rule_and_softmax_helper():
    qkv = torch.randn(2 * 5, 3 * 2 * 4, generator=torch.Generator().manual_seed(0))
    p = VC.softmax_probs(qkv.double(), 2, 5, 2, 4, 0.5)
    assert p.shape == (2, 2, 5, 5) and float((p.sum(-1) - 1).abs().max()) < 1e-12
    assert torch.equal(VC.softmax_probs(qkv.double(), 2, 5, 2, 4, 0.5, q_rows=1), p[:, :, :1])
    assert VC.tau(p.float(), p) == 4.0 * float((p.float().double() - p).abs().max())
