"""GPU: fine-tuning the DINO ViT in fp32 (Lightning's default precision "32"): vit_train.VitTrunk's fp32 branch against float64
autograd through the oracle (forward and every parameter gradient), bit-identical reruns, the frozen fp32 forward, train.py with no
--precision flag, and a 20-step AdamW trajectory that anchors the bf16 fine-tune to the fp32 one."""
import contextlib
import io
import os
import sys

import pytest
import torch

import cvcl_oracle as O
from conftest import ROOT, maxrel

pytestmark = pytest.mark.gpu
sys.path.insert(0, ROOT)


def _vit(dev, D, heads, depth, patch, seed):
    from multimodal import vision_transformer_dino_mugs as vits
    torch.manual_seed(seed)
    m = vits.VisionTransformer(img_size=[224], patch_size=patch, embed_dim=D, depth=depth, num_heads=heads, mlp_ratio=4, qkv_bias=True,
                               num_classes=0).to(dev)
    with torch.no_grad():                                   # non-trivial norms / biases so that every gradient is exercised
        for n, p in m.named_parameters():
            if n.endswith("bias"):
                p.normal_(0, 0.05)
            if "norm" in n and n.endswith("weight"):
                p.uniform_(0.7, 1.3)
    return m


@pytest.mark.parametrize("D,heads,depth,B,patch", [(128, 2, 2, 3, 16), (768, 12, 1, 2, 16), (128, 2, 1, 2, 14)])
def test_vit_finetune_f32_vs_float64_autograd(dev, D, heads, depth, B, patch):
    m = _vit(dev, D, heads, depth, patch, D + depth)
    m.compute_dtype = torch.float32
    x = torch.randn(B, 3, 224, 224, device=dev)
    r = torch.randn(B, D, device=dev)
    m.train()
    for p in m.parameters():
        p.requires_grad_(True)
    runs = []
    for _ in range(2):
        m.zero_grad(set_to_none=True)
        cls = m(x)
        (cls * r).sum().backward()
        runs.append({n: p.grad.detach().clone() for n, p in m.named_parameters() if p.grad is not None})
    assert all(torch.equal(runs[0][n], runs[1][n]) for n in runs[0])
    with torch.no_grad():
        for p in m.parameters():
            p.requires_grad_(False)
        frozen = m(x)
    e_frozen = maxrel(cls, frozen)
    # oracle: float64 autograd on the same weights and images
    sd = {k: v.detach().double().cpu().clone().requires_grad_(True) for k, v in m.state_dict().items()}
    yo = O.vit_forward(sd, x.double().cpu(), patch, heads, eps=m.norm.eps)      # (nn.LayerNorm default 1e-5 here)
    (yo * r.double().cpu()).sum().backward()
    e_fwd = maxrel(cls, yo)
    got = runs[0]
    names = [n for n, _ in m.named_parameters()]
    assert set(got) == set(names), set(names) - set(got)
    worst = (0.0, "")
    for n in names:
        a, b = got[n].double().cpu().flatten(), sd[n].grad.flatten()
        e = float((a - b).norm() / (b.norm() + 1e-300))
        worst = max(worst, (e, n))
    print(f"D {D} heads {heads} depth {depth} B {B} patch {patch}: forward max-rel {e_fwd:.2e} (vs frozen {e_frozen:.2e}), "
          f"worst gradient rel-L2 {worst[0]:.2e} ({worst[1]})")
    # measured: forward <= 1.7e-6, worst gradient 1.2e-6 (ViT-B width); bf16 storage sits at ~1e-2 on both
    assert e_fwd < 1e-5 and e_frozen < 1e-5
    assert worst[0] < 1.5e-5, worst


def test_vit_finetune_f32_through_train_entry(dev, tmp_path, monkeypatch):
    """The reference's fine-tuning command line with no --precision flag (Lightning's default "32"): every trunk parameter moves
    and a checkpoint is written and reloads."""
    import train
    import multimodal.multimodal as mm
    from multimodal import vision_transformer_dino_mugs as vits
    monkeypatch.chdir(tmp_path)
    argv = ("--dataset synthetic --batch_size 4 --val_batch_size 4 --gpus 1 --text_encoder embedding --embedding_dim 32 "
            "--lambda_lm 0 --optimize_unused --max_epochs 1 --limit_train_batches 2 --normalize_features --vit_dino --finetune_cnn "
            "--checkpoint_callback True --logger False --exp_name vitft32").split()
    assert "--precision" not in argv
    orig = mm.load_model
    mm.load_model = lambda name, pretrained: vits.VisionTransformer(img_size=[224], patch_size=16, embed_dim=768, depth=2, num_heads=12,
                                                                    mlp_ratio=4, qkv_bias=True, num_classes=0)
    try:
        torch.manual_seed(0)
        ref = mm.load_model("x", False).state_dict()
        torch.manual_seed(0)
        with contextlib.redirect_stdout(io.StringIO()):
            trainer, lit = train.main(argv)
    finally:
        mm.load_model = orig
    vit = lit.vision_encoder.model
    assert vit.compute_dtype == torch.float32
    assert float(trainer.logged_metrics["val_loss"]) > 0 and torch.isfinite(torch.tensor(float(trainer.logged_metrics["val_loss"])))
    trunk = [(n, p) for n, p in vit.named_parameters() if not n.startswith("head.")]
    assert trunk
    for n, p in trunk:
        assert torch.isfinite(p).all() and not torch.equal(p.detach().cpu(), ref[n]), n          # AdamW moved every trunk parameter
    ck = tmp_path / "checkpoints" / "vitft32" / "epoch=0.ckpt"
    assert ck.exists()
    state = torch.load(ck, map_location="cpu", weights_only=False)["state_dict"]
    key = next(k for k in state if k.endswith("blocks.0.attn.qkv.weight"))
    assert torch.equal(state[key], dict(trunk)["blocks.0.attn.qkv.weight"].detach().cpu())
    missing, unexpected = lit.load_state_dict(state, strict=True), None
    assert not missing.missing_keys and not missing.unexpected_keys


def test_vit_finetune_trajectory_bf16_against_f32(dev):
    """The bf16 fine-tune's fp32 anchor: 20 AdamW steps of a small ViT (ViT-S-like width, patch 16) from the same initial weights on
    the same batches, fp32 and bf16.  Both losses decrease, and the bf16 loss stays within 1 % of the fp32 one at every step
    (measured: 0.14 %)."""
    D, heads, depth, B = 384, 6, 2, 8
    losses = {}
    torch.manual_seed(11)
    xs = [torch.randn(B, 3, 224, 224, device=dev) for _ in range(4)]
    target = torch.randn(B, 16, device=dev)
    proj = torch.randn(D, 16, device=dev) / D ** 0.5
    for dt in (torch.float32, torch.bfloat16):
        m = _vit(dev, D, heads, depth, 16, 5)
        m.compute_dtype = dt
        m.train()
        opt = torch.optim.AdamW(m.parameters(), lr=3e-4, weight_decay=0.05)
        out = []
        for step in range(20):
            opt.zero_grad(set_to_none=True)
            loss = ((m(xs[step % 4]) @ proj - target) ** 2).mean()
            loss.backward()
            opt.step()
            out.append(float(loss.detach()))
        losses[dt] = out
    f32, b16 = losses[torch.float32], losses[torch.bfloat16]
    gap = max(abs(a - b) / a for a, b in zip(f32, b16))
    print("fp32 losses", " ".join(f"{v:.4f}" for v in f32))
    print("bf16 losses", " ".join(f"{v:.4f}" for v in b16))
    print(f"largest relative gap {gap:.3e}")
    assert f32[-1] < 0.7 * f32[0] and b16[-1] < 0.7 * b16[0]
    assert gap < 0.01
