"""GPU: the ViT's attention rollout (csrc/vit_maps.hip cvcl_attention_head_fuse, csrc/vit_rollout.hip cvcl_attention_rollout,
multimodal/vit_maps.py attention_rollout) against its float64 restatement.  The reference's ViT has no rollout; the definition is

    F_l = fuse_h softmax(q k^T scale)[h],  A^_l = (F_l + I) / rowsum(F_l + I),  R = A^_L . A^_{L-1} ... A^_{s+1}   (first q_rows rows)

Bounds.  tau = 4 x the worst error of torch's own fp32 CPU evaluation of the same expression against float64 on the same inputs,
computed inside the test (the rule of tests/test_vit_attention_gpu.py).  For the fuse kernel the error is absolute (every element is
a probability); for the chain and the whole model it is taken relative to the largest element of its row of R (after 12 layers the
elements of a row are all near 1 / T).  bf16 model: 2 x the deviation of torch CPU autocast(bfloat16) from its own fp32 run.  Row
sums: T 2^-23 for F (mean), n_layers T 2^-23 for R.  Every case prints its bound and the measured error before it asserts; the
figures measured on an MI355X are in DESIGN.md section 9 "ViT attention rollout"."""
import contextlib
import functools
import io
import json
from functools import partial

import numpy as np
import pytest
import torch

import vit_attention_common as VC
from conftest import load_golden, maxrel

pytestmark = pytest.mark.gpu

FUSIONS = ("mean", "max", "min")
#         (B, heads, T, head_dim)
SHAPES = [(3, 3, 33, 64),           # partial query and key tiles on the MFMA route
          (2, 12, 197, 64),         # the product shape
          (2, 6, 257, 64),          # crosses the 128-query and 64-key tile edges by one
          (2, 4, 17, 16)]           # VALU route


def _fuse(P, fusion):
    """[B, heads, T, T] -> [B, T, T]."""
    return P.mean(1) if fusion == "mean" else (P.max(1).values if fusion == "max" else P.min(1).values)


def _chain(Fs, start_layer=0, q_rows=None):
    """Fs: the fused matrices [B, T, T] in block order, any dtype -> the first q_rows rows of A^_last ... A^_start_layer."""
    eye = torch.eye(Fs[0].shape[-1], dtype=Fs[0].dtype)
    R = None
    for Fl in Fs[start_layer:]:
        A = Fl + eye
        A = A / A.sum(-1, keepdim=True)
        R = A if R is None else A @ R
    return R if q_rows is None else R[:, :q_rows]


def _row_rel(got, ref64):
    """Worst |got - ref| over the largest element of the row of ref."""
    return float(((got.double() - ref64).abs() / ref64.abs().amax(-1, keepdim=True)).max())


def _qkv(B, heads, T, hd, dtype, seed):
    qkv = torch.randn(B, T, 3, heads, hd, generator=torch.Generator().manual_seed(seed)).reshape(B * T, 3 * heads * hd)
    return qkv.to(dtype).contiguous()                      # bf16: the rounded values ARE the inputs


# ---- cvcl_attention_head_fuse ------------------------------------------------------------------------------------------------

@pytest.mark.parametrize("dtype", [torch.float32, torch.bfloat16], ids=["f32", "bf16"])
@pytest.mark.parametrize("B,heads,T,hd", SHAPES)
def test_head_fuse_vs_float64(dev, dtype, B, heads, T, hd):
    from multimodal import vit_maps
    scale = hd ** -0.5
    qkv = _qkv(B, heads, T, hd, dtype, seed=T + heads)
    p64 = VC.softmax_probs(qkv.double(), B, T, heads, hd, scale)
    p32 = VC.softmax_probs(qkv.float(), B, T, heads, hd, scale)            # torch's fp32 CPU evaluation of the same inputs
    qd = qkv.to(dev)
    probs = vit_maps.attention_probs(qd, B, T, heads, hd, scale, T)
    res = []
    for fusion in FUSIONS:
        ref64 = _fuse(p64, fusion)
        tau = VC.tau(_fuse(p32, fusion), ref64)
        n = B * T * T
        buf = torch.full((n + 1024,), -7.0, dtype=torch.float32, device=dev)
        got = vit_maps.attention_head_fuse(qd, B, T, heads, hd, scale, fusion, out=buf[:n].view(B, T, T))
        assert bool((buf[n:] == -7.0).all()), "written past [B][T][T]"
        err = float((got.double().cpu() - ref64).abs().max())
        again = vit_maps.attention_head_fuse(qd, B, T, heads, hd, scale, fusion)
        same = torch.equal(again, got)
        line = f"[fuse {fusion} {dtype}] B {B} heads {heads} T {T} hd {hd}: tau {tau:.3e}, kernel error {err:.3e}, second call bit-equal {same}"
        rowsum = pair = None
        if fusion == "mean":
            rowsum = float((got.double().sum(-1) - 1).abs().max())
            pair = float((got.double() - probs.double().mean(1)).abs().max())
            line += f", row sums off 1 by {rowsum:.3e} (bound {T * 2.0 ** -23:.3e}), vs head mean of cvcl_attention_probs {pair:.3e}"
        print(line)
        res.append((fusion, tau, err, same, rowsum, pair))
    for fusion, tau, err, same, rowsum, pair in res:
        assert err <= tau, (fusion, err, tau)
        assert same, fusion
        if fusion == "mean":
            assert rowsum <= T * 2.0 ** -23, rowsum
            assert pair <= tau, (pair, tau)


# ---- cvcl_attention_rollout --------------------------------------------------------------------------------------------------

@functools.lru_cache(maxsize=None)
def _fused_inputs(n_layers, T):
    """Row-stochastic F (the softmax of unit-variance scores: rowsum(F + I) = 2) and the max / min over 3 such heads (rowsum != 2),
    B = 2, with the float64 and torch-fp32-CPU chains of every start layer the tests use."""
    B, heads = 2, 3
    g = torch.Generator().manual_seed(100 * n_layers + T)
    P = torch.randn(n_layers, B, heads, T, T, generator=g).softmax(-1)
    kinds = {"mean": P[:, :, 0].contiguous(), "max": P.max(2).values.contiguous(), "min": P.min(2).values.contiguous()}
    starts = sorted({0, n_layers // 2, n_layers - 1})
    refs = {}
    for kind, Fs in kinds.items():
        for s in starts:
            refs[kind, s] = (_chain(list(Fs.double()), s), _chain(list(Fs), s))
    return kinds, starts, refs


@pytest.mark.parametrize("T", [17, 197, 257])
@pytest.mark.parametrize("n_layers", [1, 2, 12])
def test_rollout_chain_vs_float64(dev, n_layers, T):
    from multimodal import vit_maps
    kinds, starts, refs = _fused_inputs(n_layers, T)
    assert float((kinds["max"].sum(-1) - 1).abs().min()) > 1e-3 and float((kinds["min"].sum(-1) - 1).abs().min()) > 1e-3
    res = []
    for kind, Fs in kinds.items():
        Fd = Fs.to(dev)
        for s in starts:
            ref64, ref32 = refs[kind, s]
            tau = 4 * _row_rel(ref32, ref64)
            full = vit_maps.rollout_chain(Fd, s, T)
            for q_rows in (1, 7, T):
                got = full if q_rows == T else vit_maps.rollout_chain(Fd, s, q_rows)
                assert got.shape == (2, q_rows, T) and got.dtype == torch.float32
                err = _row_rel(got.cpu(), ref64[:, :q_rows])
                rowsum = float((got.double().sum(-1) - 1).abs().max())
                bit = torch.equal(got, full[:, :q_rows])
                print(f"[chain {kind}] layers {n_layers} T {T} start {s} q_rows {q_rows}: tau {tau:.3e}, kernel error {err:.3e}, "
                      f"row sums off 1 by {rowsum:.3e} (bound {n_layers * T * 2.0 ** -23:.3e}), rows of q_rows = T bit-equal {bit}")
                res.append((kind, s, q_rows, tau, err, rowsum, bit))
            assert torch.equal(vit_maps.rollout_chain(Fd, s, 1), full[:, :1])          # a second call
    for kind, s, q_rows, tau, err, rowsum, bit in res:
        assert err <= tau, (kind, s, q_rows, err, tau)
        assert rowsum <= n_layers * T * 2.0 ** -23, (kind, s, q_rows, rowsum)
        assert bit, (kind, s, q_rows)


# ---- the model's methods on the toy ViT ----------------------------------------------------------------------------------------

def _tiny(dev):
    from multimodal import vision_transformer_dino_mugs as vits
    g = load_golden("vit_tiny")
    sd = {k[2:]: v for k, v in g.items() if k.startswith("w.")}
    m = vits.VisionTransformer(img_size=[32], patch_size=8, embed_dim=32, depth=2, num_heads=2, mlp_ratio=4, qkv_bias=True,
                               norm_layer=partial(torch.nn.LayerNorm, eps=1e-6))
    m.load_state_dict(sd)
    for p in m.parameters():
        p.requires_grad_(False)
    return m.to(dev).eval(), sd


def _model_rollout(sd, x, fusion, start_layer):
    """The rollout of the whole toy model in the dtype of ``sd`` / under the ambient autocast: VC._walk's attention per block."""
    Fs = [_fuse(attn.to(sd["cls_token"].dtype), fusion) for _, _, attn, _ in VC._walk(sd, x, 8, 2, 1e-6)]
    with torch.autocast("cpu", enabled=False):              # the chain itself is fp32 in the product's bf16 mode as well
        return _chain(Fs, start_layer)


def _toy_inputs():
    gt, gi = load_golden("vit_tiny"), load_golden("vit_tiny_interp")
    return (("native", gt["x"]), ("resampled", gi["x_a"]))


def test_model_rollout_vs_float64(dev):
    m, sd = _tiny(dev)
    sd64 = VC.to_dtype(sd, torch.float64)
    res = []
    for tag, x in _toy_inputs():
        T = (x.shape[2] // 8) * (x.shape[3] // 8) + 1
        for fusion, s in (("mean", 0), ("max", 0), ("min", 1), ("mean", 1)):
            with torch.no_grad():
                ref64, ref32 = _model_rollout(sd64, x.double(), fusion, s), _model_rollout(sd, x, fusion, s)
            tau = 4 * _row_rel(ref32, ref64)
            got = m.get_attention_rollout(x.to(dev), head_fusion=fusion, start_layer=s, q_rows=T)
            assert got.shape == (x.shape[0], T, T) and got.dtype == torch.float32
            err = _row_rel(got.cpu(), ref64)
            print(f"[toy ViT {tag} {tuple(x.shape)}] {fusion} start {s}: tau {tau:.3e}, error {err:.3e}")
            res.append((tag, fusion, s, tau, err))
            cls = m.get_attention_rollout(x.to(dev), head_fusion=fusion, start_layer=s)
            assert cls.shape == (x.shape[0], 1, T) and torch.equal(cls, got[:, :1])
    for tag, fusion, s, tau, err in res:
        assert err <= tau, (tag, fusion, s, err, tau)


def test_model_rollout_bf16_vs_own_fp32(dev):
    m, sd = _tiny(dev)
    res = []
    for tag, x in _toy_inputs():
        T = (x.shape[2] // 8) * (x.shape[3] // 8) + 1
        with torch.no_grad():
            r32 = _model_rollout(sd, x, "mean", 0)
            with torch.autocast("cpu", dtype=torch.bfloat16):
                r16 = _model_rollout(sd, x, "mean", 0)
        yard = float((r16.double() - r32.double()).abs().max())
        xd = x.to(dev)
        want = m.get_attention_rollout(xd, q_rows=T)
        m.compute_dtype = torch.bfloat16
        try:
            got = m.get_attention_rollout(xd, q_rows=T)
        finally:
            m.compute_dtype = torch.float32
        err = float((got.double() - want.double()).abs().max())
        print(f"[toy ViT {tag} bf16] rollout vs own fp32: {err:.3e}; torch autocast(bf16) vs its fp32: {yard:.3e} -> bound {2 * yard:.3e}")
        res.append((got.dtype, err, yard))
    for dt, err, yard in res:
        assert dt == torch.float32 and err <= 2 * yard, (err, yard)


def test_chunked_equals_unchunked_and_forward_untouched(dev):
    from multimodal import attention_maps as A
    from multimodal import vit_maps
    m, _ = _tiny(dev)
    x = torch.randn(5, 3, 32, 32, generator=torch.Generator().manual_seed(11)).to(dev)
    T = 17
    before = m(x).clone()
    whole, grid = vit_maps.attention_rollout(m, x, "mean", 0, T)
    per_image = 2 * T * T * 4
    for budget in (2 * per_image, 1):                       # chunks of 2, 2, 1 images; a budget below one image: one by one
        part, _ = vit_maps.attention_rollout(m, x, "mean", 0, T, slab_bytes=budget)
        assert torch.equal(part, whole), budget
    assert grid == (4, 4) and whole.shape == (5, T, T)
    maps = A.vit_attention_rollout(m, x)
    assert maps.shape == (5, 4, 4) and torch.equal(maps, whole[:, 0, 1:].reshape(5, 4, 4))
    big = A.vit_attention_rollout(m, x, size=(32, 32))
    assert big.shape == (5, 32, 32) and torch.equal(big, A.bicubic_resize(maps, (32, 32)))
    for fusion in ("max", "min"):
        other = A.vit_attention_rollout(m, x, head_fusion=fusion, start_layer=1)
        assert other.shape == (5, 4, 4) and not torch.equal(other, maps)
    after = m(x).clone()
    torch.cuda.synchronize()
    assert torch.equal(before, after)
    enc = torch.nn.Module()                                 # a VisionEncoder wrapper is accepted as well
    enc.model = m
    assert torch.equal(A.vit_attention_rollout(enc, x), maps)


# ---- eval.py --attention_rollout ---------------------------------------------------------------------------------------------

def _patched_vit():
    from multimodal import vision_transformer_dino_mugs as vits
    return lambda name, pretrained: vits.VisionTransformer(img_size=[224], patch_size=16, embed_dim=768, depth=2, num_heads=12, mlp_ratio=4,
                                                           qkv_bias=True, num_classes=0, norm_layer=partial(torch.nn.LayerNorm, eps=1e-6))


def test_eval_attention_rollout(dev, tmp_path, monkeypatch):
    """eval.py --attention_maps DIR --attention_rollout on a synthetic ViT checkpoint: cams.npy [trials, 4, gh, gw] holds the rollout
    maps (finite, non-negative, each summing to 1 - R[0, 0]), the prediction records are those of a run without the flags, and the
    maps are not the plain CLS maps; MultiModalLitModel.self_attention_maps(rollout=True) returns forward()'s logits bit for bit."""
    import eval as ev
    import train
    import multimodal.multimodal as mm
    from multimodal import attention_maps as A
    from multimodal.multimodal_data_module import SyntheticEvalTrials
    from multimodal.multimodal_lit import MultiModalLitModel
    monkeypatch.chdir(tmp_path)
    monkeypatch.setattr(mm, "load_model", _patched_vit())
    exp = "multimodal_text_encoder_embedding_pretrained_cnn_False_finetune_cnn_False_seed_0"
    argv = ("--dataset synthetic --batch_size 4 --val_batch_size 4 --gpus 1 --text_encoder embedding --embedding_dim 32 --vit_dino "
            "--lambda_lm 0 --optimize_unused --max_epochs 1 --limit_train_batches 2 --normalize_features "
            f"--checkpoint_callback True --logger False --exp_name {exp}").split()
    with contextlib.redirect_stdout(io.StringIO()):
        train.main(argv)
        lit = MultiModalLitModel.load_from_checkpoint(ev.resolve_checkpoint(exp), map_location=dev).to(dev).eval()
    trials = SyntheticEvalTrials(6, 2350, seed=0 + 4, eval_type="image")
    imgs, label, n, _ = trials[0]
    imgs, tok, ln = imgs.to(dev), label.view(1, -1).to(dev), torch.tensor([n], device=dev)
    with torch.no_grad():
        lpi, lpt = lit(imgs, tok, ln)
        lpi2, lpt2, maps = lit.self_attention_maps(imgs, tok, ln, rollout=True)
        assert torch.equal(lpi, lpi2) and torch.equal(lpt, lpt2)
        assert maps.shape == (4, 14, 14) and torch.equal(maps, A.vit_attention_rollout(lit.vision_encoder, imgs))
        plain_maps = lit.self_attention_maps(imgs, tok, ln)[2]
        assert torch.equal(plain_maps, A.vit_cls_attention(lit.vision_encoder, imgs))
    base = ["--checkpoint", exp, "--eval_dataset", "synthetic", "--eval_type", "image", "--n_trials", "6", "--trial_batch", "4"]
    d, d_cls = tmp_path / "rollout", tmp_path / "cls"
    with contextlib.redirect_stdout(io.StringIO()):
        plain = ev.main(ev._parser().parse_args(base))
        rolled = ev.main(ev._parser().parse_args(base + ["--attention_maps", str(d), "--attention_rollout"]))
        ev.main(ev._parser().parse_args(base + ["--attention_maps", str(d_cls)]))
    assert json.dumps(plain) == json.dumps(rolled)
    cams, cls = np.load(d / "cams.npy"), np.load(d_cls / "cams.npy")
    assert cams.shape == (6, 4, 14, 14) and cams.dtype == np.float32
    assert np.isfinite(cams).all() and (cams >= 0).all()
    assert cls.shape == cams.shape and not np.allclose(cams, cls, rtol=1e-2, atol=0)
    vit = lit.vision_encoder.model
    for i in range(6):
        R = vit.get_attention_rollout(trials[i][0].to(dev))                          # [4, 1, 197]
        want = 1.0 - R[:, 0, 0].double().cpu().numpy()
        got = cams[i].astype(np.float64).sum((-2, -1))
        assert np.abs(got - want).max() <= 1e-5, (i, got, want)      # (other batch size: the GEMMs may tile differently)
        assert maxrel(torch.from_numpy(cams[i]), R[:, 0, 1:].reshape(4, 14, 14)) <= 1e-5, i
    with pytest.raises(SystemExit, match="--attention_maps"):
        ev.main(ev._parser().parse_args(base + ["--attention_rollout"]))
