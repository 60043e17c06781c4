"""GPU: the discard_ratio variant of the ViT attention rollout (csrc/vit_discard.hip cvcl_attention_discard, multimodal/vit_maps.py
attention_discard and attention_rollout(discard_ratio=...)).  The reference's ViT has no rollout; the definition is the one of
tests/vit_discard_common.py: per fused matrix the k = int(T T discard_ratio) smallest elements (stable order, flat index 0 kept but
counted) become +0.0 before  A^_l = (F_l + I) / rowsum(F_l + I)  is chained.

The selection is checked EXACTLY (torch.equal with discard_ref, second call bit-equal, guard elements intact).  The chain after the
discard and the whole toy model are checked with the bound of tests/test_vit_rollout_gpu.py: tau = 4 x the error of torch's own fp32
CPU evaluation of the same expression against float64, relative to the largest element of the row.  The toy-model cases compare with
a float64 run that takes its mask from its OWN float64 F, which is fair only where rounding cannot move an element across the cut, so
each case first asserts, on the references alone, that the gap between the k-th and (k+1)-th order statistic of every float64 F is at
least 16 x the fp32 error of F.  Every case prints its bound and the measured error before it asserts; the figures measured on an
MI355X are in DESIGN.md section 9 "ViT attention rollout"."""
import contextlib
import functools
import io
import json
from functools import partial

import numpy as np
import pytest
import torch

import vit_attention_common as VC
from conftest import load_golden
from vit_discard_common import chain, discard_ref, fuse, row_rel

pytestmark = pytest.mark.gpu

GUARD = 1023                                                # odd: the first matrix is only 4-byte aligned as well
SENTINEL = -7.0


def _run(dev, F, k):
    """F [n_mats, T, T] on the CPU -> (attention_discard of a guarded device copy, the guards were left alone)."""
    from multimodal import vit_maps
    n = F.numel()
    buf = torch.full((GUARD + n + GUARD,), SENTINEL, dtype=torch.float32, device=dev)
    slab = buf[GUARD:GUARD + n].view(1, *F.shape)
    slab.copy_(F)
    out = vit_maps.attention_discard(slab, k)
    assert out.data_ptr() == slab.data_ptr()                # in place
    intact = bool((buf[:GUARD] == SENTINEL).all()) and bool((buf[GUARD + n:] == SENTINEL).all())
    return out[0].cpu(), intact


def _check_exact(dev, tag, F, ks):
    res = []
    for k in ks:
        want = discard_ref(F, k)
        got, intact = _run(dev, F, k)
        again, _ = _run(dev, F, k)
        wrong = int((got.view(torch.int32) != want.view(torch.int32)).sum())         # bits, so that -0.0 would count
        zeros = int((want == 0).sum()) - int((F == 0).sum())
        print(f"[discard {tag}] {tuple(F.shape)} k {k}: {zeros} new zeros, {wrong} elements differ from the definition, "
              f"second call bit-equal {torch.equal(again, got)}, guards intact {intact}")
        res.append((k, wrong, torch.equal(got, want), torch.equal(again, got), intact))
    for k, wrong, same, twice, intact in res:
        assert wrong == 0 and same, (tag, k, wrong)
        assert twice, (tag, k)
        assert intact, (tag, k)


def _softmax(n_mats, T, seed):
    return torch.randn(n_mats, T, T, generator=torch.Generator().manual_seed(seed)).softmax(-1).contiguous()


# ---- cvcl_attention_discard: the selection, exact ----------------------------------------------------------------------------

@pytest.mark.parametrize("n_mats,T", [(1, 17),              # less than one 1024-element chunk
                                      (6, 33),              # just over one; odd T T: matrices 1 .. 5 start 4-byte aligned only
                                      (2, 197),             # the product shape
                                      (2, 257)])
def test_discard_exact(dev, n_mats, T):
    M = T * T
    _check_exact(dev, "softmax", _softmax(n_mats, T, 7 * T + n_mats), (1, int(0.5 * M), int(0.9 * M), M - 1))


def test_discard_tie_group_across_the_cut(dev):
    """Forty elements of one value, over rows 21 .. 31 and across flat index 1024, k inside the group: the lowest indices go."""
    T = 33
    F = _softmax(2, T, 5)
    flat = F.view(2, -1)
    mid = flat[0].sort().values[T * T // 2:T * T // 2 + 2]
    val = float((mid[0] + mid[1]) / 2)                      # between two neighbours of the order: no element has it yet
    idx = 700 + 9 * torch.arange(40)                        # 700 .. 1051
    assert int(idx[0]) // T == 21 and int(idx[-1]) // T == 31 and int(idx[0]) < 1024 < int(idx[-1])
    flat[:, idx] = val
    assert int((flat[0] == val).sum()) == 40
    below = int((flat[0] < val).sum())
    assert int((flat[1] < val).sum()) != below              # the second matrix is cut elsewhere: each matrix is selected on its own
    ks = (below + 1, below + 17, below + 40, below + 41)
    _check_exact(dev, "40 equal", F, ks)
    got, _ = _run(dev, F, below + 17)
    gone = (got.view(2, -1)[0, idx] == 0)
    assert bool(gone[:17].all()) and not bool(gone[17:].any())


def test_discard_all_equal(dev):
    for T in (17, 33):
        M = T * T
        F = torch.full((2, T, T), 1.0 / T)
        _check_exact(dev, "all equal", F, (1, 2, M // 2, M - 1))
        got, _ = _run(dev, F, M // 2)
        flat = got.view(2, -1)
        assert torch.equal(flat[:, 0], F[:, 0, 0]) and bool((flat[:, 1:M // 2] == 0).all()) and bool((flat[:, M // 2:] != 0).all())


def test_discard_element_zero_is_the_minimum(dev):
    T = 33
    F = _softmax(2, T, 9)
    F[:, 0, 0] = 0.5 * float(F.min())
    _check_exact(dev, "F[0, 0] min", F, (1, 2, 5, int(0.9 * T * T)))
    got, _ = _run(dev, F, 5)
    assert torch.equal(got[:, 0, 0], F[:, 0, 0]) and int((got == 0).sum()) == 2 * 4      # kept, and k - 1 others zeroed


@pytest.mark.parametrize("T", [33, 197])
def test_discard_with_exact_zeros(dev, T):
    """30 % exact zeros, as bf16 underflow produces: cuts inside the zeros, at their end and past it."""
    M = T * T
    F = _softmax(2, T, 3 * T)
    F[torch.rand(F.shape, generator=torch.Generator().manual_seed(T)) < 0.3] = 0.0
    nz = int((F[0] == 0).sum())
    assert 0.25 * M < nz < 0.35 * M
    _check_exact(dev, "30% zeros", F, (1, int(0.1 * M), nz, nz + 1, int(0.5 * M), int(0.9 * M), M - 1))


# ---- the chain after the discard ---------------------------------------------------------------------------------------------

@functools.lru_cache(maxsize=None)
def _fused_inputs(n_layers, T):
    """As tests/test_vit_rollout_gpu.py: row-stochastic F (rowsum(F + I) = 2) and the max / min over 3 such heads, B = 2."""
    B, heads = 2, 3
    g = torch.Generator().manual_seed(100 * n_layers + T)
    P = torch.randn(n_layers, B, heads, T, T, generator=g).softmax(-1)
    return {"mean": P[:, :, 0].contiguous(), "max": P.max(2).values.contiguous(), "min": P.min(2).values.contiguous()}


@pytest.mark.parametrize("T", [17, 197])
@pytest.mark.parametrize("n_layers", [2, 12])
def test_chain_after_discard_vs_float64(dev, n_layers, T):
    """The float64 chain runs on discard_ref of the SAME fp32 slab: the mask is identical by construction, the arithmetic of the
    chain on a matrix that is 90 % zeros is what is compared."""
    from multimodal import vit_maps
    k = int(T * T * 0.9)
    res = []
    for kind, Fs in _fused_inputs(n_layers, T).items():
        D = discard_ref(Fs, k)
        Dd = vit_maps.attention_discard(Fs.to(dev), k)
        assert torch.equal(Dd.cpu(), D), kind
        for s in sorted({0, n_layers // 2}):
            ref64, ref32 = chain(list(D.double()), s), chain(list(D), s)
            tau = 4 * row_rel(ref32, ref64)
            full = vit_maps.rollout_chain(Dd, s, T)
            one = vit_maps.rollout_chain(Dd, s, 1)
            err = row_rel(full.cpu(), ref64)
            rowsum = float((full.double().sum(-1) - 1).abs().max())
            bit = torch.equal(one, full[:, :1])
            print(f"[chain after discard {kind}] layers {n_layers} T {T} k {k} start {s}: tau {tau:.3e}, kernel error {err:.3e}, "
                  f"row sums off 1 by {rowsum:.3e} (bound {n_layers * T * 2.0 ** -23:.3e}), q_rows = 1 bit-equal to row 0 {bit}")
            res.append((kind, s, tau, err, rowsum, bit))
    for kind, s, tau, err, rowsum, bit in res:
        assert err <= tau, (kind, s, err, tau)
        assert rowsum <= n_layers * T * 2.0 ** -23, (kind, s, rowsum)
        assert bit, (kind, s)


# ---- the whole toy ViT -----------------------------------------------------------------------------------------------------

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


def _toy_inputs():
    gt, gi = load_golden("vit_tiny"), load_golden("vit_tiny_interp")
    return (("native", gt["x"]), ("resampled", gi["x_a"]))


def _model_fused(sd, x, fusion):
    """The fused attention of every block of the toy model in the dtype of ``sd``: VC._walk's attention per block."""
    with torch.no_grad():
        return [fuse(attn, fusion) for _, _, attn, _ in VC._walk(sd, x, 8, 2, 1e-6)]


@pytest.mark.parametrize("fusion,ratio,start", [("mean", 0.9, 0), ("max", 0.9, 0), ("min", 0.9, 1), ("mean", 0.5, 1)])
def test_model_rollout_discard_vs_float64(dev, fusion, ratio, start):
    from multimodal import vit_maps
    m, sd = _tiny(dev)
    sd64 = VC.to_dtype(sd, torch.float64)
    res = []
    for tag, x in _toy_inputs():
        T = (x.shape[2] // 8) * (x.shape[3] // 8) + 1
        k = int(T * T * ratio)
        F64, F32 = _model_fused(sd64, x.double(), fusion), _model_fused(sd, x, fusion)
        # the condition on the references alone: no element within reach of the cut
        gap = min(float((o[:, k] - o[:, k - 1]).min()) for o in (f.reshape(f.shape[0], -1).sort(-1).values for f in F64))
        ferr = max(float((a.double() - b).abs().max()) for a, b in zip(F32, F64))
        print(f"[toy ViT {tag} {tuple(x.shape)}] {fusion} ratio {ratio}: k {k} of {T * T}, smallest gap at the cut {gap:.3e}, "
              f"fp32 error of F {ferr:.3e} (x 16 = {16 * ferr:.3e})")
        assert gap >= 16 * ferr, (tag, gap, ferr)
        ref64 = chain([discard_ref(f, k) for f in F64], start)
        ref32 = chain([discard_ref(f, k) for f in F32], start)
        tau = 4 * row_rel(ref32, ref64)
        got, grid = vit_maps.attention_rollout(m, x.to(dev), fusion, start, T, discard_ratio=ratio)
        assert got.shape == (x.shape[0], T, T) and got.dtype == torch.float32 and grid == (x.shape[2] // 8, x.shape[3] // 8)
        err = row_rel(got.cpu(), ref64)
        plain = vit_maps.attention_rollout(m, x.to(dev), fusion, start, T)[0]
        moved = row_rel(plain.cpu(), ref64)
        print(f"[toy ViT {tag} {tuple(x.shape)}] {fusion} ratio {ratio} start {start}: tau {tau:.3e}, error {err:.3e} "
              f"(the rollout without the discard is {moved:.3e} away)")
        res.append((tag, tau, err, moved))
        cls = vit_maps.attention_rollout(m, x.to(dev), fusion, start, 1, discard_ratio=ratio)[0]
        assert cls.shape == (x.shape[0], 1, T) and torch.equal(cls, got[:, :1])
    for tag, tau, err, moved in res:
        assert err <= tau, (tag, fusion, ratio, start, err, tau)
        assert moved > 100 * tau, (tag, moved, tau)         # the discard is not a no-op on these inputs


# ---- invariants --------------------------------------------------------------------------------------------------------------

def test_ratio_zero_chunking_forward_and_map_sums(dev):
    from multimodal import attention_maps as A
    from multimodal import vit_maps
    m, _ = _tiny(dev)
    x = torch.randn(5, 3, 32, 32, generator=torch.Generator().manual_seed(11)).to(dev)
    T = 17
    before = m(x).clone()
    today = m.get_attention_rollout(x, "max", 1, T)         # the call as it is without the variant
    assert torch.equal(vit_maps.attention_rollout(m, x, "max", 1, T)[0], today)                       # the keyword left out
    assert torch.equal(vit_maps.attention_rollout(m, x, "max", 1, T, discard_ratio=0.0)[0], today)
    assert torch.equal(vit_maps.attention_rollout(m, x, "max", 1, T, discard_ratio=0)[0], today)
    assert torch.equal(vit_maps.attention_rollout(m, x, "max", 1, T, discard_ratio=1e-9)[0], today)   # k = int(289e-9) = 0
    assert torch.equal(A.vit_attention_rollout_discard(m, x, 0.0), A.vit_attention_rollout(m, x))
    whole, grid = vit_maps.attention_rollout(m, x, "mean", 0, T, discard_ratio=0.9)
    assert grid == (4, 4) and whole.shape == (5, T, T)
    assert not torch.equal(whole, vit_maps.attention_rollout(m, x, "mean", 0, T)[0])
    per_image = 2 * T * T * 4
    for budget in (2 * per_image, 1):                       # chunks of 2, 2, 1 images; a budget below one image: one by one
        part, _ = vit_maps.attention_rollout(m, x, "mean", 0, T, slab_bytes=budget, discard_ratio=0.9)
        assert torch.equal(part, whole), budget
    maps = A.vit_attention_rollout_discard(m, x, 0.9)
    assert maps.shape == (5, 4, 4) and torch.equal(maps, whole[:, 0, 1:].reshape(5, 4, 4))
    off = float((maps.double().sum((-2, -1)) - (1.0 - whole[:, 0, 0].double())).abs().max())
    print(f"[toy ViT] ratio 0.9: map sums off 1 - R[0, 0] by {off:.3e} (bound {2 * T * 2.0 ** -23:.3e})")
    assert off <= 2 * T * 2.0 ** -23                        # n_layers T 2^-23, the row-sum bound of the chain
    assert bool((maps >= 0).all())
    big = A.vit_attention_rollout_discard(m, x, 0.9, size=(32, 32))
    assert big.shape == (5, 32, 32) and torch.equal(big, A.bicubic_resize(maps, (32, 32)))
    enc = torch.nn.Module()                                 # a VisionEncoder wrapper is accepted as well
    enc.model = m
    assert torch.equal(A.vit_attention_rollout_discard(enc, x, 0.9), maps)
    after = m(x).clone()
    torch.cuda.synchronize()
    assert torch.equal(before, after)


# ---- eval.py --attention_rollout --rollout_discard_ratio ---------------------------------------------------------------------

def _patched_vit():
    from multimodal import vision_transformer_dino_mugs as vits
    return lambda name, pretrained: vits.VisionTransformer(img_size=[224], patch_size=16, embed_dim=768, depth=2, num_heads=12, mlp_ratio=4,
                                                           qkv_bias=True, num_classes=0, norm_layer=partial(torch.nn.LayerNorm, eps=1e-6))


def test_eval_rollout_discard_ratio(dev, tmp_path, monkeypatch):
    """eval.py --attention_maps DIR --attention_rollout --rollout_discard_ratio 0.9 on a synthetic ViT checkpoint: cams.npy has the
    shape it has without the ratio and other values (finite, non-negative), and the prediction records do not change."""
    import eval as ev
    import train
    import multimodal.multimodal as mm
    monkeypatch.chdir(tmp_path)
    monkeypatch.setattr(mm, "load_model", _patched_vit())
    exp = "multimodal_text_encoder_embedding_pretrained_cnn_False_finetune_cnn_False_seed_0"
    argv = ("--dataset synthetic --batch_size 4 --val_batch_size 4 --gpus 1 --text_encoder embedding --embedding_dim 32 --vit_dino "
            "--lambda_lm 0 --optimize_unused --max_epochs 1 --limit_train_batches 2 --normalize_features "
            f"--checkpoint_callback True --logger False --exp_name {exp}").split()
    base = ["--checkpoint", exp, "--eval_dataset", "synthetic", "--eval_type", "image", "--n_trials", "6", "--trial_batch", "4"]
    d, d9 = tmp_path / "rollout", tmp_path / "rollout09"
    with contextlib.redirect_stdout(io.StringIO()):
        train.main(argv)
        rolled = ev.main(ev._parser().parse_args(base + ["--attention_maps", str(d), "--attention_rollout"]))
        thinned = ev.main(ev._parser().parse_args(base + ["--attention_maps", str(d9), "--attention_rollout",
                                                          "--rollout_discard_ratio", "0.9"]))
    assert json.dumps(rolled) == json.dumps(thinned)
    cams, cams9 = np.load(d / "cams.npy"), np.load(d9 / "cams.npy")
    assert cams.shape == (6, 4, 14, 14) and cams9.shape == cams.shape and cams9.dtype == np.float32
    assert np.isfinite(cams9).all() and (cams9 >= 0).all()
    assert not np.allclose(cams9, cams, rtol=1e-2, atol=0)
    spread, spread9 = float((cams.max((-2, -1)) / cams.mean((-2, -1))).mean()), float((cams9.max((-2, -1)) / cams9.mean((-2, -1))).mean())
    print(f"[eval.py] peak / mean of a map: {spread:.3f} without the discard, {spread9:.3f} at ratio 0.9")
    with pytest.raises(SystemExit, match="--attention_rollout"):
        ev.main(ev._parser().parse_args(base + ["--attention_maps", str(d9), "--rollout_discard_ratio", "0.9"]))
