"""GPU: the 32-split precision (CVCL_F32X3) -- fp32 storage with split-bf16 products in every ResNeXt trunk convolution.

Kernel level: the split GEMM (csrc/gemm_split.hip) at every distinct 1x1 / downsample shape of the B = 256, 224^2 trunk on exact
integer data (one operand with 9-16 significant bits, which bf16 cannot hold, the other in {-2..2}, sums below 2^24) must equal
float64 exactly, in both orientations, and its fused BatchNorm statistics must match float64 sums of the same output.
Trunk and model level: against the float64 oracle and against the exact-fp32 mode.  Refusals: dtype 2 / 3 on entries outside
the trunk forward, --finetune_cnn and the ViT."""
import contextlib
import ctypes as C
import io

import pytest
import torch

import cvcl_oracle as O
from conftest import maxrel

pytestmark = pytest.mark.gpu

B = 256
# (M, K, N, gather (ho, wo, hi, wi, stride) or None): every distinct 1x1 convolution / downsample of the B = 256, 224^2 trunk
SHAPES = [
    (B * 56 * 56, 64, 128, None), (B * 56 * 56, 64, 256, None), (B * 56 * 56, 256, 128, None), (B * 56 * 56, 128, 256, None),
    (B * 56 * 56, 256, 256, None), (B * 28 * 28, 256, 512, (28, 28, 56, 56, 2)), (B * 28 * 28, 256, 512, None),
    (B * 28 * 28, 512, 256, None), (B * 28 * 28, 512, 512, None), (B * 14 * 14, 512, 1024, (14, 14, 28, 28, 2)),
    (B * 14 * 14, 512, 1024, None), (B * 14 * 14, 1024, 512, None), (B * 14 * 14, 1024, 1024, None),
    (B * 7 * 7, 1024, 2048, (7, 7, 14, 14, 2)), (B * 7 * 7, 1024, 2048, None), (B * 7 * 7, 2048, 1024, None),
]


@pytest.fixture(scope="module")
def H():
    from multimodal import _hip
    return _hip


def _wide_ints(shape, K, g, dev):
    """odd integers of 9..16 significant bits (|x| >= 257: hi and lo parts both non-zero), |x| small enough that
    sum_k |a w| < 2^24 with |w| <= 2"""
    amax = min((1 << 16) - 1, ((1 << 24) - 1) // (2 * K))
    mag = torch.randint(128, (amax + 1) // 2, shape, generator=g, device=dev) * 2 + 1
    sign = torch.randint(0, 2, shape, generator=g, device=dev) * 2 - 1
    return (mag * sign).float()


def _small_ints(shape, g, dev):
    return torch.randint(-2, 3, shape, generator=g, device=dev).float()


def _pack_dense(H, w, dev):
    N, K = w.shape
    nb = H.lib().cvcl_packed_weight_bytes(H.F32X3, H.PACK_DENSE, N, K, 1)
    assert nb > 0
    buf = torch.empty(nb, dtype=torch.uint8, device=dev)
    H.check(H.lib().cvcl_pack_conv_weight(H.F32X3, H.PACK_DENSE, H.ptr(w.contiguous()), H.ptr(buf), N, K, 1, H.stream_ptr()), "pack")
    return buf


@pytest.mark.parametrize("wide", ["A", "W"])
@pytest.mark.parametrize("M,K,N,gather", SHAPES)
def test_split_gemm_exact_integers_fullsize(H, dev, M, K, N, gather, wide):
    g = torch.Generator(device=dev).manual_seed(M + 7 * K + 13 * N)
    a_rows = M if gather is None else (M // (gather[0] * gather[1])) * gather[2] * gather[3]
    A = _wide_ints((a_rows, K), K, g, dev) if wide == "A" else _small_ints((a_rows, K), g, dev)
    Wt = _small_ints((N, K), g, dev) if wide == "A" else _wide_ints((N, K), K, g, dev)
    Wp = _pack_dense(H, Wt, dev)
    out = torch.full((M, N), float("nan"), device=dev)
    a = H.GemmArgs()
    a.A, a.W, a.C = H.ptr(A), H.ptr(Wp), H.ptr(out)
    a.M, a.N, a.K, a.lda, a.ldw, a.ldc = M, N, K, K, K, N
    if gather is not None:
        a.gather_ho, a.gather_wo, a.gather_hi, a.gather_wi, a.gather_stride = gather
    rows = H.lib().cvcl_gemm_stats_rows(H.F32X3, C.byref(a))
    assert 0 < rows <= 1024
    stats = torch.full((rows + 1, 2, N), float("nan"), device=dev)
    a.stats, a.stats_rows = H.ptr(stats), rows
    H.check(H.lib().cvcl_gemm(H.F32X3, C.byref(a), H.stream_ptr()), "cvcl_gemm(F32X3)")
    torch.cuda.synchronize()
    Ad = A.double()
    if gather is not None:
        ho, wo, hi, wi, s = gather
        Ad = Ad.view(-1, hi, wi, K)[:, ::s, ::s, :].reshape(M, K)
    ref = Ad @ Wt.double().t()
    assert ref.abs().max() < 2 ** 24
    bad = (out.double() != ref).sum().item()
    assert bad == 0, f"{bad} of {M * N} outputs differ from float64 (max |diff| {(out.double() - ref).abs().max().item()})"
    assert torch.isnan(stats[rows]).all()                    # nothing past the rows the query announced
    s = stats[:rows].double().sum(dim=0)
    assert maxrel(s[0], ref.sum(dim=0)) < 2e-5
    assert maxrel(s[1], (ref * ref).sum(dim=0)) < 2e-5


def _sparse_small(shape, nnz, g, dev):
    """{-2..2} with at most nnz non-zeros per row"""
    v = _small_ints(shape, g, dev)
    keep = torch.rand(shape, generator=g, device=dev).topk(nnz, dim=1).indices
    out = torch.zeros_like(v)
    return out.scatter_(1, keep, v.gather(1, keep))


def _bits_ints(shape, lo_bits, hi_bits, g, dev):
    """odd integers with lo_bits..hi_bits significant bits, random sign"""
    mag = torch.randint(1 << (lo_bits - 2), 1 << (hi_bits - 1), shape, generator=g, device=dev) * 2 + 1
    return (mag * (torch.randint(0, 2, shape, generator=g, device=dev) * 2 - 1)).float()


def _run_split_gemm(H, dev, A, Wt, M, N, K, gather):
    Wp = _pack_dense(H, Wt, dev)
    out = torch.full((M, N), float("nan"), device=dev)
    a = H.GemmArgs()
    a.A, a.W, a.C = H.ptr(A), H.ptr(Wp), H.ptr(out)
    a.M, a.N, a.K, a.lda, a.ldw, a.ldc = M, N, K, K, K, N
    if gather is not None:
        a.gather_ho, a.gather_wo, a.gather_hi, a.gather_wi, a.gather_stride = gather
    rows = H.lib().cvcl_gemm_stats_rows(H.F32X3, C.byref(a))
    assert 0 < rows <= 1024
    stats = torch.full((rows + 1, 2, N), float("nan"), device=dev)
    a.stats, a.stats_rows = H.ptr(stats), rows
    H.check(H.lib().cvcl_gemm(H.F32X3, C.byref(a), H.stream_ptr()), "cvcl_gemm(F32X3)")
    torch.cuda.synchronize()
    Ad = A.double()
    if gather is not None:
        ho, wo, hi, wi, s = gather
        Ad = Ad.view(-1, hi, wi, K)[:, ::s, ::s, :].reshape(M, K)
    ref = Ad @ Wt.double().t()
    assert ref.abs().max() < 2 ** 24
    bad = (out.double() != ref).sum().item()
    assert bad == 0, f"{bad} of {M * N} outputs differ from float64 (max |diff| {(out.double() - ref).abs().max().item()})"
    assert torch.isnan(stats[rows]).all()
    s = stats[:rows].double().sum(dim=0)
    assert maxrel(s[0], ref.sum(dim=0)) < 2e-5
    assert maxrel(s[1], (ref * ref).sum(dim=0)) < 2e-5


# M not a multiple of the 128-row tile (B = 3): clamped re-reads, masked stores, and the masked rows kept out of the statistics
TAIL_SHAPES = [(3 * 28 * 28, 256, 512, (28, 28, 56, 56, 2)), (3 * 28 * 28, 512, 256, None), (3 * 7 * 7, 1024, 2048, (7, 7, 14, 14, 2)),
               (3 * 7 * 7, 2048, 1024, None)]


@pytest.mark.parametrize("mode", ["A21", "W21", "both11"])
@pytest.mark.parametrize("M,K,N,gather", SHAPES[::3] + TAIL_SHAPES)
def test_split_gemm_needs_every_term(H, dev, M, K, N, gather, mode):
    """Operands whose third bf16 part is non-zero (17-21 significant bits: x2 != 0), or both operands with a non-zero second part
    (a1 w1 != 0): the three terms the 6-term form adds are each needed for the exact result.  Sparse rows (<= 3 non-zeros per dot
    product) keep every partial sum an integer below 2^24.  A 3-term kernel fails all three modes."""
    g = torch.Generator(device=dev).manual_seed(M + 3 * K + 5 * N + len(mode))
    a_rows = M if gather is None else (M // (gather[0] * gather[1])) * gather[2] * gather[3]
    if mode == "A21":
        A, Wt = _bits_ints((a_rows, K), 17, 21, g, dev), _sparse_small((N, K), 3, g, dev)
    elif mode == "W21":
        A, Wt = _sparse_small((a_rows, K), 3, g, dev), _bits_ints((N, K), 17, 21, g, dev)
    else:
        A = _sparse_small((a_rows, K), 3, g, dev).abs().clamp_(max=1) * _bits_ints((a_rows, K), 9, 11, g, dev)
        Wt = _bits_ints((N, K), 9, 11, g, dev)
    _run_split_gemm(H, dev, A, Wt, M, N, K, gather)


@pytest.mark.parametrize("wide", ["A", "W"])
@pytest.mark.parametrize("M,K,N,gather", TAIL_SHAPES)
def test_split_gemm_exact_integers_ragged_m(H, dev, M, K, N, gather, wide):
    g = torch.Generator(device=dev).manual_seed(M + 11 * K + N)
    a_rows = M if gather is None else (M // (gather[0] * gather[1])) * gather[2] * gather[3]
    A = _wide_ints((a_rows, K), K, g, dev) if wide == "A" else _small_ints((a_rows, K), g, dev)
    Wt = _small_ints((N, K), g, dev) if wide == "A" else _wide_ints((N, K), K, g, dev)
    _run_split_gemm(H, dev, A, Wt, M, N, K, gather)


def _ints_below(shape, amax, g, dev):
    """odd integers |x| in [257, amax] (>= 9 significant bits: the second bf16 part is non-zero)"""
    mag = torch.randint(128, (amax + 1) // 2, shape, generator=g, device=dev) * 2 + 1
    return (mag * (torch.randint(0, 2, shape, generator=g, device=dev) * 2 - 1)).float()


def _check_stats(stats, rows, ref_rows):
    assert torch.isnan(stats[rows]).all()
    s = stats[:rows].double().sum(dim=0)
    assert maxrel(s[0], ref_rows.sum(dim=0)) < 2e-5
    assert maxrel(s[1], (ref_rows * ref_rows).sum(dim=0)) < 2e-5


@pytest.mark.parametrize("wide", ["x", "w"])
def test_split_stem_exact_integers_fullsize(H, dev, wide):
    """cvcl_stem_conv7x7(CVCL_F32X3) at B = 256, 224^2 on integer data, against float64 (and its fused statistics)."""
    Bs, S = B, 224
    g = torch.Generator(device=dev).manual_seed(77 + len(wide))
    amax = ((1 << 24) - 1) // (2 * 147)
    x = _ints_below((Bs, 3, S, S), amax, g, dev) if wide == "x" else _small_ints((Bs, 3, S, S), g, dev)
    w = _small_ints((64, 3, 7, 7), g, dev) if wide == "x" else _ints_below((64, 3, 7, 7), amax, g, dev)
    lib = H.lib()
    nb = lib.cvcl_packed_weight_bytes(H.F32X3, H.PACK_STEM7, 64, 3, 7)
    wp = torch.empty(nb, dtype=torch.uint8, device=dev)
    H.check(lib.cvcl_pack_conv_weight(H.F32X3, H.PACK_STEM7, H.ptr(w), H.ptr(wp), 64, 3, 7, H.stream_ptr()), "pack stem")
    rows = lib.cvcl_stem_conv_stats_rows(H.F32X3, Bs, S, S)
    assert 0 < rows <= 1024
    stats = torch.full((rows + 1, 2, 64), float("nan"), device=dev)
    y = torch.full((Bs, S // 2, S // 2, 64), float("nan"), device=dev)
    H.check(lib.cvcl_stem_conv7x7(H.F32X3, H.ptr(x), H.ptr(wp), H.ptr(y), H.ptr(stats), rows, None, Bs, S, S, H.stream_ptr()), "stem")
    torch.cuda.synchronize()
    cols = torch.nn.functional.unfold(x.double(), 7, padding=3, stride=2)          # [B, 147, L]
    ref = torch.einsum("bkl,ok->blo", cols, w.double().reshape(64, 147)).reshape(-1, 64)
    del cols
    assert ref.abs().max() < 2 ** 24
    got = y.double().reshape(-1, 64)
    assert (got != ref).sum().item() == 0, (got - ref).abs().max().item()
    _check_stats(stats, rows, ref)


# (C, H, stride): every stage's grouped 3x3 at the B = 256, 224^2 shapes (layer 1 has no stride-2 block)
GCONV_SHAPES = [(128, 56, 1), (256, 56, 2), (256, 28, 1), (512, 28, 2), (512, 14, 1), (1024, 14, 2), (1024, 7, 1)]


@pytest.mark.parametrize("wide", ["x", "w"])
@pytest.mark.parametrize("Cc,S,stride", GCONV_SHAPES)
def test_split_gconv_exact_integers_fullsize(H, dev, Cc, S, stride, wide):
    """cvcl_gconv3x3(CVCL_F32X3) with its BN + ReLU prologue (scale 1, shift in {-2, 0, 2}: the activation stays integer, and the
    zero padding must stay zero where relu(shift) would not be) against float64, and its fused statistics."""
    Bs, G = B, 32
    cg = Cc // G
    g = torch.Generator(device=dev).manual_seed(Cc * S + stride + len(wide))
    K = 9 * cg
    if wide == "x":
        amax = ((1 << 24) - 1) // (2 * K) - 2
        x = _ints_below((Bs, S, S, Cc), amax, g, dev)
        w = _small_ints((Cc, cg, 3, 3), g, dev)
    else:
        x = _small_ints((Bs, S, S, Cc), g, dev)
        w = _ints_below((Cc, cg, 3, 3), ((1 << 24) - 1) // (4 * K), g, dev)
    scale = torch.ones(Cc, device=dev)
    shift = (torch.randint(-1, 2, (Cc,), generator=g, device=dev) * 2).float()
    lib = H.lib()
    nb = lib.cvcl_packed_weight_bytes(H.F32X3, H.PACK_GCONV3, Cc, cg, 3)
    wp = torch.empty(nb, dtype=torch.uint8, device=dev)
    H.check(lib.cvcl_pack_conv_weight(H.F32X3, H.PACK_GCONV3, H.ptr(w), H.ptr(wp), Cc, cg, 3, H.stream_ptr()), "pack gconv")
    rows = lib.cvcl_gconv3x3_stats_rows(H.F32X3, Bs, S, S, Cc, stride)
    assert 0 < rows <= 1024
    Ho = (S - 1) // stride + 1
    stats = torch.full((rows + 1, 2, Cc), float("nan"), device=dev)
    y = torch.full((Bs, Ho, Ho, Cc), float("nan"), device=dev)
    H.check(lib.cvcl_gconv3x3(H.F32X3, H.ptr(x), H.ptr(scale), H.ptr(shift), H.ptr(wp), H.ptr(y), H.ptr(stats), rows, None,
                              Bs, S, S, Cc, G, stride, H.stream_ptr()), "gconv")
    torch.cuda.synchronize()
    act = torch.relu(x.double() + shift.double()).permute(0, 3, 1, 2)
    ref = torch.empty(Bs, Ho * Ho, Cc, dtype=torch.float64, device=dev)
    for b0 in range(0, Bs, 64):                                                      # (float64 im2col in slices of 64 images)
        cols = torch.nn.functional.unfold(act[b0:b0 + 64], 3, padding=1, stride=stride)          # [b, C * 9, L]
        cols = cols.view(cols.shape[0], G, cg * 9, -1)
        ref[b0:b0 + 64] = torch.einsum("bgkl,gok->blgo", cols, w.double().view(G, cg, cg * 9)).reshape(cols.shape[0], -1, Cc)
        del cols
    ref = ref.reshape(-1, Cc)
    assert ref.abs().max() < 2 ** 24
    got = y.double().reshape(-1, Cc)
    assert (got != ref).sum().item() == 0, (got - ref).abs().max().item()
    _check_stats(stats, rows, ref)


def _load_oracle_params_into(model, p):
    sd = model.state_dict()
    for k, v in p.items():
        sd[k].copy_(v)


@pytest.mark.parametrize("Bt,S,training", [(2, 224, True), (2, 224, False), (3, 64, True), (3, 64, False), (256, 224, True),
                                            (256, 224, False)])
def test_split_trunk_vs_float64_oracle(H, dev, Bt, S, training):
    """cvcl_resnext50_fwd(CVCL_F32X3) through ResNet against the float64 oracle.  Bound: the CPU emulation of the split products
    (every 1x1 product formed from the six part products, DESIGN.md "32-split") moved the pooled output by < 1e-4 at B = 256 on
    noise frames; the GPU's fp32 summation order adds ~1e-4 (the exact mode's own bound is 2e-4): 5e-4 leaves margin."""
    from multimodal.resnext import ResNet
    p = O.resnext50_random_params(seed=1)
    g = torch.Generator().manual_seed(Bt * S)
    for k in list(p.keys()):
        if k.endswith("running_mean"):
            p[k] = torch.randn(p[k].shape, generator=g) * 0.1
        elif k.endswith("running_var"):
            p[k] = torch.rand(p[k].shape, generator=g) * 0.5 + 0.75
        elif ("bn" in k or "downsample.1" in k) and k.endswith(".weight"):
            p[k] = torch.rand(p[k].shape, generator=g) * 0.5 + 0.75
        elif ("bn" in k or "downsample.1" in k) and k.endswith(".bias"):
            p[k] = torch.randn(p[k].shape, generator=g) * 0.1
    x = torch.randn(Bt, 3, S, S, generator=g)
    stats_o = {}
    pd = {k: (v.double() if v.is_floating_point() else v) for k, v in p.items()}
    with torch.no_grad():
        pooled_o, fmap_o = O.resnext50_forward(pd, x.double(), training, stats_out=stats_o)
    model = ResNet()
    _load_oracle_params_into(model, p)
    model = model.to(dev)
    model.compute_dtype = torch.float32
    model.trunk_arithmetic = "split"
    assert model.trunk_dtype() == H.F32X3
    model.train(training)
    for prm in model.parameters():
        prm.requires_grad_(False)
    pooled, fmap = model.trunk(x.to(dev))
    e_p, e_f = maxrel(pooled.double(), pooled_o), maxrel(fmap.double(), fmap_o)
    print(f"32-split trunk train={training} B={Bt} S={S}: pooled rel {e_p:.2e}, layer4 rel {e_f:.2e}")
    assert e_p < 5e-4 and e_f < 5e-4
    sd = model.state_dict()
    if training:
        for k in ("bn1.running_mean", "layer1.0.bn2.running_var", "layer2.0.downsample.1.running_mean",
                  "layer4.2.bn3.running_var", "layer3.5.bn1.running_mean"):
            assert maxrel(sd[k].double(), stats_o[k]) < 2e-4, k
        assert int(sd["layer4.2.bn3.num_batches_tracked"]) == 1


@pytest.fixture(scope="module")
def c2(dev):
    import bench
    lit, ve, _opt = bench.build_model("c2", dev, "32")
    batch = bench.synthetic_batch_on_device(B, seed=0, device=dev)
    return lit, ve, batch


def _logits(lit, batch, precision):
    keep = {k: v.clone() for k, v in lit.state_dict().items() if "running_" in k or "num_batches_tracked" in k}
    gn, lit.model.global_negatives = lit.model.global_negatives, False
    try:
        lit.set_precision(precision)
        lit.train()
        lit.model.text_embed.eval()
        with torch.no_grad():
            li, _ = lit.model(batch[0], batch[1], batch[2])
        torch.cuda.synchronize()
        return li.float().clone()
    finally:
        lit.model.global_negatives = gn
        lit.load_state_dict(keep, strict=False)


def test_c2_split_logits_vs_fp32_noise_point(H, dev, c2):
    import bench
    lit, ve, batch = c2
    par = bench.logits_vs_fp32(lit, batch, "32-split")
    print("noise point:", par)
    assert par["logits_rel_vs_fp32"] < 1e-3
    a, b, c = _logits(lit, batch, "32-split"), _logits(lit, batch, "32"), _logits(lit, batch, "32-split")
    assert not torch.equal(a, b), "32-split gave the exact mode's logits bit for bit: the split kernels did not run"
    assert torch.equal(a, c), "two 32-split runs differ"
    lit.set_precision("32")


def test_c2_split_logits_vs_fp32_conditioned_point(H, dev, c2):
    import bench
    lit, ve, _batch = c2
    evalb = bench.structured_batch_on_device(B, seed=4242, device=dev)
    bn3 = [m.bn3 for m in ve.model.modules() if hasattr(m, "bn3")]
    g_keep = [b.weight.detach().clone() for b in bn3]
    try:
        with torch.no_grad():
            for b in bn3:
                b.weight.fill_(0.25)
        par = bench.logits_vs_fp32(lit, evalb, "32-split")
    finally:
        with torch.no_grad():
            for b, g in zip(bn3, g_keep):
                b.weight.copy_(g)
        lit.set_precision("32")
    print("conditioned point:", par)
    assert par["logits_rel_vs_fp32"] < 1e-3


def test_c2_split_two_stream_trunk_is_bit_identical(H, dev, c2):
    lit, ve, batch = c2
    one = _logits(lit, batch, "32-split")
    ve.model.enable_trunk_stream(dev, inputs="ready", n_streams=2)
    try:
        outs = [_logits(lit, batch, "32-split") for _ in range(3)]    # both streams of the ring, then the first again
    finally:
        ve.model.enable_trunk_stream(dev, inputs=None)
        lit.set_precision("32")
    for o in outs:
        assert torch.equal(o, one)


def test_eval_graph_replay_follows_the_arithmetic(H, dev):
    from multimodal.multimodal import TextEncoder, VisionEncoder
    from multimodal.multimodal_data_module import read_vocab
    from multimodal.multimodal_lit import MultiModalLitModel
    import bench
    torch.manual_seed(0)
    args = bench.c2_args()
    with contextlib.redirect_stdout(io.StringIO()):
        ve = VisionEncoder(args)
        lit = MultiModalLitModel(ve, TextEncoder(read_vocab(), ve.last_cnn_out_dim, args), args)
    lit.to(dev).eval()
    x = bench.synthetic_batch_on_device(8, seed=3, device=dev)[0]
    eager = {}
    with torch.no_grad():
        for p in ("32", "32-split"):
            lit.set_precision(p)
            ve.enable_hip_graphs(False)
            eager[p] = ve(x)[0].clone()                      # (features, layer-4 map)
        assert not torch.equal(eager["32"], eager["32-split"])
        ve.enable_hip_graphs(True)
        for p in ("32", "32-split", "32"):
            lit.set_precision(p)
            got = ve(x)[0]
            torch.cuda.synchronize()
            assert torch.equal(got, eager[p]), p
        ve.enable_hip_graphs(False)


def test_finetune_and_vit_refuse_32_split(H, dev):
    import bench
    from multimodal.multimodal import TextEncoder, VisionEncoder
    from multimodal.multimodal_data_module import read_vocab
    from multimodal.multimodal_lit import MultiModalLitModel
    args = bench.c2_args()
    args.finetune_cnn = True
    with contextlib.redirect_stdout(io.StringIO()):
        ve = VisionEncoder(args)
        lit = MultiModalLitModel(ve, TextEncoder(read_vocab(), ve.last_cnn_out_dim, args), args)
    lit.to(dev)
    with pytest.raises(H.CvclError, match="32-split"):
        lit.set_precision("32-split")
    assert ve.model.trunk_dtype() == H.F32                   # refused before anything changed
    # a trunk switched to split arithmetic behind set_precision's back: the differentiable twin refuses before any launch
    ve.model.trunk_arithmetic = "split"
    with pytest.raises(H.CvclError, match="32-split"):
        ve.model.trunk(torch.zeros(2, 3, 64, 64, device=dev))
    ve.model.trunk_arithmetic = "exact"

    lit4, ve4, _ = bench.build_model("c4", dev, "32")
    with pytest.raises(H.CvclError, match="32-split"):
        lit4.set_precision("32-split")


def test_non_trunk_entries_refuse_dtype_2_and_3(H, dev):
    lib = H.lib()
    s = H.stream_ptr()
    out = torch.full((4096,), 7.0, device=dev)
    src = torch.ones(4096, device=dev)
    ws = torch.zeros(1 << 20, dtype=torch.uint8, device=dev)
    part = torch.full((4096,), 7.0, device=dev)
    for dt in (2, 3):
        assert lib.cvcl_gemm_tn(dt, H.ptr(src), 16, H.ptr(src), 16, 64, 16, 16, H.ptr(out), 16, H.ptr(ws), ws.numel(), s) == -1
        assert b"dtype" in lib.cvcl_last_error()
        assert lib.cvcl_bn_bwd(dt, 0, H.ptr(src), H.ptr(src), H.ptr(src), H.ptr(src), H.ptr(src), H.ptr(src), H.ptr(src), H.ptr(src),
                               H.ptr(out), H.ptr(out), H.ptr(out), None, 64, 16, H.ptr(part), 8, H.ptr(part), s) == -1
        assert b"dtype" in lib.cvcl_last_error()
        assert lib.cvcl_gradcam_pairs(dt, H.ptr(src), 2, 16, 64, H.ptr(src), 2, 0, 0, H.ptr(src), H.ptr(src), H.ptr(src), 1e-8,
                                      H.ptr(out), s) == -1
        assert b"dtype" in lib.cvcl_last_error()
        assert lib.cvcl_layernorm(dt, H.ptr(src), 64, H.ptr(src), H.ptr(src), 1e-5, H.ptr(out), 1, 16, 64, s) == -1
        assert b"dtype" in lib.cvcl_last_error()
        assert lib.cvcl_attention(dt, H.ptr(src), None, H.ptr(out), 1, 8, 2, 64, 0.125, s) == -1
        assert b"dtype" in lib.cvcl_last_error()
        assert lib.cvcl_gemm_tn_workspace_bytes(dt, 64, 16, 16) == 0
        assert lib.cvcl_bn_bwd_partial_rows(dt, 64, 16) == 0
    for dt in (3, -1):
        a = H.GemmArgs()
        a.A, a.W, a.C, a.M, a.N, a.K, a.lda, a.ldw, a.ldc = H.ptr(src), H.ptr(src), H.ptr(out), 16, 128, 32, 32, 32, 128
        assert lib.cvcl_gemm(dt, C.byref(a), s) == -1
        assert b"dtype" in lib.cvcl_last_error()
        assert lib.cvcl_resnext50_workspace_bytes(dt, 2, 64, 64) == 0
        assert lib.cvcl_col_stats(dt, H.ptr(src), 64, 16, H.ptr(out), 64, s) == -1
        assert b"dtype" in lib.cvcl_last_error()
    torch.cuda.synchronize()
    assert (out == 7.0).all() and (part == 7.0).all()
