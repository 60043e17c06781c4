"""CPU side of the CLIP evaluation (reference eval.py:29-45, 205-207, 224-226): the float64 restatement the GPU tests compare
against is itself pinned to an independent implementation (``transformers.CLIPModel``), the tokenizer to ``transformers.CLIPTokenizer``
on a synthetic merges file; state-dict shape inference, the C ABI additions, the eval.py parser and the refusals need no GPU."""
import os
import re

import pytest
import torch

import clip_common as CC
from conftest import ROOT


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


@pytest.fixture(scope="module")
def merges_file(tmp_path_factory):
    merges = CC.learn_merges(CC.vocab_words(), 300)
    assert len(merges) == 300
    return CC.write_merges(tmp_path_factory.mktemp("bpe") / "bpe_synthetic.txt", merges), merges


# ---- (a) the restatement against transformers ---------------------------------------------------------------------------------------
def test_restatement_matches_transformers_clip():
    transformers = pytest.importorskip("transformers")
    vocab = 99
    tower = dict(hidden_size=128, intermediate_size=512, num_hidden_layers=2, num_attention_heads=2, hidden_act="quick_gelu",
                 layer_norm_eps=1e-5)
    cfg = transformers.CLIPConfig(
        text_config=dict(tower, vocab_size=vocab, max_position_embeddings=77, eos_token_id=vocab - 1, bos_token_id=vocab - 2, pad_token_id=0),
        vision_config=dict(tower, image_size=42, patch_size=14), projection_dim=32, logit_scale_init_value=1.5)
    cfg._attn_implementation = "sdpa"                    # (the eager form takes its soft-max in float32)
    torch.manual_seed(0)
    hf = transformers.CLIPModel(cfg).double().eval()
    with torch.no_grad():
        for n, p in hf.named_parameters():                  # away from the initialisation's zeros / ones: biases and LayerNorms count
            if n.endswith("bias") or "norm" in n:
                p.add_(torch.randn_like(p) * 0.1)
    sd = CC.from_transformers(hf.state_dict())
    g = torch.Generator().manual_seed(1)
    image = torch.randn(3, 3, 42, 42, generator=g, dtype=torch.float64)
    tok = torch.zeros(4, 77, dtype=torch.long)
    for b, n in enumerate((1, 5, 30, 75)):                  # SOS, n words, EOS (= the largest id, once per row), zero padding
        tok[b, 0], tok[b, n + 1] = vocab - 2, vocab - 1
        tok[b, 1:n + 1] = torch.randint(1, vocab - 2, (n,), generator=g)
    with torch.no_grad():
        out = hf(input_ids=tok, pixel_values=image)
    rel = lambda a, b: float((a - b).abs().max() / b.abs().max())
    img_hf = hf.visual_projection(hf.vision_model(pixel_values=image).pooler_output)
    txt_hf = hf.text_projection(hf.text_model(input_ids=tok).pooler_output)
    e_img, e_txt = rel(CC.encode_image(sd, image), img_hf.detach()), rel(CC.encode_text(sd, tok), txt_hf.detach())
    lpi, lpt = CC.logits(sd, image, tok)
    e_lpi, e_lpt = rel(lpi, out.logits_per_image), rel(lpt, out.logits_per_text)
    print(f"restatement vs transformers.CLIPModel (float64): image {e_img:.1e}, text {e_txt:.1e}, logits {e_lpi:.1e}")
    assert max(e_img, e_txt, e_lpi, e_lpt) < 1e-12


# ---- (b) the tokenizer ------------------------------------------------------------------------------------------------------------
STRINGS = ["A Ball", "the   kitty\tcat ", "it's the dog's toy, isn't it?", "2 apples and 37 bananas!", "Hello... World!!", "we'll  see; they've gone",
           "room 101", "a-b-c d_e", "I'm here (now)", "what's 'that'?", "CRIB & chair #4", "sand,sand.sand"]


def test_tokenizer_matches_transformers(merges_file):
    transformers = pytest.importorskip("transformers")
    from multimodal import clip_model as CM
    path, merges = merges_file
    tk = CM.SimpleTokenizer(path)
    assert len(tk.encoder) == 512 + len(merges) + 2
    sot, eot = tk.encoder[CM.SOT], tk.encoder[CM.EOT]
    assert (sot, eot) == (512 + len(merges), 512 + len(merges) + 1)
    hf = transformers.CLIPTokenizer(vocab=dict(tk.encoder), merges=[tuple(m) for m in merges])
    words = CC.vocab_words()
    assert len(words) == 2350
    texts = words + STRINGS
    got = CM.tokenize(texts, path)
    assert got.shape == (len(texts), 77) and got.dtype == torch.int64
    for text, row in zip(texts, got):
        want = hf(text)["input_ids"]
        n = len(want)
        assert want[0] == sot and want[-1] == eot, text
        assert row[:n].tolist() == want, (text, row[:n].tolist(), want)
        assert int(row[n:].abs().sum()) == 0 and int(row.argmax()) == n - 1, text       # zero padding; EOT is the first maximum
    assert CM.tokenize("ball", path).shape == (1, 77)
    assert CM.tokenize(["a b c"], path, context_length=5).tolist() == [[sot] + tk.encode("a b c") + [eot]]
    with pytest.raises(RuntimeError, match="too long"):
        CM.tokenize(["a b c d"], path, context_length=5)
    with pytest.raises(RuntimeError, match="too long"):
        CM.tokenize("ball " * 76, path)


def test_tokenizer_reads_gzip(merges_file, tmp_path):
    import gzip
    from multimodal import clip_model as CM
    path, _ = merges_file
    gz = tmp_path / "bpe_synthetic.txt.gz"
    with open(path, "rb") as f, gzip.open(gz, "wb") as o:
        o.write(f.read())
    assert torch.equal(CM.tokenize(STRINGS, str(gz)), CM.tokenize(STRINGS, path))


# ---- (c) build_model --------------------------------------------------------------------------------------------------------------
def test_build_model_shapes_fp16_and_extra_keys():
    from multimodal import clip_model as CM
    sd = CC.random_state_dict(seed=3, W=128, layers=3, patch=14, R=84, Wt=64, tlayers=2, vocab=300, ctx=77, E=48)
    half = {k: v.half() for k, v in sd.items()}
    half.update(input_resolution=torch.tensor(84), context_length=torch.tensor(77), vocab_size=torch.tensor(300))
    m = CM.build_model(half)
    v = m.visual
    assert (v.embed_dim, v.patch_size, v.input_resolution, v.output_dim, len(v.transformer.resblocks)) == (128, 14, 84, 48, 3)
    assert (m.context_length, m.vocab_size, m.transformer.width, len(m.transformer.resblocks), m.transformer.heads) == (77, 300, 64, 2, 1)
    assert not m.training
    got = m.state_dict()
    assert sorted(got) == sorted(sd)                          # OpenAI's names, nothing else, the three extra keys ignored
    for k, t in got.items():
        assert t.dtype == torch.float32 and torch.equal(t, half[k].float()), k
    with pytest.raises(RuntimeError):                         # strict: a missing tensor is an error
        CM.build_model({k: t for k, t in sd.items() if k != "ln_final.bias"})


def test_load_plain_state_dict_file(tmp_path):
    from multimodal import clip_model as CM
    sd = CC.random_state_dict(seed=4)
    p = tmp_path / "clip_sd.pt"
    torch.save(sd, p)
    m, norm = CM.load(str(p), device="cpu")
    assert torch.equal(m.visual.proj, sd["visual.proj"])
    x = torch.rand(2, 3, 4, 4)
    want = (x - torch.tensor(CM.CLIP_MEAN).view(3, 1, 1)) / torch.tensor(CM.CLIP_STD).view(3, 1, 1)
    assert torch.equal(norm(x), want)


# ---- (d) the C ABI additions --------------------------------------------------------------------------------------------------------
def test_abi_additions(H):
    txt = open(os.path.join(ROOT, "include", "cvcl_hip.h")).read()
    assert re.search(r"#define CVCL_ABI_VERSION 7\b", txt) and H.ABI_VERSION == 7 and H.lib().cvcl_abi_version() == 7
    assert re.search(r"CVCL_ACT_QUICK_GELU = 3\b", txt) and H.ACT_QUICK_GELU == 3
    code = re.sub(r"/\*.*?\*/", "", txt, flags=re.S)
    for name, nargs in (("cvcl_attention_causal", 9), ("cvcl_clip_text_pool", 10)):
        m = re.search(name + r"\s*\(([^)]*)\)", code)
        assert m and len(m.group(1).split(",")) == nargs, name
        assert len(H.SIGNATURES[name][1]) == nargs and hasattr(H.lib(), name)
    lib = H.lib()
    # argument checks answer before any launch (no GPU here)
    assert lib.cvcl_attention_causal(H.F32, None, None, 1, 77, 2, 64, 0.125, None) == -1 and b"cvcl_attention_causal" in lib.cvcl_last_error()
    assert lib.cvcl_attention_causal(H.F32, 16, 16, 1, 77, 2, 256, 0.125, None) == -1
    assert lib.cvcl_attention_causal(7, 16, 16, 1, 77, 2, 64, 0.125, None) != 0
    assert lib.cvcl_clip_text_pool(None, None, None, None, 1e-5, None, 1, 77, 128, None) == -1 and b"cvcl_clip_text_pool" in lib.cvcl_last_error()
    assert lib.cvcl_clip_text_pool(16, 16, 16, 16, 1e-5, 16, 0, 77, 128, None) == -1


def test_quick_gelu_refused_routes_without_gpu(H):
    """plan_gemm refuses QuickGELU where no kernel implements it, before anything is enqueued: CVCL_F32X3, LayerNorm-folded, C_pre / G."""
    import ctypes as C
    lib = H.lib()

    def block(**kw):
        a = H.GemmArgs()
        a.A, a.W, a.C = 16, 16, 16
        a.M, a.N, a.K, a.lda, a.ldw, a.ldc = 512, 256, 256, 256, 256, 256
        a.bias, a.act = 16, H.ACT_QUICK_GELU
        for k, v in kw.items():
            setattr(a, k, v)
        return a
    assert lib.cvcl_gemm(H.F32X3, C.byref(block()), None) == -1 and b"QuickGELU" in lib.cvcl_last_error()
    assert lib.cvcl_gemm(H.BF16, C.byref(block(C_pre=16)), None) != 0
    assert lib.cvcl_gemm(H.BF16, C.byref(block(G=16, ldg=256)), None) != 0
    assert lib.cvcl_gemm(H.BF16, C.byref(block(M=65792, N=4096, K=1024, lda=1024, ldw=1024, ldc=4096, ln_stats=16, ln_colsum=16)), None) != 0
    assert not lib.cvcl_gemm_ln_supported(C.byref(block(M=65792, N=4096, K=1024, lda=1024, ldw=1024, ldc=4096, ln_stats=16, ln_colsum=16)))
    a = block(M=65792, N=4096, K=1024, lda=1024, ldw=1024, ldc=4096, ln_stats=16, ln_colsum=16)
    assert lib.cvcl_gemm8w(1, C.byref(a), None) == -1 and b"QuickGELU" in lib.cvcl_last_error()
    a.act = H.ACT_GELU                                        # (the same block with GELU is what the DINO ViT's folded route runs)
    assert lib.cvcl_gemm_ln_supported(C.byref(a))


# ---- (e) eval.py ------------------------------------------------------------------------------------------------------------------
def _eval_main(argv):
    import eval as ev
    return ev.main(ev._parser().parse_args(argv))


def test_eval_parser_and_exit_messages(tmp_path):
    import eval as ev
    a = ev._parser().parse_args(["--clip_eval", "--clip_checkpoint", "w.pt", "--clip_bpe", "bpe.txt", "--eval_dataset", "synthetic"])
    assert a.clip_eval and a.clip_checkpoint == "w.pt" and a.clip_bpe == "bpe.txt" and a.precision == "32"
    assert ev._parser().parse_args([]).clip_checkpoint is None and ev._parser().parse_args([]).clip_bpe is None
    with pytest.raises(SystemExit, match=r"--clip_checkpoint.*--clip_bpe"):
        _eval_main(["--clip_eval", "--eval_dataset", "synthetic"])
    with pytest.raises(SystemExit, match=r"--clip_bpe"):
        _eval_main(["--clip_eval", "--clip_checkpoint", "w.pt", "--eval_dataset", "synthetic"])
    both = ["--clip_eval", "--clip_checkpoint", "w.pt", "--clip_bpe", "bpe.txt", "--eval_dataset", "synthetic"]
    for extra, word in ((["--attention_maps", str(tmp_path)], "attention_maps"), (["--attention_rollout"], "attention_rollout"),
                        (["--hip_graph"], "hip_graph"), (["--precision", "32-split"], "32-split")):
        with pytest.raises(SystemExit, match=word):
            _eval_main(both + extra)
    with pytest.raises(SystemExit, match="synthetic"):
        _eval_main(["--clip_eval", "--clip_checkpoint", "w.pt", "--clip_bpe", "bpe.txt", "--eval_dataset", "saycam"])
    args = ev._parser().parse_args(both + ["--eval_type", "text", "--stage", "dev"])
    assert ev.clip_results_filename(args) == "results/synthetic/clip_text_synthetic_dev_eval_predictions.json"
    assert ev.CLIP_CONFIG == {"model": "clip", "seed": None, "shuffle_utterances": None, "cnn": "clip", "augment_frames": None,
                              "multiple_frames": None}


def test_synthetic_trials_under_clip_eval(merges_file):
    import argparse
    from multimodal import clip_model as CM
    from multimodal.multimodal_data_module import IMAGENET_MEAN, IMAGENET_STD, SyntheticDataModule
    path, _ = merges_file
    for et in ("image", "text"):
        common = dict(eval_type=et, n_eval_trials=2, seed=0)
        plain = SyntheticDataModule(argparse.Namespace(**common))
        clip = SyntheticDataModule(argparse.Namespace(clip_eval=True, clip_bpe=path, **common))
        for d in (plain, clip):
            d.setup()
        a, b = plain.eval_sets["test"][1], clip.eval_sets["test"][1]
        frames = a[0] * torch.tensor(IMAGENET_STD).view(1, 3, 1, 1) + torch.tensor(IMAGENET_MEAN).view(1, 3, 1, 1)     # the same frames in [0, 1]
        assert torch.allclose(b[0], CM.normalize_frames(frames), atol=1e-6)
        meta = clip.eval_sets["test"].metadata()[1]
        names = [meta["target_category"]] + (meta["foil_categories"] if et == "text" else [])
        assert torch.equal(b[1], CM.tokenize(names, path)) and b[1].shape == (len(names), 77)
        assert b[3] == a[3]


# ---- (f) no CPU path, refused precisions and shapes ------------------------------------------------------------------------------------
def test_refusals(H):
    from multimodal import clip_model as CM
    m = CM.build_model(CC.random_state_dict(seed=5))
    with pytest.raises(H.CvclError):
        m.encode_image(torch.randn(1, 3, 84, 84))
    with pytest.raises(H.CvclError):
        m.encode_text(torch.zeros(1, 77, dtype=torch.long))
    with pytest.raises(H.CvclError):
        m(torch.randn(1, 3, 84, 84), torch.zeros(1, 77, dtype=torch.long))
    for p in ("32-split", "fp8", "16"):
        with pytest.raises(H.CvclError, match="precision"):
            m.set_precision(p)
    assert m.set_precision("bf16").visual.compute_dtype == torch.bfloat16 and m.set_precision("32").visual.compute_dtype == torch.float32
    with pytest.raises(H.CvclError, match="multiple of 64"):
        CM.build_model(CC.random_state_dict(seed=5, W=96))
    with pytest.raises(H.CvclError, match="multiple of 64"):
        CM.build_model(CC.random_state_dict(seed=5, Wt=32))
    with pytest.raises(H.CvclError, match="288"):                                     # ViT-L/14@336: 577 tokens
        CM.build_model(CC.random_state_dict(seed=5, W=64, layers=1, R=336, Wt=64, tlayers=1))
    CM.build_model(CC.random_state_dict(seed=5, W=64, layers=1, R=224, Wt=64, tlayers=1))   # 257 tokens: accepted
