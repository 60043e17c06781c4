"""GPU, two ranks on one device over gloo (RCCL refuses two ranks per GPU; the collectives' call pattern is the same):
the data-parallel path end to end, through the product's own entry points.

* one C2 step at 256 pairs per rank through DataParallelEngine + OverlappedUpdate with global negatives (N = 512) against
  the oracle's single-process loss / gradients on the concatenated features (SURVEY.md 8e parity definition: reference
  calculate_contrastive_loss math, multimodal.py:796-822, applied to cat_r(features_r); gradients = SUM over ranks);
* ``train.py --gpus 2`` (Trainer.fit: per-rank data shards, per-rank RNG, --local_negatives / lambda_lm handling) against the
  single-process run on the 2B batch."""
import math
import os
import socket
import subprocess
import sys

import pytest
import torch

import cvcl_oracle as O
from conftest import ROOT, maxrel

pytestmark = pytest.mark.gpu
WORKER = os.path.join(ROOT, "tests", "dist_worker.py")


def _free_port():
    s = socket.socket()
    s.bind(("127.0.0.1", 0))
    p = s.getsockname()[1]
    s.close()
    return p


def _run_ranks(args, world=2, timeout=600):
    env = dict(os.environ)
    env.update(CVCL_DIST_BACKEND="gloo", MASTER_ADDR="127.0.0.1", HSA_ENABLE_IPC_MODE_LEGACY="0")
    for k in ("RANK", "WORLD_SIZE", "LOCAL_RANK"):
        env.pop(k, None)
    cmd = [sys.executable, "-m", "torch.distributed.run", "--nnodes=1", f"--nproc-per-node={world}", "--master-addr", "127.0.0.1",
           "--master-port", str(_free_port()), WORKER] + args
    r = subprocess.run(cmd, env=env, capture_output=True, text=True, timeout=timeout)
    assert r.returncode == 0, r.stdout[-3000:] + r.stderr[-3000:]


def _global_negatives_vs_oracle(tmp_path, world):
    _run_ranks(["bench_step", str(tmp_path)], world=world, timeout=1500)
    r = [torch.load(tmp_path / f"rank{i}.pt", weights_only=False) for i in range(world)]
    pooled = torch.cat([x["pooled"] for x in r]).float()
    tok, ln = torch.cat([x["tok"] for x in r]), torch.cat([x["len"] for x in r])
    assert pooled.shape == (256 * world, 2048) and not torch.equal(r[0]["pooled"], r[1]["pooled"])   # ranks saw different shards
    names = {"fc.weight": "vision_encoder.model.fc.weight", "fc.bias": "vision_encoder.model.fc.bias",
             "emb": "text_encoder.embedding.weight"}
    for k in names.values():
        for i in range(1, world):
            assert torch.equal(r[0]["before"][k], r[i]["before"][k]), (k, i)                          # replicas start identical
    w = r[0]["before"][names["fc.weight"]].clone().requires_grad_()
    b = r[0]["before"][names["fc.bias"]].clone().requires_grad_()
    emb = r[0]["before"][names["emb"]].clone().requires_grad_()
    fi = O.l2_normalize(O.linear(pooled, w, b))
    ft = O.l2_normalize(O.embedding_meanpool(emb, tok, ln)[0])
    lpi, lpt = O.similarity_logits(fi, ft, torch.tensor(-math.log(0.07)))
    loss = O.contrastive_loss(lpi, lpt)[0]
    loss.backward()
    for i in range(world):
        assert abs(r[i]["losses"][0] - float(loss)) < 2e-4 * abs(float(loss)), (i, r[i]["losses"], float(loss))
        g = r[i]["grads"]
        assert maxrel(g[names["fc.weight"]], w.grad) < 2e-4, i
        assert maxrel(g[names["fc.bias"]], b.grad) < 2e-4, i
        assert maxrel(g[names["emb"]], emb.grad) < 2e-4, i
        # ONE feature all-gather (the stacked [2, B, E]) and one gradient bucket per step
        assert r[i]["collectives_per_step"] == {"all_gather": 1.0, "all_reduce": 1.0, "broadcast": 0.0}, r[i]["collectives_per_step"]
        assert r[i]["broadcasts_total"] == 1                     # rank 0's storage centres, once, at the first train-mode pass
        # every replica evaluates the same bf16 forward function: rank 0's calibrated storage centres, broadcast
        assert r[i]["centres"] is not None and torch.equal(r[i]["centres"], r[0]["centres"]), i
    for i in range(1, world):
        for k in names.values():                                                                  # replicas stay bit-identical
            assert torch.equal(r[0]["grads"][k], r[i]["grads"][k]), (k, i)
            assert torch.equal(r[0]["after1"][k], r[i]["after1"][k]), (k, i)
        assert r[0]["losses"] == r[i]["losses"]
    for k in names.values():
        assert not torch.equal(r[0]["after1"][k], r[0]["before"][k]), k
    assert r[0]["losses"][1] < r[0]["losses"][0] + 0.5


def test_two_ranks_global_negatives_n512_vs_oracle(tmp_path):
    _global_negatives_vs_oracle(tmp_path, 2)


def test_four_ranks_global_negatives_n1024_vs_oracle(tmp_path):
    """More than two ranks through the product's distributed path -- 4 ranks x 256 pairs, 1024 global negatives (gather order
    beyond a pair, own-row gradient products at [256, 1024] x [1024, 512], the replicated 1024^2 loss, SUM over 4 contributors),
    four processes sharing one GPU over gloo; the oracle evaluates the reference's loss on the concatenated features.  Four, not
    BASELINE configs[2]'s eight: with the pytest process the GPU stays open in at most five processes at once."""
    _global_negatives_vs_oracle(tmp_path, 4)


def test_two_ranks_spatial_embeddings_under_global_negatives_vs_oracle(tmp_path):
    """--embedding_type spatial with data-parallel GLOBAL negatives (reference multimodal.py:757-787 applied to the concatenated
    per-location / per-word rows; round 4 raised NotImplementedError here): two ranks x 4 pairs -> the 8 x 8 spatial logits on every
    rank.  The ranks' token matrices have DIFFERENT pad lengths (as the collate produces on real data): the product pads the word
    rows to parallel.common_text_length before the fixed-size gathers.  Oracle: the reference's spatial similarity + symmetric InfoNCE on the ranks' layer-4 maps and tokens, concatenated in rank
    order; loss identical on both ranks, gradients of the 1x1 projection and the word embeddings = the oracle's (SUM over ranks)."""
    import torch.nn.functional as F
    _run_ranks(["spatial_step", str(tmp_path)], world=2, timeout=900)
    r = [torch.load(tmp_path / f"rank{i}.pt", weights_only=False) for i in range(2)]
    for sim in ("max", "mean"):
        a, b = r[0][sim], r[1][sim]
        assert a["tok"].shape[1] != b["tok"].shape[1]                                             # ranks padded to different L
        Lc = max(a["tok"].shape[1], b["tok"].shape[1])                                            # (zero rows add nothing: any common L)
        for x in (a, b):
            x["tok"] = F.pad(x["tok"], (0, Lc - x["tok"].shape[1]), value=0)
        assert not torch.equal(a["tok"], b["tok"])                                                # different shards
        for k, v in a["params"].items():
            assert torch.equal(v, b["params"][k]), k                                               # identical replicas
        fmap = torch.cat([a["fmap"], b["fmap"]])
        tok, ln = torch.cat([a["tok"], b["tok"]]), torch.cat([a["len"], b["len"]])
        w8 = a["params"]["vision_encoder.model.8.weight"].clone().requires_grad_()
        b8 = a["params"]["vision_encoder.model.8.bias"].clone().requires_grad_()
        emb = a["params"]["text_encoder.embedding.weight"].clone().requires_grad_()
        nlt = a["params"]["model.logit_neg_log_temperature"].clone().requires_grad_()
        feat = F.normalize(F.conv2d(fmap, w8, b8), p=2, dim=1)
        txt = F.normalize(F.embedding(tok, emb, padding_idx=0), p=2, dim=-1)
        lpi, lpt = O.spatial_similarity_logits(feat, txt, ln, nlt, sim)
        assert lpi.shape == (8, 8)
        loss = O.contrastive_loss(lpi, lpt)[0]
        loss.backward()
        for x in (a, b):
            assert abs(x["loss"] - float(loss)) < 2e-4 * max(1.0, abs(float(loss))), (sim, x["loss"], float(loss))
            g = x["grads"]
            assert maxrel(g["vision_encoder.model.8.weight"], w8.grad) < 5e-4, sim
            assert maxrel(g["vision_encoder.model.8.bias"], b8.grad) < 5e-4, sim
            assert maxrel(g["text_encoder.embedding.weight"], emb.grad) < 5e-4, sim
            assert abs(float(g["model.logit_neg_log_temperature"]) - float(nlt.grad)) < 5e-4 * max(1.0, abs(float(nlt.grad))), sim
            assert x["all_gathers"] == 3                                                           # image rows, text rows, lengths
        for k in a["grads"]:
            assert torch.equal(a["grads"][k], b["grads"][k]), (sim, k)


def test_rccl_world1_drives_the_whole_multi_gpu_path_bit_identically(tmp_path):
    """The RCCL branch on the one GPU there is: a world-size-1 ``nccl`` process group with $CVCL_FORCE_DIST=1 runs the feature
    all-gather (all_gather_into_tensor), the bucketed all-reduce launched from the gradient hooks / from trunk_train's side
    stream, OverlappedUpdate and the two trunk streams.  With one rank every collective is the identity, so losses, parameters
    and BatchNorm buffers must equal the plain single-process schedule bit for bit -- any missing stream edge (a collective
    reading a bucket before its producer stream has written it, an update applied before the wait) breaks that."""
    env = dict(os.environ)
    for k in ("RANK", "WORLD_SIZE", "LOCAL_RANK", "CVCL_DIST_BACKEND"):
        env.pop(k, None)
    env.update(MASTER_ADDR="127.0.0.1", MASTER_PORT=str(_free_port()), HSA_ENABLE_IPC_MODE_LEGACY="0")
    r = subprocess.run([sys.executable, WORKER, "rccl_w1", str(tmp_path)], env=env, capture_output=True, text=True, timeout=900)
    assert r.returncode == 0, r.stdout[-3000:] + r.stderr[-3000:]
    res = torch.load(tmp_path / "w1.pt", weights_only=False)
    assert res["librccl_mapped"]
    for mode in ("frozen", "finetune"):
        a, b = res[mode + "_dist"], res[mode + "_plain"]
        assert a["losses"] == b["losses"], (mode, a["losses"], b["losses"])
        assert a["losses"][-1] < a["losses"][0]
        for k, v in a["state"].items():
            assert torch.equal(v, b["state"][k]), (mode, k)


COMMON = ("--dataset synthetic --text_encoder embedding --embedding_dim 64 --vit_dino --normalize_features --fix_temperature "
          "--optimize_unused --checkpoint_callback False --logger False --max_epochs 1 --limit_train_batches 2 "
          "--check_val_every_n_epoch 100 --lr 1e-3 --weight_decay 0.1 --precision 32 --seed 3")


def _single_process(tmp_path, extra, batch):
    out = tmp_path / "single"
    out.mkdir()
    env = dict(os.environ)
    for k in ("RANK", "WORLD_SIZE", "LOCAL_RANK"):
        env.pop(k, None)
    cmd = [sys.executable, WORKER, "train", str(out), "--"] + (COMMON + f" --gpus 1 --batch_size {batch} " + extra).split()
    r = subprocess.run(cmd, env=env, capture_output=True, text=True, timeout=600)
    assert r.returncode == 0, r.stdout[-3000:] + r.stderr[-3000:]
    return torch.load(out / "rank0.pt", weights_only=False)


@pytest.mark.parametrize("extra", ["--lambda_lm 0", "--lambda_lm 0.5"])
def test_trainer_fit_two_ranks_equals_single_process_on_the_global_batch(tmp_path, extra):
    """Frozen ViT trunk (no BatchNorm: a rank's features do not depend on its shard-mates), global negatives: two ranks x B
    take exactly the optimizer steps of one process on the 2B batch -- each rank reads its own shard (DistributedSampler),
    InfoNCE gradients are summed, and the rank-local LM mean enters with 1 / world."""
    B = 4
    two = tmp_path / "two"
    two.mkdir()
    _run_ranks(["train", str(two), "--"] + (COMMON + f" --gpus 2 --batch_size {B} " + extra).split())
    r = [torch.load(two / f"rank{i}.pt", weights_only=False) for i in range(2)]
    ref = _single_process(tmp_path, extra, 2 * B)
    assert r[0]["global_step"] == r[1]["global_step"] == ref["global_step"] == 2
    for k, v in ref["params"].items():
        assert torch.equal(r[0]["params"][k], r[1]["params"][k]), k
        d = float((r[0]["params"][k] - v).abs().max())
        assert d < 2e-5 * max(1.0, float(v.abs().max())), (k, d)


def test_trainer_fit_local_negatives_averages_gradients(tmp_path):
    """--local_negatives = Lightning-DDP semantics: each rank's own B x B loss, gradients averaged.  Same update as a single
    process that averages the two half-batch gradients (computed here with the product itself, one half at a time)."""
    import contextlib
    import io
    B = 4
    two = tmp_path / "two"
    two.mkdir()
    argv = (COMMON + f" --gpus 2 --batch_size {B} --lambda_lm 0 --local_negatives --limit_train_batches 1").split()
    _run_ranks(["train", str(two), "--"] + argv)
    r = [torch.load(two / f"rank{i}.pt", weights_only=False) for i in range(2)]
    # single-process emulation: build the same model, run the two shards, average, step
    import train as train_entry
    from multimodal import lightning as pl
    from multimodal.multimodal import TextEncoder, VisionEncoder
    from multimodal.multimodal_data_module import SyntheticDataModule
    from multimodal.multimodal_lit import MultiModalLitModel
    args = train_entry._setup_parser().parse_args((COMMON + f" --gpus 1 --batch_size {B} --lambda_lm 0 --local_negatives").split())
    pl.seed_everything(args.seed)
    with contextlib.redirect_stdout(io.StringIO()):
        data = SyntheticDataModule(args)
        ve = VisionEncoder(args=args)
        lit = MultiModalLitModel(ve, TextEncoder(data.read_vocab(), ve.last_cnn_out_dim, args=args), args)
    dev = torch.device("cuda:0")
    lit.to(dev).train()
    lit.set_precision("32")
    opt = lit.configure_optimizers()
    data.setup()
    from multimodal.multimodal_data_module import multiModalDataset_collate_fn
    shards = [[data.train_set[rk + 2 * i] for i in range(B)] for rk in range(2)]                   # DistributedSampler(shuffle=False)
    grads = []
    for items in shards:
        x, y, ln, raw = multiModalDataset_collate_fn(items)
        opt.zero_grad(set_to_none=True)
        out = lit.training_step((x.to(dev), y.to(dev), ln.to(dev), raw), 0)
        out["loss"].backward()
        grads.append({k: v.grad.clone() for k, v in lit.named_parameters() if v.grad is not None})
    opt.zero_grad(set_to_none=True)
    for k, v in lit.named_parameters():
        if k in grads[0]:
            v.grad = (grads[0][k] + grads[1][k]) / 2
    opt.step()
    for k, v in lit.named_parameters():
        if v.requires_grad and k in r[0]["params"]:
            assert torch.equal(r[0]["params"][k], r[1]["params"][k]), k
            d = float((r[0]["params"][k] - v.detach().cpu()).abs().max())
            assert d < 2e-5 * max(1.0, float(v.abs().max())), (k, d)


def test_bench_spawns_its_own_ranks(tmp_path):
    """``python bench.py --gpus 2 --full`` outside torch.distributed.run starts two fresh ranks itself (before touching the GPU)
    and rank 0 prints the one JSON line with the whole-job throughput, the parity figures and the collectives' timings."""
    import json
    env = dict(os.environ)
    env.update(CVCL_DIST_BACKEND="gloo", CVCL_TRUNK_STREAMS="1")          # two ranks share this box's one GPU
    for k in ("RANK", "WORLD_SIZE", "LOCAL_RANK", "MASTER_PORT"):
        env.pop(k, None)
    r = subprocess.run([sys.executable, os.path.join(ROOT, "bench.py"), "--gpus", "2", "--steps", "3", "--warmup", "1", "--full",
                        "--no-cpu-baseline", "--no-roofline"], env=env, capture_output=True, text=True, timeout=900)
    assert r.returncode == 0, r.stdout[-2000:] + r.stderr[-3000:]
    lines = [l for l in r.stdout.splitlines() if l.startswith("{")]
    assert len(lines) == 1
    line = json.loads(lines[0])
    assert line["n_gpus"] == 2 and line["config"]["global_batch"] == 512 and line["config"]["trunk_streams"] == 1
    assert line["value"] > 0 and line["config"]["negatives"].startswith("global") and "logits_rel_vs_fp32" in line
    # the self-verification block of a multi-rank line (what the first 8-GPU RCCL run will be read by)
    d = line["distributed"]
    assert d["backend"] == "gloo" and d["ranks_seen"] == 2 and [x["rank"] for x in d["ranks"]] == [0, 1]
    assert d["shared_devices"] is True and d["ranks"][0]["device"] == d["ranks"][1]["device"]        # (this box: two ranks, one GPU, gloo)
    assert d["allgather_us"] > 0 and d["allreduce_us"] > 0
    assert 0 < d["ms_per_step_per_rank"]["min"] <= d["ms_per_step_per_rank"]["max"] <= line["ms_per_step"] * 1.0001


def test_bench_refuses_two_rccl_ranks_on_one_device():
    """A rank whose LOCAL_RANK has no device of its own must not silently wrap onto device 0 under RCCL (the mis-launch would
    still print a throughput line): bench.py exits non-zero before it initialises the process group."""
    env = dict(os.environ)
    env.update(RANK="1", WORLD_SIZE="2", LOCAL_RANK=str(torch.cuda.device_count()), MASTER_ADDR="127.0.0.1", MASTER_PORT="29999")
    env.pop("CVCL_DIST_BACKEND", None)
    r = subprocess.run([sys.executable, os.path.join(ROOT, "bench.py"), "--gpus", "2", "--steps", "1", "--warmup", "0"], env=env,
                       capture_output=True, text=True, timeout=300)
    assert r.returncode != 0 and "one rank per GPU" in (r.stderr + r.stdout)
    assert not [l for l in r.stdout.splitlines() if l.startswith("{")]
