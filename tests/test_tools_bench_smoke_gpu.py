"""Every tool under tools/ that times through tools/timing.py and has a ``main(argv)`` runs once, in-process, at the smallest shapes
its kernels accept.  This proves that the tools run and that every timed entry of their JSON line carries its median, minimum and
maximum under the one naming scheme (K, min_K, max_K).  The sizes are toys: the figures mean nothing and are not recorded."""
import importlib
import json
import math
import os
import sys

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(ROOT, "tools"))

pytestmark = pytest.mark.gpu

QUICK = ["--repeats", "2", "--window-ms", "2"]
VIT = ["--batch", "2", "--model", "2x32x2x32", "--patches", "8", "--dtypes", "bf16,f32"]        # depth 2, width 32, 2 heads, 32 x 32

# tool -> (arguments, timed key paths, other key paths): the keys the tool's README row names; "*" = every element of a list.  A timed
# path ends at a median K and must have min_K and max_K beside it.
CASES = {
    "bench_alignment": (["--shapes", "64x32x4"] + QUICK,
                        ["shapes/64x32x4/hip_chain/us", "shapes/64x32x4/torch_chain/us", "shapes/64x32x4/hip_class_means/us",
                         "shapes/64x32x4/hip_cosine_self/us", "shapes/64x32x4/hip_pearson/us"],
                        ["shapes/64x32x4/class_means_GBps", "shapes/64x32x4/chain_speedup_over_torch"]),
    "bench_neighbors": (["--nq", "8", "--nb", "64", "--pixel-nb", "64", "--size", "32", "--dim", "64"] + QUICK,
                        ["cosine_nb64/ms", "cosine_nb64/grouped22_ms", "cosine_nb64/eager_slice_ms", "cosine_nb64/eager_per_category_ms",
                         "pixels_nb64/ms", "pixels_nb64/eager_slice_ms"],
                        ["cosine_nb64/queries_per_s", "cosine_nb64/fraction_of_fp32_mfma_peak", "cosine_nb64/eager_scaled_ms",
                         "cosine_nb64/speedup_vs_eager", "pixels_nb64/sad_lane_instructions_per_s", "pixels_nb64/eager_scaled_ms"]),
    "bench_knn": (["--nq", "8", "--nb", "64", "--k", "1,5", "--dim", "64", "--classes", "10"] + QUICK,
                  ["nb64/k1/knn_cosine_ms", "nb64/k5/nearest_cosine_ms", "nb64/k5/knn_vote_ms", "nb64/k5/eager_topk_ms", "nb64/k5/eager_vote_ms",
                   "adversary_130x1500x64_k64/ascending_ms", "adversary_130x1500x64_k64/shuffled_ms"],
                  ["nb64/k5/over_nearest_cosine", "nb64/k5/speedup_vs_eager_topk"]),
    "bench_hash": (["--nq", "8", "--nb", "48", "--frames", "16", "--size", "32", "--eager-chunk", "8", "--ratio-slice", "2",
                    "--ratio-base-slice", "16"] + QUICK,
                   ["hash/ms", "hash/nhwc_ms", "hash/eager_ms", "hamming/ms", "hamming/grouped22_ms", "hamming/eager_ms", "digit_ratio/ms",
                    "digit_ratio/grouped22_ms", "digit_ratio/grouped22_sorted_ms"],
                   ["hash/equals_eager", "hamming/equals_eager", "digit_ratio/host_dp_scaled_ms", "digit_ratio/equals_host_dp"]),
    "bench_vit_attention": (VIT + QUICK,
                            ["cases/*/get_last_selfattention/hip/ms", "cases/*/get_last_selfattention/eager_torch/ms",
                             "cases/*/vit_cls_attention/hip/ms", "cases/*/get_intermediate_layers_2/hip/ms", "cases/*/kernel_q_rows_T/ms",
                             "cases/*/kernel_q_rows_1/ms"],
                            ["cases/*/kernel_q_rows_1/write_gbs", "cases/*/vit_cls_attention/speedup"]),
    "bench_vit_rollout": (VIT + ["--discard_ratio", "0.5"] + QUICK,
                          ["cases/*/vit_attention_rollout/ms", "cases/*/eager_torch/ms", "cases/*/vit_cls_attention/ms",
                           "cases/*/vit_attention_rollout_discard/ms", "cases/*/kernel_head_fuse/ms", "cases/*/kernel_rollout_q_rows_1/ms",
                           "cases/*/kernel_discard/copy/ms", "cases/*/kernel_discard/copy_discard/ms",
                           "cases/*/kernel_discard/copy_eager_discard/ms"],
                          ["cases/*/speedup_vs_eager", "cases/*/kernel_head_fuse/gbs", "cases/*/kernel_rollout_q_rows_T/slab_gbs"]),
    "bench_word_statistics": (["--loop-batches", "1"] + QUICK,
                              ["hip_accumulate/us", "torch_accumulate/us", "hip_topk/us", "torch_topk/us"],
                              ["accumulate_GBps", "topk_GBps", "loop/bitwise_equal"]),
    "bench_ngram": (["--tokens", "20000", "--loop-batches", "1", "--orders", "3"] + QUICK,
                    ["N3/keys_kernel/us", "N3/ce_loss_kernel/us", "N3/probs_kernel/us", "N3/update/us", "N3/calculate_ce_loss/us",
                     "N3/torch_ce_loss/us", "N3/rebuild/s"],
                    ["N3/loop/speedup", "N3/torch_over_hip"]),
    "bench_clip": (["--batches", "2", "--launches", "3", "--tower", "2x64x8x32"],
                   ["c_fc_quick_gelu_us", "c_fc_gelu_us", "c_fc_none_us", "hip_32_B2_ms", "hip_bf16_B2_ms", "torch_fp32_B2_ms",
                    "torch_autocast_bf16_B2_ms"],
                   ["hip_32_B2_img_s", "c_fc_quick_gelu_over_gelu"]),
    "bench_frame_store": (["--files", "256", "--steps", "1", "--warmup", "1", "--workers", "0", "--reps", "3"],
                          ["launch_identity/indexed/median_us", "launch_identity/plain/median_us", "launch_augment/indexed/median_us"],
                          ["host_frames_per_s", "device_frames_frames_per_s", "frame_store_frames_per_s", "launch_identity/plain/p90_us"]),
    "bench_caption_gradcam": (["--batch", "2", "--length", "4", "--launches", "2", "--loop_images", "1"],
                              ["a_loop/ms_per_map", "b_batched/ms", "seed_kernel/us", "seed_kernel/rotating_us"],
                              ["b_batched/launches", "b_batched/classes", "speedup_per_map", "seed_kernel/gb_per_s"]),
    "bench_linear_probe": (["--trials", "2", "--group", "2", "--size", "64", "--train-batches", "4"] + QUICK,
                           ["32_grouped_ms", "32_per_trial_ms", "32-split_grouped_ms", "train_32_B4_ms_per_step"],
                           ["32-split_speedup", "32_grouped_trials_per_s", "train_32-split_B4_images_per_s"]),
    "bench_gradcam": (["--batch", "2", "--vocab", "8", "--loop_images", "1"] + QUICK,
                      ["eval_forward_ms", "a_loop/ms_per_image", "b_diagonal_resized/ms", "c_all_pairs/ms"],
                      ["c_all_pairs/contraction_ms", "b_diagonal_resized/maps_per_s"]),
    "bench_textgen": (["--batch", "4", "--beam", "3", "--decode-length", "4"] + QUICK,
                      ["hip_ms_per_decode", "eager_ms_per_decode"],
                      ["captions_per_s", "hip_launches_per_decode", "speedup"]),
    "bench_split": (["--batch", "8"] + QUICK,
                    ["modes/32-split/ms_per_step", "modes/32/ms_per_step", "modes/bf16/ms_per_step"],
                    ["modes/32/pairs_per_s", "split_over_fp32_step", "split_vs_fp32/noise/logits_rel_vs_fp32", "split_kernel_ms_by_class"]),
}


def lookup(node, path):
    """every value at ``path`` ("a/b/*/c"; "*" fans out over a list)"""
    nodes = [node]
    for part in path.split("/"):
        nodes = [x for n in nodes for x in n] if part == "*" else [n[part] for n in nodes]
    return nodes


def timed_entries(node, found):
    """collects (median, min, max) of every timed entry below ``node``: a dict key K (or median_K) beside min_K and max_K"""
    if isinstance(node, dict):
        for k, v in node.items():
            if k.startswith("min_"):
                base = k[4:]
                median = node[base] if base in node else node["median_" + base]
                found.append((base, median, v, node["max_" + base]))
            timed_entries(v, found)
    elif isinstance(node, list):
        for v in node:
            timed_entries(v, found)
    return found


@pytest.mark.parametrize("tool", sorted(CASES))
def test_tool_runs_and_reports_median_min_max(tool, capsys):
    import torch
    argv, timed, other = CASES[tool]
    threads = torch.get_num_threads()
    try:
        importlib.import_module(tool).main(argv)
    finally:
        torch.set_num_threads(threads)                      # (bench_hash pins its host yardstick to one core)
    lines = [line for line in capsys.readouterr().out.splitlines() if line.startswith("{")]
    assert len(lines) == 1, lines
    res = json.loads(lines[0])
    for path in timed + other:
        assert lookup(res, path), path                      # a KeyError names a missing key; an empty fan-out fails here
    for path in timed:
        head, _, key = path.rpartition("/")
        base = key[len("median_"):] if key.startswith("median_") else key
        for parent in (lookup(res, head) if head else [res]):
            assert "min_" + base in parent and "max_" + base in parent, path
    found = timed_entries(res, [])
    assert len(found) >= len(timed)
    for base, median, lo, hi in found:
        assert all(isinstance(v, (int, float)) and math.isfinite(v) and v > 0 for v in (median, lo, hi)), (base, median, lo, hi)
        assert lo <= median <= hi, (base, median, lo, hi)
