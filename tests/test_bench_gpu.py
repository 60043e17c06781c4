"""GPU: a plain ``bench.py`` run (no ``--full``) prints the headline line alone -- throughput and step time of the timed steps,
nothing measured in passes of its own -- and writes what the last timed step computed under ``--dump-outputs``."""
import json
import os
import subprocess
import sys

import numpy as np
import pytest

from conftest import ROOT

pytestmark = pytest.mark.gpu


def test_plain_bench_prints_the_headline_only(tmp_path):
    out_dir = tmp_path / "outputs"
    r = subprocess.run([sys.executable, os.path.join(ROOT, "bench.py"), "--gpus", "1", "--steps", "2", "--warmup", "1",
                        "--dump-outputs", str(out_dir)], capture_output=True, text=True, timeout=600)
    assert r.returncode == 0, r.stdout[-2000:] + r.stderr[-3000:]
    lines = [l for l in r.stdout.splitlines() if l.startswith("{")]
    assert len(lines) == 1
    line = json.loads(lines[0])
    assert line["metric"].startswith("image-text pairs/sec") and line["unit"] == "pairs/s" and line["higher_is_better"] is True
    assert line["dtype"] == "bf16" and line["n_gpus"] == 1 and line["steps"] == 2 and line["warmup"] == 1
    assert line["value"] > 0 and line["ms_per_step"] > 0
    assert abs(line["value"] - 256 * 1e3 / line["ms_per_step"]) <= 1e-3 * line["value"]
    for k in ("parity", "logits_rel_vs_fp32", "roofline", "kernel_ms_per_step", "tail_ms_per_step", "fp32_parity_mode", "c4", "c5",
              "c4p14", "finetune_cnn", "cpu_baseline", "distributed"):
        assert k not in line, k
    got = {f[:-4]: np.load(out_dir / f) for f in os.listdir(out_dir)}
    assert "step.loss" in got and any(k.startswith("param.") for k in got) and any(k.startswith("grad.") for k in got)
    assert abs(float(got["step.loss"]) - line["final_loss"]) <= 1e-5 * max(1.0, abs(line["final_loss"]))
