"""tools/timing.py on the device: two real sides (device-to-device copies of 1 MiB and 16 MiB, plain torch ops) through ``window`` and
``measure``.  Nothing here says which side is faster: the machine is shared, and the test is about the helper."""
import math
import os
import sys

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(ROOT, "tools"))
import timing  # noqa: E402

pytestmark = pytest.mark.gpu

WARMUP, REPEATS = 3, 3
PROBE = 1 + 5          # timing.calls_for: one call, then (a copy of this size is far below the 5 ms window) one window of five


def test_window_and_measure_on_two_copies():
    import torch
    dev = torch.device("cuda:0")
    count, fns = {}, {}
    for name, nbytes in (("copy_1MiB", 1 << 20), ("copy_16MiB", 16 << 20)):
        src, dst = torch.zeros(nbytes, dtype=torch.uint8, device=dev), torch.empty(nbytes, dtype=torch.uint8, device=dev)
        count[name] = 0

        def fn(name=name, src=src, dst=dst):
            count[name] += 1
            dst.copy_(src)
        fns[name] = fn

    ms = timing.window(fns["copy_1MiB"], 10)
    assert math.isfinite(ms) and ms > 0 and count["copy_1MiB"] == 10
    count["copy_1MiB"] = 0

    res = timing.measure(fns, repeats=REPEATS, window_ms=5.0, warmup=WARMUP)
    assert list(res) == list(fns)
    for name, r in res.items():
        print(name, {k: r[k] for k in ("ms", "min_ms", "max_ms", "calls")})
        assert len(r["samples"]) == REPEATS
        assert all(math.isfinite(v) and v > 0 for v in r["samples"] + [r["ms"], r["min_ms"], r["max_ms"]])
        assert r["min_ms"] <= r["ms"] <= r["max_ms"]
        assert 1 <= r["calls"] <= 20000
        assert count[name] == WARMUP + PROBE + REPEATS * r["calls"]
