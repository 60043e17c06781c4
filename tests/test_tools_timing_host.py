"""tools/timing.py on a fake clock: the order of the windows, the calibration rule, the statistics, and that nothing else under
tools/ times with device events."""
import os
import statistics
import sys

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(ROOT, "tools"))
import timing  # noqa: E402


class FakeClock:
    """window(fn, calls) that runs nothing, logs (name, calls) and returns ``per_call[name]`` ms per call"""

    def __init__(self, fns, per_call):
        self.names = {id(fn): name for name, fn in fns.items()}
        self.per_call, self.log = per_call, []

    def __call__(self, fn, calls):
        name = self.names[id(fn)]
        self.log.append((name, calls))
        return self.per_call[name]


def sides(*names):
    count = {n: 0 for n in names}

    def make(n):
        def fn():
            count[n] += 1
        return fn
    return {n: make(n) for n in names}, count


def test_sides_alternate_round_by_round():
    fns, count = sides("hip", "eager", "floor")
    clock = FakeClock(fns, {"hip": 1.0, "eager": 4.0, "floor": 0.5})
    res = timing.measure(fns, repeats=4, window_ms=200.0, warmup=3, window=clock)
    probe = [("hip", 1), ("hip", 5), ("eager", 1), ("eager", 5), ("floor", 1), ("floor", 5)]     # after each side's warm-up, in order
    assert clock.log[:6] == probe
    rounds = clock.log[6:]
    assert [n for n, _ in rounds] == ["hip", "eager", "floor"] * 4
    for name in fns:
        assert [c for n, c in rounds if n == name] == [res[name]["calls"]] * 4
    assert count == {"hip": 3, "eager": 3, "floor": 3}            # the fake clock runs nothing: only the warm-up calls ran
    assert list(res) == ["hip", "eager", "floor"]


@pytest.mark.parametrize("per_call_ms, want_calls, want_probe", [
    (0.002, 20000, [1, 5]),         # 2 us: 100 000 calls would fill the window -> the clamp
    (1.0, 200, [1, 5]),             # 1 ms -> 200 calls
    (250.0, 1, [1]),                # slower than the window: one call, found by the single probe call and not run again
    (200.0, 1, [1]),                # exactly the window counts as filling it
    (150.0, 1, [1, 5]),             # just under: probed with five, still one call
])
def test_calibration(per_call_ms, want_calls, want_probe):
    fns, _ = sides("s")
    clock = FakeClock(fns, {"s": per_call_ms})
    assert timing.calls_for(fns["s"], 200.0, window=clock) == want_calls
    assert [c for _, c in clock.log] == want_probe


def test_fixed_calls_suppress_the_probe():
    fns, _ = sides("a", "b")
    clock = FakeClock(fns, {"a": 1.0, "b": 1.0})
    res = timing.measure(fns, repeats=2, calls=1, window=clock)
    assert clock.log == [("a", 1), ("b", 1)] * 2 and res["a"]["calls"] == res["b"]["calls"] == 1
    clock = FakeClock(fns, {"a": 1.0, "b": 1.0})
    res = timing.measure(fns, repeats=2, window_ms=10.0, calls={"a": 7}, window=clock)            # b is not named: it is probed
    assert clock.log == [("b", 1), ("b", 5)] + [("a", 7), ("b", 10)] * 2
    assert (res["a"]["calls"], res["b"]["calls"]) == (7, 10)


def test_statistics_are_those_of_the_samples():
    fns, _ = sides("a", "b")
    script = {"a": iter([3.0, 1.0, 2.0, 10.0, 4.0]), "b": iter([5.0, 5.5, 4.5, 6.0, 5.0])}
    res = timing.measure(fns, repeats=5, calls=2, window=lambda fn, calls: next(script["a" if fn is fns["a"] else "b"]))
    assert res["a"]["samples"] == [3.0, 1.0, 2.0, 10.0, 4.0] and res["b"]["samples"] == [5.0, 5.5, 4.5, 6.0, 5.0]
    for r in res.values():
        assert len(r["samples"]) == 5
        assert (r["ms"], r["min_ms"], r["max_ms"]) == (statistics.median(r["samples"]), min(r["samples"]), max(r["samples"]))
    assert res["a"]["ms"] == 3.0 and res["a"]["max_ms"] == 10.0
    assert timing.entry(res["a"], "us", 1e3) == {"us": 3000.0, "min_us": 1000.0, "max_us": 10000.0}
    assert timing.entries(res, digits=1) == {"a": 3.0, "min_a": 1.0, "max_a": 10.0, "b": 5.0, "min_b": 4.5, "max_b": 6.0}


def test_arguments_become_measure_keywords():
    import argparse
    ap = argparse.ArgumentParser()
    timing.add_arguments(ap)
    assert timing.keywords(ap.parse_args([])) == {"repeats": 7, "window_ms": 200.0}
    assert timing.keywords(ap.parse_args(["--repeats", "3", "--window-ms", "5"])) == {"repeats": 3, "window_ms": 5.0}


def test_only_timing_py_times_with_device_events():
    tools = os.path.join(ROOT, "tools")
    hits = []
    for d, dirs, files in os.walk(tools):
        dirs[:] = [x for x in dirs if x != "__pycache__"]           # the interpreter's cache of timing.py itself
        for f in files:
            p = os.path.join(d, f)
            if os.path.relpath(p, tools) == "timing.py":
                continue
            with open(p, errors="replace") as fh:
                text = fh.read()
            if "enable_timing" in text or "elapsed_time" in text:
                hits.append(os.path.relpath(p, ROOT))
    assert hits == []
