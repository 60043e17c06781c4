"""cvcl_gemm over the routing case table (tests/gemm_route_cases.py): whatever kernel plan_gemm picks, the call writes exactly the
statistics rows cvcl_gemm_stats_rows announced and refuses a buffer one row short (the refusals that need no device:
tests/test_gemm_route_abi.py)."""
import ctypes as C

import pytest
import torch

from multimodal import _hip as H

import gemm_route_cases as T

WITH_ROWS = [c for c in T.CASES if c.get("stats") == "rows"]


def _short_message(lib, c, rows):
    """the refusal of a buffer of rows - 1: a block the streaming / 8-wave kernel would have taken goes on to the 128 x 128 kernels,
    which refuse it against their own grid_m (or, statistics-only behind a BN operand, have no kernel for it)"""
    if c["dt"] == T.F32X3:
        return f"cvcl_gemm(CVCL_F32X3): stats_rows {rows - 1} < {rows} (partial rows only)"
    if c.get("no_C") and c.get("prologue"):
        return "cvcl_gemm: statistics-only / BN-tail epilogues need the direct-to-LDS bf16 path"
    return f"cvcl_gemm: stats_rows {rows - 1} < grid_m {lib.cvcl_gemm_grid_m(c['dt'], c['M'], c['N'], 0)}"


@pytest.mark.gpu
@pytest.mark.parametrize("c", WITH_ROWS, ids=[c["tag"] for c in WITH_ROWS])
def test_stats_rows_written_exactly(c):
    lib = H.lib()
    b = T.GpuBlock(lib, c)
    rows, stats = b.args.stats_rows, b.t["stats"]
    assert stats.shape[0] == rows + 1 and torch.isnan(stats).all()
    H.check(lib.cvcl_gemm(c["dt"], C.byref(b.args), H.stream_ptr()), c["tag"])
    torch.cuda.synchronize()
    assert torch.isfinite(stats[:rows]).all(), "rows cvcl_gemm_stats_rows announced were not all written"
    assert torch.isnan(stats[rows]).all(), "a row past cvcl_gemm_stats_rows was written"
    b.args.stats_rows = rows - 1
    assert lib.cvcl_gemm(c["dt"], C.byref(b.args), H.stream_ptr()) != 0
    assert lib.cvcl_last_error().decode() == _short_message(lib, c, rows)
