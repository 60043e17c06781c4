"""cvcl_gemm's refusals and probes over the routing case table (tests/gemm_route_cases.py), on dummy pointers: no device needed.
plan_gemm decides a refusal before any pointer is used or anything is launched; the only device calls before it are the cached
occupancy / CU-count queries, which fall back to fixed values without a device."""
import ctypes as C

import pytest

from multimodal import _hip as H

import gemm_route_cases as T

BAD_SHAPES = [c for c in T.REFUSALS if min(c["M"], c["N"], c["K"]) <= 0]


@pytest.mark.parametrize("c", T.REFUSALS, ids=[c["tag"] for c in T.REFUSALS])
def test_refusal_messages(c):
    lib = H.lib()
    a = T.build_args(lib, c, lambda *_: T.DUMMY)
    assert lib.cvcl_gemm(c["dt"], C.byref(a), None) != 0
    assert lib.cvcl_last_error().decode() == c["refuse"]


@pytest.mark.parametrize("c", BAD_SHAPES, ids=[c["tag"] for c in BAD_SHAPES])
def test_probes_of_a_bad_shape(c):
    """a block without a positive shape selects no kernel: the LayerNorm probe says no, and the row count is that of the tiled kernels'
    grid for M x N (which has no K), 0 where M or N is not positive"""
    lib = H.lib()
    a = T.build_args(lib, c, lambda *_: T.DUMMY)
    assert lib.cvcl_gemm_ln_supported(C.byref(a)) == 0
    want = lib.cvcl_gemm_grid_m(c["dt"], c["M"], c["N"], 0) if c["M"] > 0 and c["N"] > 0 else 0
    assert lib.cvcl_gemm_stats_rows(c["dt"], C.byref(a)) == want
