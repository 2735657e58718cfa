"""The instantiation table of the regression network's kernels (tools/kernel_table.py), without a GPU: for every family, the
symbols its case list launches -- by the Python mirror of the dispatch -- are exactly the symbols the built libwhvi_hip.so
ships.  A new instantiation without a case fails here, and so does a case whose symbol is no longer shipped.  The GPU side
(tests/test_kernel_table_gpu.py) runs every case against float64 and checks the mirror against whvi_last_kernel."""
import os
import sys

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(ROOT, "tools"))
import kernel_table as kt  # noqa: E402


@pytest.fixture(scope="module")
def shipped():
    from shipped_isa import ShippedLibrary
    with ShippedLibrary() as lib:
        yield {f: {n for n in lib.kernels if kt.family(n) == f} for f in kt.FAMILIES}


@pytest.mark.parametrize("fam", kt.FAMILIES)
def test_case_list_reaches_exactly_the_shipped_instantiations(fam, shipped):
    reached = kt.reached(256)[fam]
    assert shipped[fam], f"no {fam} in the library"
    assert sorted(shipped[fam] - reached) == [], "shipped, but no case launches it"
    assert sorted(reached - shipped[fam]) == [], "a case launches it, but the library does not ship it"


@pytest.mark.parametrize("cus", [256, 304, 228, 80])
def test_cases_reach_both_sides_of_the_xcd_condition(cus):
    """For any CU count: each NT family has cases with and without the XCD-contiguous block order, and every instantiation
    is the same whatever the CU count (only B moves)."""
    sides = {"small_k_apply": set(), "row_dot": set()}
    for case in kt.CASES:
        c = kt.sized(case, cus)
        la = kt.launch(c, cus)
        if case["family"] in sides and la.nt:
            sides[case["family"]].add(la.xcd)
        if case.get("xcd") is not None:
            assert la.xcd == case["xcd"] and c["B"] - case["B"] < 1000 * max(1, (1 << 14) // c["S"]), case["id"]
    assert sides == {"small_k_apply": {True, False}, "row_dot": {True, False}}
    assert kt.reached(cus) == kt.reached(256)


def test_mirror_on_known_launches():
    """Launches whose grid and symbol the sources state: config 4's first layer (2048 blocks on 256 CUs: XCD order),
    the 2050-block small_k case of tests/test_layer_apply_gpu.py (no reorder), config 2's cached quarter-tile layer,
    and the long-stream bwd of config 4's share."""
    c4 = kt.small_k_apply(16, 45730, 1024, 2, 256)
    assert (c4.symbol, c4.grid, c4.xcd) == ("whvi::small_k_apply_kernel<float, 2, 1, true>", 2048, True)
    odd = kt.small_k_apply(5, 16387, 1024, 2, 256)
    assert (odd.grid, odd.xcd) == (2050, False)
    assert kt.small_k_apply(2, 50, 4096, 3, 256).symbol == "whvi::small_k_apply_kernel<float, 3, 4, false>"
    assert kt.diag_apply("float", 32, 4096, 9, kt.DIAG_X_SHARED).symbol == "whvi::diag_apply_kernel<float, 9, 4, false, true>"
    assert kt.diag_apply("float", 32, 8192, 9, kt.DIAG_X_SHARED).symbol == "whvi::diag_apply_kernel<float, 9, 16, true, true>"
    assert kt.diag_apply("float", 2, 9, 11, 0).symbol == "whvi::diag_apply_kernel<float, 11, 16, false, false>"
    bwd = kt.diag_apply_bwd("float", 16, 45730, 10, 0, True, 256)
    assert bwd.symbol == "whvi::diag_apply_bwd_kernel<float, 10, true, false, true>" and bwd.xcd and bwd.grid == 2048
    assert kt.row_dot(4, 40001, 9).symbol == "whvi::row_dot_kernel<float, 9, true>"
    with pytest.raises(ValueError):
        kt.mlp_apply(8, 1, 11)                      # 4 D (K + 4) bytes of LDS > 64 KiB
    with pytest.raises(ValueError):
        kt.mlp_apply_bwd(4, 3, 8)
