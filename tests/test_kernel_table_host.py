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


def _diag_fwd_cases():
    return [c for c in kt.CASES + kt.ORDER_CASES if c["family"] == "diag_apply"]


def test_diag_apply_cases_reach_the_three_block_orders():
    """diag_apply's forward walks its tiles in the plain, the XCD-contiguous or the sample-fastest order; the cases reach
    each, every order case takes the order and the grid it names, and the options (bias on and off, no mean row, relu_in,
    relu_out) each occur under each order."""
    orders = {kt.launch(c, 256).order for c in _diag_fwd_cases()}
    assert orders == {kt.ORDER_PLAIN, kt.ORDER_XCD, kt.ORDER_SAMPLE_FASTEST}
    seen = {o: set() for o in orders}
    for c in kt.ORDER_CASES:
        la = kt.launch(c, 256)
        assert (la.order, la.grid, la.nt) == (c["order"], c["grid"], True), c["id"]
        assert la.xcd == (la.order == kt.ORDER_XCD)
        seen[la.order] |= {("bias", c["bias"]), ("mean_plus", c["mean_plus"])}
        seen[la.order] |= {k for k in ("relu_in", "relu_out") if c[k]}
    for o, opts in seen.items():
        assert opts >= {("bias", True), ("bias", False), ("mean_plus", False), "relu_in", "relu_out"}, (kt.ORDER_NAMES[o], opts)
    # the order cases launch shipped instantiations only
    assert {kt.launch(c, 256).symbol for c in kt.ORDER_CASES} <= kt.reached(256)["diag_apply_kernel"]


def test_mirror_equals_the_order_query_on_every_diag_apply_case():
    """whvi_diag_apply_order is computed by the function the launch uses (diag_apply_launch) and needs no device: on every
    diag_apply case the mirror gives the same order, out of place and -- per-sample input -- in place."""
    from whvi_amd import _hip
    query = _hip.lib().whvi_diag_apply_order
    n = 0
    for c in _diag_fwd_cases():
        flags = c["tune"] | (kt.DIAG_X_SHARED if c["shared"] else 0)
        for in_place in ((False,) if c["shared"] else (False, True)):
            got = query(0 if c["dtype"] == "float" else 1, c["S"], c["B"], c["log2d"], flags, int(in_place))
            want = kt.diag_apply(c["dtype"], c["S"], c["B"], c["log2d"], flags, in_place).order
            assert got == want, (c["id"], in_place, got, want)
            n += 1
    assert n > 150
    # the in-place rule of the size dispatch: 192 MiB in place is cached (counted once), out of place it streams
    assert query(0, 12, 4096, 10, 0, 1) == kt.ORDER_PLAIN and kt.diag_apply("float", 12, 4096, 10, 0, True).nt is False
    assert query(0, 12, 4096, 10, 0, 0) == kt.ORDER_XCD and kt.diag_apply("float", 12, 4096, 10, 0, False).order == kt.ORDER_XCD
    # what whvi_diag_apply refuses before launching comes back as its error code; empty launches are plain
    assert query(0, 3, 5, 13, 0, 0) == -2 and query(1, 3, 5, 12, 0, 0) == -2 and query(0, 3, 5, 1, 0, 0) == -2
    assert query(2, 3, 5, 6, 0, 0) == -1 and query(0, -1, 5, 6, 0, 0) == -1 and query(0, 3, 5, 6, 1024, 0) == -1
    assert query(0, 3, 5, 6, kt.DIAG_X_SHARED, 1) == -5 and query(0, 1 << 20, 1 << 12, 6, 0, 0) == -2
    assert query(0, 0, 5, 6, 0, 0) == 0
    assert _hip.diag_apply_order(__import__("torch").float32, 16, 8192, 1024, _hip.DIAG_X_SHARED) == _hip.DIAG_ORDER_SAMPLE_FASTEST


def test_mirror_on_known_launches():
    """Launches whose grid and symbol the sources state: config 4's first layer (2048 blocks on 256 CUs: XCD order),
    the 2050-block small_k case of tests/test_layer_apply_gpu.py (no reorder), config 2's cached quarter-tile layer,
    and the long-stream bwd of config 4's share; the block orders of diag_apply's forward at config 2, config 4 and the
    three shared-input shapes the size dispatch sends to the sample-fastest order."""
    c4 = kt.small_k_apply(16, 45730, 1024, 2, 256)
    assert (c4.symbol, c4.grid, c4.xcd) == ("whvi::small_k_apply_kernel<float, 2, 1, true>", 2048, True)
    odd = kt.small_k_apply(5, 16387, 1024, 2, 256)
    assert (odd.grid, odd.xcd) == (2050, False)
    assert kt.small_k_apply(2, 50, 4096, 3, 256).symbol == "whvi::small_k_apply_kernel<float, 3, 4, false>"
    assert kt.diag_apply("float", 32, 4096, 9, kt.DIAG_X_SHARED).symbol == "whvi::diag_apply_kernel<float, 9, 4, false, true>"
    assert kt.diag_apply("float", 32, 8192, 9, kt.DIAG_X_SHARED).symbol == "whvi::diag_apply_kernel<float, 9, 16, true, true>"
    assert kt.diag_apply("float", 2, 9, 11, 0).symbol == "whvi::diag_apply_kernel<float, 11, 16, false, false>"
    c2 = kt.diag_apply("float", 32, 4096, 9, kt.DIAG_X_SHARED)              # config 2: 256 MiB written, cache-resident
    assert (c2.nt, c2.grid, c2.order) == (False, 16384, kt.ORDER_PLAIN)
    c4 = kt.diag_apply("float", 16, 45730, 10, 0)                           # config 4's square layer: 45 730 blocks
    assert (c4.nt, c4.grid, c4.order, c4.xcd) == (True, 45730, kt.ORDER_PLAIN, False)
    for S, B, L, grid in ((16, 8192, 10, 8192), (32, 8192, 9, 8192), (64, 8192, 11, 65536)):
        la = kt.diag_apply("float", S, B, L, kt.DIAG_X_SHARED)
        assert (la.nt, la.grid, la.order, la.xcd) == (True, grid, kt.ORDER_SAMPLE_FASTEST, False)
    # the ragged streaming shapes of tests/test_diag_apply_gpu.py: NT, but plain order for either kind of input
    for S, B, L, grid in ((32, 4099, 9, 4099), (5, 16385, 10, 5121)):
        for flags in (0, kt.DIAG_X_SHARED):
            la = kt.diag_apply("float", S, B, L, flags)
            assert (la.nt, la.grid, la.order) == (True, grid, kt.ORDER_PLAIN)
    bwd = kt.diag_apply_bwd("float", 16, 45730, 10, 0, True, 256)
    assert bwd.symbol == "whvi::diag_apply_bwd_kernel<float, 10, true, false, true>" and bwd.xcd and bwd.grid == 2048
    assert kt.row_dot(4, 40001, 9).symbol == "whvi::row_dot_kernel<float, 9, true>"
    with pytest.raises(ValueError):
        kt.mlp_apply(8, 1, 11)                      # 4 D (K + 4) bytes of LDS > 64 KiB
    with pytest.raises(ValueError):
        kt.mlp_apply_bwd(4, 3, 8)
