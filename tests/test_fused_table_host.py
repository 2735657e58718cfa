"""The instantiation table of the fused forward (tools/fused_table.py), without a GPU: the symbols its case list launches -- by
the Python mirror of fused_plan -- are exactly the fused_shs_kernel / fused_shs16_kernel symbols the built libwhvi_hip.so
ships (for float / double: the golden list); the mirror agrees with whvi_fused_shs_plan, the query that calls the function the
launch itself calls, on every case at three CU counts; every case is ragged, minimal and inside the memory cap; and the case
list covers every (instantiation class x block map) pair the dispatch can produce.  The GPU side
(tests/test_fused_table_gpu.py) runs every case, whole output, bit for bit."""
import os
import sys

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(ROOT, "tools"))
import fused_table as ft  # noqa: E402

GOLDEN = os.path.join(ROOT, "tests", "golden", "fused_shs_kernel_symbols_f32_f64.txt")
CUS = (256, 304, 64)


@pytest.fixture(scope="module")
def shipped():
    from shipped_isa import ShippedLibrary
    with ShippedLibrary() as lib:
        yield {n for n in lib.kernels if n.startswith("whvi::fused_shs_kernel<") or n.startswith("whvi::fused_shs16_kernel<")}


def test_case_list_reaches_exactly_the_shipped_instantiations(shipped):
    reached = ft.reached(256)
    assert len(shipped) >= 360, "the library ships fewer fused-forward instantiations than the golden list pins"
    assert reached & set(ft.UNREACHABLE) == set(), "a case launches a symbol reported unreachable"
    assert sorted(shipped - reached - set(ft.UNREACHABLE)) == [], "shipped, but no case launches it"
    assert sorted((reached | set(ft.UNREACHABLE)) - shipped) == [], "a case launches it, but the library does not ship it"
    assert ft.shipped() == shipped, "the mirror's statement of what the dispatch instantiates"
    golden = {line.strip() for line in open(GOLDEN) if line.strip()}
    assert len(golden) == 280
    assert {s for s in reached | set(ft.UNREACHABLE) if s.startswith("whvi::fused_shs_kernel<")} == golden
    # one case per symbol at least, and each case names the symbol it is there for
    assert {c["want_symbol"] for c in ft.CASES} == reached
    assert len({c["id"] for c in ft.CASES}) == len(ft.CASES)


@pytest.mark.parametrize("cus", CUS)
def test_mirror_equals_the_plan_query_on_every_case(cus):
    """whvi_fused_shs_plan is computed by fused_plan, which launch_fused / launch_fused16 call, and touches no device when the
    CU count is given: on every case, at every CU count, stage, nt, same_sample_blocks and grid are the mirror's."""
    from whvi_amd import _hip
    for spec in ft.SPECS:
        c = ft.sized(spec, cus)
        la = ft.launch(c, cus)
        got = _hip.fused_shs_plan(ft.DTYPE_CODE[c["dtype"]], c["rows"], c["log2d"], c["n_samples"], c["sample_stride"], c["group_rows"],
                                  c["axis"], ft.flags_of(c), c["in_place"], c["eye"], not c["c"], cus)
        assert got == (0, la.stage, int(la.nt), la.mode, la.grid), (c["id"], cus, got, la)
        assert ft.block_map(bool(got[2]), got[4], got[3]) == c["want_map"] == la.map, c["id"]
    assert ft.reached(cus) == ft.reached(256)
    assert ft.covered(cus) == ft.MATRIX


def test_plan_query_returns_the_launch_refusals_and_needs_no_device():
    """What whvi_fused_shs_ex_* refuses before it looks at a pointer's value comes back as the same code; an empty launch and
    the thread-per-row kernel of rows shorter than a chunk have no plan (stage 0, mode 0)."""
    from whvi_amd import _hip
    q = _hip.fused_shs_plan
    F32, F64, F16, BF16 = 0, 1, 2, 4
    assert q(F32, 4, 14, cus=256)[0] == -2 and q(F64, 4, 13, cus=256)[0] == -2 and "supported range" in _hip.last_error()
    assert q(F32, -1, 9, cus=256)[0] == -1 and q(3, 4, 9, cus=256)[0] == -1 and q(9, 4, 9, cus=256)[0] == -1
    assert q(F32, 4, 9, 0, cus=256)[0] == -1 and q(F32, 4, 9, 1, 0, cus=256)[0] == -1 and q(F32, 4, 9, 1, 1, 0, cus=256)[0] == -1
    assert q(F32, 1 << 32, 2, cus=256)[0] == -2 and "32 bits" in _hip.last_error()
    assert q(F32, 4, 9, 2, 2, flags=16, cus=256)[0] == -1 and "unknown fused flags" in _hip.last_error()
    assert q(F32, 4, 9, axis=2, cus=256)[0] == -1
    assert q(F32, 4, 9, 2, 2, flags=4, in_place=True, cus=256)[0] == -5 and "shared source" in _hip.last_error()
    assert q(F32, 4, 9, 2, 2, axis=0, flags=4, cus=256)[0] == -1 and q(F32, 4, 7, 2, 2, flags=4, cus=256)[0] == -1
    assert q(F32, 4, 9, 2, 2, flags=8, cus=256)[0] == -1 and "one-transform" in _hip.last_error()          # c given
    assert q(F32, 4, 9, 2, 2, flags=8, c_null=True, cus=256)[0] == 0
    assert q(F64, 4, 6, 2, 2, flags=8, c_null=True, cus=256)[0] == -1                                        # f64: 512-byte rows
    assert q(F32, 4, 9, src_null=True, cus=256)[0] == -1 and q(F32, 4, 3, group_rows=9, axis=0, src_null=True, cus=256)[0] == -1
    assert q(F32, 4, 3, group_rows=8, axis=0, src_null=True, cus=256)[0] == 0
    assert q(F32, 4, 9, in_place=True, src_null=True, cus=256)[0] == -1
    for half in (F16, BF16):
        assert q(half, 4, 9, axis=0, cus=256)[0] == -1 and "row-axis" in _hip.last_error()
        assert q(half, 4, 9, flags=4, cus=256)[0] == -1 and q(half, 4, 9, flags=8, c_null=True, cus=256)[0] == -1
        assert q(half, 4, 9, src_null=True, cus=256)[0] == -1 and q(half, 4, 2, cus=256)[0] == -2 and q(half, 4, 14, cus=256)[0] == -2
        assert q(half, 4, 9, cus=256) == (0, 0, 0, 0, 1)
    assert q(F32, 0, 9, cus=256) == (0, 0, 0, 0, 0)                                                          # empty batch
    assert q(F32, 0, 9, 2, 2, flags=12, c_null=True, cus=256) == (0, 0, 0, 0, 0)
    assert q(F32, 1000, 1, cus=256) == (0, 0, 0, 0, 4) and q(F32, 1000, 0, cus=256) == (0, 0, 0, 0, 4)       # thread per row
    assert ft.launch(dict(dtype="float", log2d=1, rows=1000, eye=False, axis=1), 256).grid == 4
    # the launches the sources quote: BASELINE config 3's order on f64 rows of 4096 takes mode 1 from 16 tiles per CU up
    assert q(F64, 64 * 4096, 12, 64, 1, flags=3, cus=256) == (0, 1, 1, 1, 65536)
    assert q(F64, 64 * 4096 + 1, 12, 64, 1, flags=3, cus=256) == (0, 0, 1, 0, 65537)
    assert q(F32, 64 * 8192, 11, 64, 8192, flags=4, cus=256) == (0, 1, 1, 2, 65536)                          # config 3, shared source
    # the same arguments on a smaller chip reach the tuned dispatch earlier: the CU count is the argument's, not a device's
    assert q(F32, 8 * 2048 + 1, 10, cus=64)[1] == 1 and q(F32, 8 * 2048 + 1, 10, cus=256)[1] == 0


def test_every_case_is_ragged_minimal_and_inside_the_memory_cap():
    for cus in CUS:
        for spec in ft.SPECS:
            c = ft.sized(spec, cus)
            la = ft.launch(c, cus)
            assert ft.in_regime(c, cus), c["id"]
            assert la.grid >= 3, (c["id"], "a first, a middle and a last block")
            # ragged: rows past the last whole block, a partial last tile where a tile holds several rows -- but modes 1 and 2
            # exist only on whole blocks (fused_plan: rows % (4 n_samples) == 0; rows == n_samples * sample_stride with
            # sample_stride a multiple of eight blocks' rows)
            assert ft.ragged(c) != c["whole_blocks"], c["id"]
            assert c["whole_blocks"] == (la.mode != 0 or "near_miss" in c), c["id"]
            assert la.mode == 0 or "near_miss" not in c, c["id"]
            assert c["n_samples"] in (3, 5, 7), c["id"]
            if c.get("near_miss") == "mode2":        # one term of mode 2's rule fails: eight-block groups
                rpb = ft.rows_per_block(c["dtype"], c["log2d"])
                assert c["shared"] and c["rows"] == 3 * c["sample_stride"] and c["sample_stride"] % rpb == 0
                assert (c["sample_stride"] // rpb) % 8 == 4, c["id"]
            if c.get("near_miss") == "mode1":        # one term of mode 1's rule fails: whole groups of 4 n_samples rows
                assert la.big and c["sample_stride"] == 1 and c["a_ps"] and c["rows"] % 4 == 0 and c["rows"] % 12 == 4, c["id"]
                assert not ft.small_tile(c["dtype"], c["log2d"]), c["id"]
            # minimal: at half the rows the launch is no longer the case's
            assert not ft.in_regime(ft.halved(c), cus), (c["id"], cus)
            assert ft.held_bytes(c) <= ft.MEMORY_CAP, (c["id"], ft.held_bytes(c) / 2 ** 20)
            if c["in_place"]:
                assert c["b"] and not c["shared"] and not c["eye"], c["id"]
            assert not (c["one"] and c["c"]) and (c["a"] or not c["a_ps"]) and (c["c"] or not c["c_ps"]), c["id"]


def test_the_case_list_covers_the_block_map_matrix_and_spreads_the_options():
    """Every (instantiation class x block map) the dispatch can produce has a case: mode 2 cached and streaming, mode 1 on a
    grid that is and is not a multiple of 8, xcd against plain for every streaming class.  Each option occurs on and off."""
    assert ft.covered(256) == ft.MATRIX
    maps = {}
    for c in ft.CASES:
        la = ft.launch(c, 256)
        maps.setdefault(la.map, set()).add(la.nt)
    assert maps == {"plain": {False, True}, "xcd": {True}, "sample-fastest": {False, True}, "plain+wave-strided": {False, True},
                    "xcd+wave-strided": {True}}
    for mode1 in ("float", "double"):
        grids = {ft.launch(c, 256).grid % 8 == 0 for c in ft.CASES if c["dtype"] == mode1 and "wave" in c["want_map"]
                 and ft.launch(c, 256).nt}
        assert grids == {True, False}, mode1
    for key, values in (("in_place", 2), ("a", 2), ("b", 2), ("c", 2), ("a_ps", 2), ("c_ps", 2), ("layout", 3), ("n_samples", 3)):
        for fam16 in (False, True):
            seen = {c[key] for c in ft.CASES if (ft.SIZE[c["dtype"]] == 2) == fam16}
            assert len(seen) == values, (key, fam16, seen)
    rows_axis = [c for c in ft.CASES if c["axis"] == ft.AXIS_ROW or c["eye"]]
    for eye in (False, True):
        assert {c["gr"] for c in rows_axis if c["eye"] == eye} == {"one", "odd", "D"}
    assert {c["sample_stride"] == 1 for c in ft.CASES} == {True, False}
