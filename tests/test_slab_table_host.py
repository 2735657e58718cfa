"""The case list of the slab-walking kernels (tools/slab_table.py), without a GPU.

Six kernel templates share fused_bwd_geom (whvi_amd/csrc/fused_bwd.hpp): a block of four waves owns a sample's slab of rows and
each wave walks it one tile at a time.  Before this list, every shape on which the suite compared their VALUES with anything
gave each wave exactly one tile, and every such launch was cached -- ``test_the_older_shapes_stop_at_one_tile_per_wave`` states
that as a test, so this docstring stays true.  The list takes every shipped instantiation past that corner: a cached case with
at least three tiles per wave and a streaming (NT) case with at least two, both with a ragged last slab.  Here:

  * the symbols the list launches -- by the Python mirror -- are exactly the symbols the built libwhvi_hip.so ships, for the six
    templates and the three finishing kernels: a new instantiation without a case fails, naming it;
  * the mirror of the geometry against the library's workspace queries (S * n_slabs * part_floats * 4), on every case and on a
    few hundred seeded (S, B, log2d) triples;
  * the regimes: what ``walk`` and ``stream`` promise, and that each family meets each option in both.

tests/test_slab_table_gpu.py runs every case against float64 and checks the mirror against whvi_last_kernel."""
import os
import random
import sys

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(ROOT, "tools"))
import slab_table as st  # noqa: E402


@pytest.fixture(scope="module")
def shipped():
    from shipped_isa import ShippedLibrary
    with ShippedLibrary() as lib:
        yield {f: {n for n in lib.kernels if st.family(n) == f} for f in st.FAMILIES}


@pytest.mark.parametrize("fam", st.FAMILIES)
def test_case_list_reaches_exactly_the_shipped_instantiations(fam, shipped):
    reached = st.reached()[fam]
    assert shipped[fam], f"no {fam} in the library"
    assert sorted(shipped[fam] - reached) == [], "shipped, but no case launches it"
    assert sorted(reached - shipped[fam]) == [], "a case launches it, but the library does not ship it"


def test_the_list_is_two_cases_per_instantiation():
    assert len(st.CASES) == 186 and len({c["id"] for c in st.CASES}) == 186
    assert sum(len(s) for f, s in st.reached().items() if f in st.KERNEL_FAMILIES) == 186
    by_args = {}
    for c in st.CASES:
        sym = st.launch(c).symbol
        by_args.setdefault(sym.rsplit(", ", 1)[0], []).append((c["regime"], sym.rsplit(", ", 1)[1]))
    assert all(sorted(v) == [("stream", "true>"), ("walk", "false>")] for v in by_args.values()), by_args


def _part_floats(case):
    D = 1 << case["log2d"]
    if case["entry"] == "fused_shs_bwd":
        return 3 * D
    if case["entry"] == "fused_shs_stacked_bwd":
        return 3 * D * case["J"]
    return (4 if case["bias"] else 3) * D * case["J"]


def test_geometry_mirror_against_the_workspace_queries():
    """The workspace queries need no device and size S * n_slabs slots with the launch's own fused_bwd_geom."""
    from whvi_amd import _hip
    L = _hip.lib()
    n = 0
    for c in st.CASES:
        S, B, log2d = c["S"], c["B"], c["log2d"]
        if not c["entry"].endswith("_bwd"):
            continue
        want = S * st.fused_bwd_geom(S, B, log2d)[0] * _part_floats(c) * 4
        if c["entry"] == "fused_shs_bwd":
            got = L.whvi_fused_shs_bwd_workspace(S, B, log2d)
        elif c["entry"] == "fused_shs_stacked_bwd":
            got = L.whvi_fused_shs_stacked_bwd_workspace(S, B, log2d, c["J"])
        else:
            got = L.whvi_fused_shs_stacked_layer_bwd_workspace(S, B, log2d, c["J"], int(c["bias"]))
        assert int(got) == want, (c["id"], int(got), want)
        assert st.launch(c).grid == S * st.fused_bwd_geom(S, B, log2d)[0]
        n += 1
    assert n == 42 + 32 + 64
    rng = random.Random(20240)
    for i in range(400):
        log2d = rng.randint(st.MIN_LOG2D, st.MAX_LOG2D)
        S = rng.choice((1, 2, 3, 5, 8, 16, 64, 341, 342, 1024, 1500))
        B = rng.choice((rng.randint(1, 70), rng.randint(1, 5000), rng.randint(1, 400000)))
        n_slabs, slab = st.fused_bwd_geom(S, B, log2d)
        rpt = st.fused_bwd_tile_rows(log2d)
        assert slab % rpt == 0 and (n_slabs - 1) * slab < B <= n_slabs * slab
        assert int(L.whvi_fused_shs_bwd_workspace(S, B, log2d)) == S * n_slabs * (3 << log2d) * 4, (S, B, log2d)
        J = 2 if log2d == 11 else 2 + i % 3
        if log2d <= 11:
            assert int(L.whvi_fused_shs_stacked_bwd_workspace(S, B, log2d, J)) == S * n_slabs * J * (3 << log2d) * 4, (S, B, log2d, J)


def test_tile_sizes():
    assert [st.fused_bwd_k(L) for L in range(6, 13)] == [4, 4, 4, 4, 4, 8, 16]
    assert [st.fused_bwd_k(L, 8) for L in range(6, 13)] == [2, 2, 2, 2, 2, 4, 8]
    assert [st.fused_bwd_tile_rows(L) for L in range(6, 13)] == [16, 8, 4, 2, 1, 1, 1]
    # the shapes the sources and the case list's description quote
    assert st.fused_bwd_geom(3, 4106, 10) == (316, 13) and st.last_slab_rows(3, 4106, 10) == 11
    assert st.fused_bwd_geom(3, 65681, 6) == (316, 208) and st.last_slab_rows(3, 65681, 6) == 161
    assert st.tiles_per_wave(8, 4096, 10) == 8                 # the peak-memory tests' shape: bytes asserted there, no values


def test_walk_cases_are_cached_and_walk_three_tiles():
    for c in (c for c in st.CASES if c["regime"] == "walk"):
        la = st.launch(c)
        assert la.nt is False and la.tiles_per_wave >= 3, (c["id"], la)
        assert c["S"] == 3 and st.ragged(c["S"], c["B"], c["log2d"]), c["id"]
        assert la.symbol.endswith(", false>")


def test_stream_cases_cross_the_threshold_by_little():
    for c in (c for c in st.CASES if c["regime"] == "stream"):
        la = st.launch(c)
        assert la.nt is True and la.tiles_per_wave >= 2, (c["id"], la)
        assert st.NT_MIN_BYTES < st.streamed_bytes(c) < 1.5 * st.NT_MIN_BYTES, (c["id"], st.streamed_bytes(c))
        assert c["S"] == 3 and st.ragged(c["S"], c["B"], c["log2d"]), c["id"]
        assert la.symbol.endswith(", true>")
        # the smallest batch that streams, but for the step to a ragged last slab
        assert st.streamed_bytes(dict(c, B=c["B"] - 1000)) <= st.NT_MIN_BYTES or c["B"] <= 1000, c["id"]


def test_every_family_meets_every_option_in_both_regimes():
    for entry in st.ENTRIES:
        for regime in ("walk", "stream"):
            mine = [c for c in st.CASES if c["entry"] == entry and c["regime"] == regime]
            keys = ["shared", "poison"] + (["need_x"] if entry.endswith("_bwd") else [])
            if entry.startswith("fused_shs_stacked_layer"):
                keys += ["bias", "relu_in", "relu_out"]
                assert {c["n_cols"] < c["J"] << c["log2d"] for c in mine} == {True, False}, (entry, regime, "narrowed")
                assert {c["ld"] > c["n_cols"] for c in mine} == {True, False}, (entry, regime, "pitch")
                for c in mine:
                    assert c["n_cols"] % 4 == 0 and (c["J"] - 1) << c["log2d"] < c["n_cols"] <= c["J"] << c["log2d"]
            for k in keys:
                assert {bool(c[k]) for c in mine} == {True, False}, (entry, regime, k)
            if "J" in mine[0]:
                assert len({c["J"] for c in mine}) >= 3, (entry, regime)


def test_the_older_shapes_stop_at_one_tile_per_wave():
    """The gap this list closes: on every shape the suite compared values on before it, at every supported D, no wave goes
    round its loop twice -- and none of these launches streams (a few hundred KiB at the most)."""
    for S, B in st.EXISTING_SHAPES:
        for log2d in range(st.MIN_LOG2D, st.MAX_LOG2D + 1):
            assert st.tiles_per_wave(S, B, log2d) == 1, (S, B, log2d)
            assert S * B * (4 << log2d) * 10 < st.NT_MIN_BYTES
    # and the slices tests/test_slab_table_gpu.py compares each case with are in that regime by construction
    for log2d in range(st.MIN_LOG2D, st.MAX_LOG2D + 1):
        assert st.tiles_per_wave(1, st.one_tile_rows(log2d), log2d) == 1
        assert st.tiles_per_wave(1, st.one_tile_rows(log2d) + 1, log2d) == 2
