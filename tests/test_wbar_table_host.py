"""The instantiation table of the weight-construction kernels (tools/wbar_table.py), without a GPU.

wbar_fwd_kernel and wbar_bwd_kernel are the library's largest family: 246 instantiations over float / double, log2 D, quarter
and 16 KiB tiles, cached and non-temporal, the mean row, the two butterfly networks and the one-launch mean form.  Here:

  * the shipped symbols of the two templates are exactly ``reached() | UNREACHABLE`` (disjoint), and exactly what the mirror says
    the dispatch instantiates; none uses scratch.  A new instantiation without a case fails, naming it; so does a deleted case;
  * every case's sizes are in the regime its name claims, recomputed here from the byte constants alone;
  * every switch occurs both ways for every entry and type, R < D occurs at every D of every entry, and a last tile that is not
    full and a tile count that is no multiple of 4 occur for every (entry, type, NT);
  * the argument checks of the three dispatch functions that tests/test_abi.py does not pin answer before any device call.

tests/test_wbar_table_gpu.py runs every case and checks the mirror against whvi_last_kernel."""
import ctypes
import os
import sys

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(ROOT, "tools"))
import wbar_table as wt  # noqa: E402

MIB = 1 << 20


@pytest.fixture(scope="module")
def shipped():
    from shipped_isa import ShippedLibrary
    with ShippedLibrary() as lib:
        yield {n: k for n, k in lib.kernels.items() if n.startswith(("whvi::wbar_fwd_kernel<", "whvi::wbar_bwd_kernel<"))}


def test_case_list_reaches_exactly_the_shipped_instantiations(shipped):
    reached, unreachable = wt.reached(), set(wt.UNREACHABLE)
    assert len(shipped) == 246
    assert sorted(reached & unreachable) == [], "listed as unreachable, but a case launches it"
    assert sorted(set(shipped) - reached - unreachable) == [], "shipped, but no case launches it and UNREACHABLE does not list it"
    assert sorted((reached | unreachable) - set(shipped)) == [], "a case launches it or UNREACHABLE lists it, but it is not shipped"
    inst = wt.instantiated()
    assert inst["wbar_fwd_kernel"] | inst["wbar_bwd_kernel"] == set(shipped)
    assert [n for n, k in shipped.items() if k["scratch"]] == []
    assert all(reason for reason in wt.UNREACHABLE.values())


def test_counts():
    """The figures DESIGN.md quotes."""
    assert len(wt.CASES) == 268 and len({c["id"] for c in wt.CASES}) == 268
    reached = wt.reached()
    assert len(reached) == 216 and len(wt.UNREACHABLE) == 30
    count = lambda fam, T, pool: sum(1 for s in pool if s.startswith(f"whvi::{fam}<{T},"))  # noqa: E731
    inst = wt.instantiated()
    for T in ("float", "double"):
        assert count("wbar_fwd_kernel", T, inst["wbar_fwd_kernel"]) == 45 and count("wbar_fwd_kernel", T, reached) == 35
        assert count("wbar_bwd_kernel", T, inst["wbar_bwd_kernel"]) == (88 if T == "float" else 68)
        assert count("wbar_bwd_kernel", T, reached) == (78 if T == "float" else 68)
    nt = [s for s in reached if s.split(", ")[3].startswith("true")]               # the fourth template argument: NT
    assert len(nt) == 24 + 48
    # every reachable instantiation has a case of kind "inst": the boundary cases add none
    assert {wt.launch(c).shipped for c in wt.CASES if c["kind"] == "inst"} == reached


def _bytes(c):
    return c["J"] * c["S"] * c["R"] * (1 << c["log2d"]) * (4 if c["dtype"] == "float" else 8)


def _tiles(dtype, log2d):
    """(K, KS) from the register budget: 16 chunks of 16 bytes per lane, one row at least; a quarter of that, one row at least."""
    row_chunks = (1 << log2d) * (4 if dtype == "float" else 8) // 16
    need = max(row_chunks // 64, 1)
    return max(need, 16), max(need, 4)


def test_every_case_is_in_the_regime_it_claims():
    for c in wt.CASES:
        la, nb, D = wt.launch(c), _bytes(c), 1 << c["log2d"]
        K, KS = _tiles(c["dtype"], c["log2d"])
        assert (K, KS) == (wt.pick_k(c["dtype"], c["log2d"]), wt.small_k(c["dtype"], c["log2d"]))
        assert 1 <= c["R"] <= D and nb <= 1.3 * 256 * MIB or c["id"].endswith("_sliced") and nb <= 512 * MIB, c["id"]
        assert la.grid == -(-(-(-nb // (1024 * la.k))) // 4)
        if c["regime"] == "cached":
            assert not la.nt and nb < 256 * MIB, c["id"]
        if c["regime"] == "stream":
            assert la.nt and la.k == K and nb >= 256 * MIB, c["id"]
        if c["entry"] == "wbar_fwd_mean":
            assert la.k == KS and not la.nt and la.shipped.endswith(", false, true>")
        if c["entry"] == "wbar_fwd":
            if KS < K:
                assert (la.k, la.nt) == ((KS, False) if nb <= 256 * MIB else (K, True)), c["id"]
            else:
                assert (la.k, la.nt) == (K, nb >= 256 * MIB), c["id"]
            group = 1024 * la.k * 32                           # bytes of 8 x 4 tiles
            whole = c["R"] * D * (4 if c["dtype"] == "float" else 8) % group == 0
            assert (la.xcd_blocks > 0) == (la.nt and c["base"] and whole), c["id"]
            assert la.reorder == (la.nt and la.xcd_blocks == 0 and la.grid % 8 == 0)
            if c["id"].endswith("_sliced"):
                assert la.xcd_blocks == c["R"] * D * (4 if c["dtype"] == "float" else 8) // group and c["J"] * c["S"] >= 2
                assert la.grid == 8 * la.xcd_blocks * c["J"] * c["S"]
            elif c["regime"] == "stream":
                assert la.xcd_blocks == 0 and c["R"] < D and not whole, c["id"]
        if c["entry"] == "wbar_bwd":
            small = KS < K and (c["tiles"] == "small" or (c["tiles"] is None and nb <= 256 * MIB))
            assert la.k == (KS if small else K), c["id"]
            assert la.nt == (not small and nb > 256 * MIB), c["id"]
            lds = not small and c["dtype"] == "float" and 8 <= c["log2d"] <= 12 and not c["no_lds"] and nb <= 128 * MIB
            assert la.policy == ("lds" if lds else "dpp"), c["id"]
            tag = c["id"].split("_")[3]
            if c["kind"] == "inst":
                assert {"small": small, "big": not small and not la.nt, "stream": la.nt}[tag], c["id"]
                if "_big_" in c["id"]:
                    assert c["id"].split("_")[4] == la.policy, c["id"]


def test_boundary_cases_sit_on_the_thresholds():
    by_id = {c["id"]: c for c in wt.CASES}
    sym = lambda i: wt.launch(by_id[i]).shipped.split("<")[1]  # noqa: E731
    assert _bytes(by_id["fwd_f32_L10_256MiB_exact"]) == 256 * MIB and _bytes(by_id["fwd_f32_L10_256MiB_above"]) == 256 * MIB + 4096
    assert sym("fwd_f32_L10_256MiB_exact") == "float, 10, 4, false, false>"           # KS < K: <= 256 MiB is small
    assert sym("fwd_f32_L10_256MiB_above") == "float, 10, 16, true, false>"
    assert sym("fwd_f64_L9_256MiB_exact") == "double, 9, 4, false, false>" and sym("fwd_f64_L9_256MiB_above") == "double, 9, 16, true, false>"
    assert _bytes(by_id["fwd_f32_L12_256MiB_below"]) == 256 * MIB - 16384
    assert sym("fwd_f32_L12_256MiB_below") == "float, 12, 16, false, false>"          # KS == K: >= 256 MiB streams
    assert sym("fwd_f32_L12_256MiB_exact") == "float, 12, 16, true, false>" == sym("fwd_f32_L12_256MiB_above")
    assert sym("fwd_f64_L11_256MiB_below") == "double, 11, 16, false, false>" and sym("fwd_f64_L11_256MiB_exact") == "double, 11, 16, true, false>"
    assert sym("bwd_f32_L10_256MiB_exact") == "float, 10, 4, false, false, 0>"        # <= 256 MiB: quarter tiles
    assert sym("bwd_f32_L10_256MiB_above") == "float, 10, 16, true, true, 0>"         # > 256 MiB: NT
    assert sym("bwd_f32_L10_256MiB_exact_big") == "float, 10, 16, false, false, 0>"   # BIG_TILES at 256 MiB: still cached
    assert sym("bwd_f32_L10_256MiB_above_big") == "float, 10, 16, true, true, 0>"
    assert sym("bwd_f64_L9_256MiB_exact") == "double, 9, 4, false, false, 0>" and sym("bwd_f64_L9_256MiB_above") == "double, 9, 16, true, true, 0>"
    assert _bytes(by_id["bwd_f32_L10_128MiB_exact_big"]) == 128 * MIB and _bytes(by_id["bwd_f32_L10_128MiB_above_big"]) == 128 * MIB + 16384
    assert sym("bwd_f32_L10_128MiB_exact_big") == "float, 10, 16, false, true, 2>"    # <= 128 MiB: the LDS network
    assert sym("bwd_f32_L10_128MiB_above_big") == "float, 10, 16, false, false, 0>"
    assert len([c for c in wt.CASES if c["kind"] == "boundary"]) == 20


def test_mirror_on_known_launches():
    """Launches whose symbol other tests of the suite state (tests/test_config_parity.py, tests/test_streaming_parity_gpu.py)."""
    assert wt.wbar_bwd("float", 11, 1, 33, 2048, wt.WBAR_MEAN).symbol == "whvi::wbar_bwd_kernel<float, 11, 16, true, true, 0>"
    assert wt.wbar_bwd("float", 11, 1, 2, 2048, 0).symbol == "whvi::wbar_bwd_kernel<float, 11, 8, false, false, 0>"
    assert wt.wbar_bwd("double", 12, 1, 3, 4096, 0).symbol == "whvi::wbar_bwd_kernel<double, 12, 32, true, false, 0>"
    assert wt.wbar_fwd("double", 12, 1, 2, 4096).symbol == "whvi::wbar_fwd_kernel<double, 12, 32, true>"
    assert wt.wbar_fwd("float", 11, 1, 17, 2048).symbol == "whvi::wbar_fwd_kernel<float, 11, 16, true>"
    # config 2's layer: 32 samples of D = 512 (32 MiB) -- quarter tiles, cached, and the one-launch mean form
    assert wt.wbar_fwd("float", 9, 1, 32, 512).shipped == "whvi::wbar_fwd_kernel<float, 9, 4, false, false>"
    assert wt.wbar_fwd("float", 9, 1, 32, 512, inline_mean=True).symbol == "whvi::wbar_fwd_kernel<float, 9, 4, false, true>"
    # the XCD-sliced order: 1 GiB of D = 2048 matrices with a mean matrix -- 16 MiB per matrix = 32 groups
    la = wt.wbar_fwd("float", 11, 1, 64, 2048, base=True)
    assert (la.nt, la.xcd_blocks, la.reorder, la.grid) == (True, 32, False, 16384)
    assert wt.wbar_fwd("float", 11, 1, 64, 2048).reorder and wt.wbar_fwd("float", 11, 1, 64, 2047, base=True).xcd_blocks == 0
    for bad in (lambda: wt.wbar_fwd("float", 13, 1, 1, 8, inline_mean=True), lambda: wt.wbar_fwd("double", 13, 1, 1, 8),
                lambda: wt.wbar_bwd("float", 1, 1, 1, 2), lambda: wt.wbar_bwd("float", 4, 1, 1, 17), lambda: wt.wbar_bwd("float", 4, 1, 1, 16, 16)):
        with pytest.raises(ValueError):
            bad()
    assert [wt.small_k("float", L) for L in range(2, 14)] == [4] * 9 + [8, 16, 32]
    assert [wt.small_k("double", L) for L in range(1, 13)] == [4] * 9 + [8, 16, 32]
    assert [wt.lds_ok("float", L) for L in range(2, 14)] == [False] * 6 + [True] * 5 + [False] and not any(wt.lds_ok("double", L) for L in range(1, 13))


def test_every_switch_both_ways_for_every_entry_and_type():
    for T in ("float", "double"):
        fwd = [c for c in wt.CASES if c["entry"] == "wbar_fwd" and c["dtype"] == T]
        for what, f in (("base", lambda c: c["base"]), ("first", lambda c: c["first"] > 0), ("spare", lambda c: c["spare"] > 0),
                        ("R == D", lambda c: c["R"] == 1 << c["log2d"]), ("nt", lambda c: wt.launch(c).nt)):
            assert {bool(f(c)) for c in fwd} == {True, False}, (T, what)
        stream = [c for c in fwd if wt.launch(c).nt]
        assert {wt.launch(c).reorder for c in stream if not wt.launch(c).xcd_blocks} == {True, False}, T
        assert {wt.launch(c).xcd_blocks > 0 for c in stream} == {True, False}
        assert {c["base"] for c in stream if not wt.launch(c).xcd_blocks} == {True, False}       # base given, the condition failing
        # every streaming instantiation with a D large enough: one case on each side of the slicing condition
        for L in wt.log2ds(T):
            mine = [c for c in stream if c["log2d"] == L and c["kind"] == "inst"]
            big_enough = (1 << L) ** 2 * wt.SIZE[T] >= 1024 * wt.pick_k(T, L) * 32
            assert sorted(wt.launch(c).xcd_blocks > 0 for c in mine) == ([False, True] if big_enough else [False]), (T, L)
        assert {c["first"] for c in fwd} == {0, 1, 2}
        mean = [c for c in wt.CASES if c["entry"] == "wbar_fwd_mean" and c["dtype"] == T]
        bwd = [c for c in wt.CASES if c["entry"] == "wbar_bwd" and c["dtype"] == T]
        for what, f in (("mean", lambda c: c["mean"]), ("no_lds", lambda c: c["no_lds"]), ("R == D", lambda c: c["R"] == 1 << c["log2d"]),
                        ("nt", lambda c: wt.launch(c).nt), ("small", lambda c: wt.launch(c).k < wt.pick_k(T, c["log2d"]))):
            assert {bool(f(c)) for c in bwd} == {True, False}, (T, what)
        assert {c["tiles"] for c in bwd} == {None, "small", "big"}
        assert {wt.launch(c).reorder for c in bwd if wt.launch(c).nt} == {True, False}, T
        assert {wt.launch(c).policy for c in bwd} == ({"lds", "dpp"} if T == "float" else {"dpp"})
        # the big cached tiles through tiles="big", with and without no_lds
        assert {c["no_lds"] for c in bwd if c["tiles"] == "big" and not wt.launch(c).nt} == {True, False}
        for entry, mine in (("wbar_fwd", fwd), ("wbar_fwd_mean", mean), ("wbar_bwd", bwd)):
            # R < D at every D of every entry, with a row above D / 2 so that every bit of the row index is set somewhere
            for L in wt.log2ds(T, entry):
                assert any((1 << L) // 2 < c["R"] < 1 << L or (L == 1 and c["R"] == 1) for c in mine if c["log2d"] == L), (entry, T, L)
                assert any(c["R"] == 1 << L for c in mine if c["log2d"] == L) or entry != "wbar_fwd_mean", (entry, T, L)
            for nt in ({False} if entry == "wbar_fwd_mean" else {False, True}):
                pool = [c for c in mine if wt.launch(c).nt == nt]
                assert any(wt.ragged(c) for c in pool), (entry, T, nt, "no case with a last tile that is not full")
                assert any(wt.tiles(c) % 4 for c in pool), (entry, T, nt, "no case whose tile count is no multiple of 4")
                assert any(c["J"] > 1 and c["S"] > 1 for c in pool), (entry, T, nt)


def test_nonfinite_selection():
    picked = wt.nonfinite_cases()
    keys = {(c["entry"], c["dtype"], wt.network(c), wt.launch(c).nt) for c in picked}
    want = {(e, T, "fwd", nt) for e in ("wbar_fwd",) for T in wt.SIZE for nt in (False, True)}
    want |= {("wbar_fwd_mean", T, "fwd", False) for T in wt.SIZE}
    want |= {("wbar_bwd", T, "dpp", nt) for T in wt.SIZE for nt in (False, True)} | {("wbar_bwd", "float", "lds", False)}
    assert keys == want and len(picked) == len(want)


def test_argument_checks_answer_before_any_device_call():
    """What tests/test_abi.py::test_argument_checks_of_the_training_step_entry_points leaves out: negative sizes, log2(D) above the
    range (and below it for float64 and the backward), the one-launch mean form's limit, u_first / u_group, the 32-bit row
    index, each null operand, a misaligned base / grad_w, R > D in the backward, and the empty launches of the mean form."""
    from whvi_amd import _hip
    L = _hip.lib()
    buf = (ctypes.c_char * 512)()
    p = (ctypes.addressof(buf) + 15) & ~15
    ARG, SIZE, ALIGN = -1, -2, -3
    err = _hip.last_error
    for fwd, lo, hi in ((L.whvi_wbar_fwd_f32, 2, 13), (L.whvi_wbar_fwd_f64, 1, 12)):
        for J, S, R in ((-1, 1, 1), (1, -1, 1), (1, 1, -1)):
            assert fwd(p, p, p, p, None, J, S, R, 4, max(S, 1), 0, None) == ARG and "negative" in err()
        assert fwd(p, p, p, p, None, 1, 1, 1, hi + 1, 1, 0, None) == SIZE and "supported range" in err()
        assert fwd(p, p, p, p, None, 1, 1, 1, lo - 1, 1, 0, None) == SIZE
        assert fwd(p, p, p, p, None, 1, 1, 2, 4, 1, -1, None) == ARG and "u_group" in err()
        assert fwd(p, p, p, p, None, 1, 1, 2, 4, 1 << 31, 0, None) == ARG and "u_group" in err()
        assert fwd(p, p, p, p, None, 1, 3, 2, 4, 3, 1, None) == ARG                       # rows 1 .. 3 of a group of 3
        assert fwd(p, p, p, p, None, 1 << 16, 1 << 12, 16, 4, 1 << 12, 0, None) == SIZE and "32 bits" in err()
        for hole in range(1, 4):
            a = [p, p, p, p]
            a[hole] = None
            assert fwd(*a, None, 1, 1, 2, 4, 1, 0, None) == ARG and "null" in err()
        assert fwd(p, p, p, p, p + 8, 1, 1, 2, 4, 1, 0, None) == ALIGN and "base" in err()
        assert fwd(None, None, None, None, None, 3, 0, 4, 4, 0, 0, None) == 0 and fwd(None, None, None, None, None, 3, 2, 0, 4, 2, 0, None) == 0
    for mean, lo, low in ((L.whvi_wbar_fwd_mean_f32, 2, 12), (L.whvi_wbar_fwd_mean_f64, 1, 11)):
        assert mean(p, p, p, p, 1, 1, 2, low + 1, None) == SIZE and "one-launch form" in err()
        assert mean(p, p, p, p, 1, 1, 2, low + 2, None) == SIZE and "supported range" in err()
        assert mean(p, p, p, p, 1, 1, 2, lo - 1, None) == SIZE
        assert mean(p, p, p, p, 1, -1, 2, 4, None) == ARG and mean(p, p, p, p, 1, 1, 17, 4, None) == ARG and "exceeds D" in err()
        assert mean(None, p, p, p, 1, 1, 2, 4, None) == ARG and mean(p, p, None, p, 1, 1, 2, 4, None) == ARG
        assert mean(p + 4, p, p, p, 1, 1, 2, 4, None) == ALIGN
        assert mean(None, None, None, None, 0, 3, 4, 4, None) == 0 and mean(None, None, None, None, 2, 0, 4, 4, None) == 0
    for bwd, lo, hi in ((L.whvi_wbar_bwd_f32, 2, 13), (L.whvi_wbar_bwd_f64, 1, 12)):
        for J, S, R in ((-1, 1, 1), (1, -1, 1), (1, 1, -1)):
            assert bwd(p, p, p, p, p, p, p, J, S, R, 4, 0, None) == ARG and "negative" in err()
        assert bwd(p, p, p, p, p, p, p, 1, 1, 1, lo - 1, 0, None) == SIZE and bwd(p, p, p, p, p, p, p, 1, 1, 1, hi + 1, 0, None) == SIZE
        assert bwd(p, p, p, p, p, p, p, 1, 1, 17, 4, 0, None) == ARG and "exceeds D" in err()
        assert bwd(p, p, p, p, p, p, p, 1 << 16, 1 << 12, 16, 4, 0, None) == SIZE and "32 bits" in err()
        assert bwd(p, p, p, p, p, p, p, 1, 1, 2, 4, -1, None) == ARG and "flags" in err()
        for hole in range(7):
            a = [p] * 7
            a[hole] = None
            assert bwd(*a, 1, 1, 2, 4, 0, None) == ARG and "null" in err(), hole
        assert bwd(p, p, p, p + 8, p, p, p, 1, 1, 2, 4, 0, None) == ALIGN and "grad_w" in err()
        for flags in range(16):                                           # every flag word: an empty launch is no error
            assert bwd(None, None, None, None, None, None, None, 0, 2, 4, 4, flags, None) == 0
    assert wt.bwd_flags(True, True, "small") == 7 and wt.bwd_flags(False, False, "big") == 8
    assert (_hip.lib().whvi_hip_abi_version(), wt.WBAR_MEAN, wt.WBAR_NO_LDS, wt.WBAR_SMALL_TILES, wt.WBAR_BIG_TILES) == (1, 1, 2, 4, 8)
