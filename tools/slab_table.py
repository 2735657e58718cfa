#!/usr/bin/env python3
"""tools/slab_table.py -- the slab-walking kernels (the block geometry fused_bwd_geom of whvi_amd/csrc/fused_bwd.hpp): which
instantiation each launch runs, how many tiles each wave walks, and a case list that takes every shipped instantiation past
one tile per wave -- once cached, once streaming.

Six kernel templates share the geometry: a block of four waves owns (sample, a slab of that sample's rows) and each wave walks
its slab one tile at a time, ``for (rt = r_begin + wave * RPT; rt < r_end; rt += 4 * RPT)``; the backward kernels carry their
grad_a / grad_b / grad_c sums from tile to tile, and a finishing kernel adds the blocks' partial sums.  The mirrors below
restate, in Python, the geometry (fused_bwd_k, fused_bwd_tile_rows, fused_bwd_geom) and, per entry point, the streamed-byte
rule that picks the non-temporal (NT) instantiation.  ``launch(case)`` returns the demangled symbol ``whvi_last_kernel``
reports, every symbol the call launches (finishing kernel included), the grid, ``nt`` and ``tiles_per_wave``.

``CASES`` holds two cases per shipped (template arguments without NT):
    walk   : cached (NT = false), at least three tiles per wave, S = 3 samples, the last slab of every sample shorter than the
             others and -- where a tile has several rows -- ending inside a tile;
    stream : S = 3 and the smallest batch that crosses the entry's 256 MiB rule (NT = true), raised to the next batch with such
             a ragged last slab.
These are the smallest shapes that reach each regime, not the timed workloads.  The options (shared / own x, need_x, and for
the layer kernels bias, relu_in, relu_out, a narrowed n_cols and a pitch wider than n_cols) are spread over the cases by index.
tests/test_slab_table_host.py checks the list against the built library and the mirror against the workspace queries;
tests/test_slab_table_gpu.py runs every case against float64.  Pure Python: no torch, no GPU.

    python tools/slab_table.py        # every case with its symbol, grid, tiles per wave and streamed MiB"""
import itertools
import os
import sys
from collections import namedtuple

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
from kernel_table import NT_MIN_BYTES, family  # noqa: E402,F401

MIN_LOG2D, MAX_LOG2D = 6, 12                   # fused_bwd.hpp: FUSED_BWD_MIN_LOG2D / FUSED_BWD_MAX_LOG2D
STACKED_MAX_LOG2D = 11                         # fused_stacked_fwd.hpp: FUSED_STACKED_MAX_LOG2D
LDS_BYTES = 65536                              # fused_stacked_fwd.hpp: FUSED_STACKED_LDS_BYTES
SAMPLES = 3                                    # every case: an odd sample count, so the slab count does not divide evenly

KERNEL_FAMILIES = ("fused_shs_bwd_kernel", "fused_shs_stacked_kernel", "fused_stacked16_kernel", "fused_shs_stacked_bwd_kernel",
                   "fused_shs_stacked_layer_kernel", "fused_shs_stacked_layer_bwd_kernel")
FINISH_FAMILIES = ("fused_shs_bwd_finish_kernel", "fused_shs_stacked_bwd_finish_kernel",
                   "fused_shs_stacked_layer_bwd_finish_kernel")
FAMILIES = KERNEL_FAMILIES + FINISH_FAMILIES
ENTRIES = ("fused_shs_bwd", "fused_shs_stacked", "fused_shs_stacked16", "fused_shs_stacked_bwd", "fused_shs_stacked_layer",
           "fused_shs_stacked_layer_bwd")
ACT_BYTES = {"float": 4, "__half": 2, "__hip_bfloat16": 2}

# the suite's value-checking shapes (S, B) before this case list: every one of them gives one tile per wave at every D
EXISTING_SHAPES = ((1, 1), (3, 5), (2, 777), (4, 64), (3, 65), (3, 37), (3, 7), (2, 9), (2, 64))

Launch = namedtuple("Launch", "symbol symbols grid nt tiles_per_wave")


def _b(v):
    return "true" if v else "false"


def _cdiv(a, b):
    return -(-a // b)


# ---- the geometry (fused_bwd.hpp)
def fused_bwd_k(log2d, vec=4):
    """Chunks of 16 bytes per lane of one wave tile: one row from D = 1024 up, 1024 elements below; vec elements per chunk."""
    return ((1 << (log2d - 8)) if log2d >= 10 else 4) * 4 // vec


def fused_bwd_tile_rows(log2d):
    return (fused_bwd_k(log2d) * 256) >> log2d


def fused_bwd_target(log2d):
    """Blocks one call aims at."""
    return 512 if log2d >= 12 else 1024


def fused_bwd_geom(S, B, log2d):
    """(n_slabs, slab_rows) of one call: a function of the arguments alone."""
    rpt = fused_bwd_tile_rows(log2d)
    n = _cdiv(fused_bwd_target(log2d), S)
    n = max(min(n, _cdiv(B, 4 * rpt)), 1)
    slab = _cdiv(_cdiv(B, n), rpt) * rpt
    return _cdiv(B, slab), slab


def tiles_per_wave(S, B, log2d):
    """Tiles the busiest wave of a block walks: ceil(slab_rows / (4 rpt))."""
    return _cdiv(fused_bwd_geom(S, B, log2d)[1], 4 * fused_bwd_tile_rows(log2d))


def last_slab_rows(S, B, log2d):
    n_slabs, slab = fused_bwd_geom(S, B, log2d)
    return B - (n_slabs - 1) * slab


def ragged(S, B, log2d):
    """The last slab of each sample is shorter than the others and, where a tile has several rows, ends inside a tile."""
    rpt = fused_bwd_tile_rows(log2d)
    n_slabs, slab = fused_bwd_geom(S, B, log2d)
    last = last_slab_rows(S, B, log2d)
    return n_slabs > 1 and last < slab and (rpt == 1 or last % rpt != 0)


def one_tile_rows(log2d):
    """The most rows of one sample (S = 1) that still give every wave at most one tile."""
    return fused_bwd_target(log2d) * 4 * fused_bwd_tile_rows(log2d)


# ---- the streamed bytes per row that set nt, per entry point, as the sources have them
def row_bytes(case):
    """Streamed bytes per (sample, row) of the entry's rule: nt = rows * row_bytes > NT_MIN_BYTES."""
    e, D = case["entry"], 1 << case["log2d"]
    own, need_x = (0 if case["shared"] else 1), (1 if case.get("need_x") else 0)
    if e == "fused_shs_bwd":                    # fused_bwd_f32.hip: grad_y, x unless shared, grad_x unless skipped
        return D * ACT_BYTES[case["dtype"]] * (1 + own + need_x)
    if e in ("fused_shs_stacked", "fused_shs_stacked16"):          # the J output segments, the source unless shared
        return D * ACT_BYTES[case["dtype"]] * (case["J"] + own)
    if e == "fused_shs_stacked_bwd":            # the J segments of grad_y, x unless shared, grad_x unless skipped
        return D * 4 * (case["J"] + own + need_x)
    if e == "fused_shs_stacked_layer":          # the n_cols written columns, the source unless shared
        return 4 * case["n_cols"] + (D * 4 if own else 0)
    if e == "fused_shs_stacked_layer_bwd":      # the n_cols columns of grad_y (and of y), x unless shared, grad_x unless skipped
        return 4 * (case["n_cols"] * (2 if case["relu_out"] else 1) + D * own + D * need_x)
    raise ValueError(e)


def streamed_bytes(case):
    return case["S"] * case["B"] * row_bytes(case)


def supported(entry, log2d, J=1, bias=False):
    if entry == "fused_shs_bwd":
        return MIN_LOG2D <= log2d <= MAX_LOG2D
    if entry in ("fused_shs_stacked", "fused_shs_stacked16"):
        return MIN_LOG2D <= log2d <= STACKED_MAX_LOG2D and 1 <= J <= LDS_BYTES // (12 << log2d)
    if entry == "fused_shs_stacked_layer":
        return MIN_LOG2D <= log2d <= STACKED_MAX_LOG2D and 1 <= J <= LDS_BYTES // ((16 if bias else 12) << log2d)
    if entry in ("fused_shs_stacked_bwd", "fused_shs_stacked_layer_bwd"):
        return (MIN_LOG2D <= log2d <= 10 and 2 <= J <= 4) or (log2d == 11 and J == 2)
    raise ValueError(entry)


def launch(case):
    """The mirror's answer for one case."""
    e, L, S, B = case["entry"], case["log2d"], case["S"], case["B"]
    T = case["dtype"]
    if not supported(e, L, case.get("J", 1), bool(case.get("bias"))):
        raise ValueError(f"{e}: log2(D) = {L}, J = {case.get('J')}")
    k = fused_bwd_k(L, 16 // ACT_BYTES[T])
    nt = streamed_bytes(case) > NT_MIN_BYTES
    n_slabs, _ = fused_bwd_geom(S, B, L)
    finish = ()
    if e == "fused_shs_bwd":
        sym, finish = f"whvi::fused_shs_bwd_kernel<{T}, {L}, {k}, {_b(nt)}>", ("whvi::fused_shs_bwd_finish_kernel",)
    elif e == "fused_shs_stacked":
        sym = f"whvi::fused_shs_stacked_kernel<{T}, {L}, {k}, {_b(nt)}>"
    elif e == "fused_shs_stacked16":
        sym = f"whvi::fused_stacked16_kernel<{T}, {L}, {k}, {_b(nt)}>"
    elif e == "fused_shs_stacked_bwd":
        sym = f"whvi::fused_shs_stacked_bwd_kernel<{T}, {L}, {k}, {case['J']}, {_b(nt)}>"
        finish = ("whvi::fused_shs_stacked_bwd_finish_kernel",)
    elif e == "fused_shs_stacked_layer":
        sym = f"whvi::fused_shs_stacked_layer_kernel<{T}, {L}, {k}, {_b(nt)}>"
    else:
        sym = f"whvi::fused_shs_stacked_layer_bwd_kernel<{T}, {L}, {k}, {case['J']}, {_b(case['bias'])}, {_b(nt)}>"
        finish = ("whvi::fused_shs_stacked_layer_bwd_finish_kernel",)
    return Launch(sym, (sym,) + finish, S * n_slabs, nt, tiles_per_wave(S, B, L))


# ---- the case list
def sized(case, regime):
    """The case at the batch size of its regime.  walk: the largest cached batch up to 4106 tiles' rows (less 15 rows where a
    tile has several) with at least three tiles per wave and a ragged last slab -- 4106 rows for D >= 1024 (316 slabs of 13 rows
    and one of 11), 65 681 for D = 64 (slabs of 208 rows, the last 161), fewer where that would stream.  stream: the smallest
    batch whose streamed bytes cross NT_MIN_BYTES, raised to the next ragged one with at least two tiles per wave."""
    c = dict(case, regime=regime, S=SAMPLES)
    L, per_row = c["log2d"], row_bytes(case)
    rpt = fused_bwd_tile_rows(L)
    if regime == "walk":
        top = min(4106 * rpt - (15 if rpt > 1 else 0), NT_MIN_BYTES // (SAMPLES * per_row))
        for B in range(top, 0, -1):
            if tiles_per_wave(SAMPLES, B, L) >= 3 and ragged(SAMPLES, B, L):
                c["B"] = B
                return c
        raise AssertionError(f"{case['id']}: no cached batch walks three tiles per wave")
    first = NT_MIN_BYTES // (SAMPLES * per_row) + 1
    for B in range(first, first + 1000):
        if tiles_per_wave(SAMPLES, B, L) >= 2 and ragged(SAMPLES, B, L):
            c["B"] = B
            return c
    raise AssertionError(f"{case['id']}: no ragged batch within 1000 rows of the streaming threshold")


def _spread(i):
    """Options spread over the cases by index: (shared, need_x, bias, relu_in, relu_out, narrowed n_cols, wider ld, poison)."""
    return i % 2 == 0, i % 3 != 0, i % 3 != 0, i % 4 == 1, i % 4 >= 2, i % 2 == 1, i % 3 == 1, i % 5 == 0


def _layer_cols(log2d, J, narrowed, wider):
    """n_cols ends inside the last block and is a multiple of 4; the pitch is n_cols or eight floats more."""
    D = 1 << log2d
    n_cols = (J - 1) * D + D // 2 + 4 if narrowed else J * D
    return n_cols, n_cols + (8 if wider else 0)


def _both(out, base, i):
    """The walk and the stream case of one instantiation; the stream case takes the next index's options, so the two regimes of
    an instantiation differ in them and, over a family, each regime meets each option."""
    for regime, k in (("walk", i), ("stream", i + 1)):
        shared, need_x, bias, relu_in, relu_out, narrowed, wider, poison = _spread(k)
        c = dict(base, shared=shared, poison=poison)
        e = c["entry"]
        if e.endswith("_bwd"):
            c["need_x"] = need_x
        if e == "fused_shs_stacked_layer":
            # the bias is staged with the triples: without one where J quadruples would not fit the LDS
            c["bias"] = bias and supported(e, c["log2d"], c["J"], True)
        if e.startswith("fused_shs_stacked_layer"):
            c.update(relu_in=relu_in, relu_out=relu_out)
            c["n_cols"], c["ld"] = _layer_cols(c["log2d"], c["J"], narrowed, wider)
        c["id"] = f"{c['id']}_{regime}"
        out.append(_fitted(c, regime))


# Three tiles per wave on ~1024 blocks are at least 8209 tiles' rows: 32 MiB per D-wide tensor (D <= 2048).  A launch that
# streams eight D-widths per row or more (J = 4 with relu_out's y, say) cannot walk that far and stay cached, so a walk case
# gives up the fewest of its byte-adding options, tried in this order, that let it fit.
_RELAX = (("need_x", False), ("shared", True), ("relu_out", False))


def _fitted(c, regime):
    have = [(k, v) for k, v in _RELAX if k in c and c[k] != v]
    for n in range(len(have) + 1):
        for drop in itertools.combinations(have, n):
            try:
                return sized(dict(c, **dict(drop)), regime)
            except AssertionError:
                if regime != "walk":
                    raise
    raise AssertionError(f"{c['id']}: no option set fits the {regime} regime")


def _build_cases():
    out = []
    names = {"float": "f32", "__half": "f16", "__hip_bfloat16": "bf16"}
    i = 0
    for T in ("float", "__half", "__hip_bfloat16"):
        for L in range(MIN_LOG2D, MAX_LOG2D + 1):
            _both(out, dict(id=f"bwd_{names[T]}_L{L}", entry="fused_shs_bwd", dtype=T, log2d=L), i)
            i += 1
    # the forward kernels take J as an argument: the block counts rotate over what the LDS holds
    for i, L in enumerate(range(MIN_LOG2D, STACKED_MAX_LOG2D + 1)):
        J = 1 + i % min(4, LDS_BYTES // (12 << L))
        _both(out, dict(id=f"stacked_L{L}_J{J}", entry="fused_shs_stacked", dtype="float", log2d=L, J=J), i)
    i = 0
    for T in ("__half", "__hip_bfloat16"):
        for L in range(MIN_LOG2D, STACKED_MAX_LOG2D + 1):
            J = 1 + (i + 1) % min(4, LDS_BYTES // (12 << L))
            _both(out, dict(id=f"stacked16_{names[T]}_L{L}_J{J}", entry="fused_shs_stacked16", dtype=T, log2d=L, J=J), i)
            i += 1
    shipped_lj = [(L, J) for L in range(MIN_LOG2D, 11) for J in (2, 3, 4)] + [(11, 2)]
    for i, (L, J) in enumerate(shipped_lj):
        _both(out, dict(id=f"stacked_bwd_L{L}_J{J}", entry="fused_shs_stacked_bwd", dtype="float", log2d=L, J=J), i)
    for i, L in enumerate(range(MIN_LOG2D, STACKED_MAX_LOG2D + 1)):
        J = 1 + (i + 2) % min(4, LDS_BYTES // (16 << L))
        _both(out, dict(id=f"layer_L{L}_J{J}", entry="fused_shs_stacked_layer", dtype="float", log2d=L, J=J), i)
    i = 0
    for L, J in shipped_lj:
        for bias in (False, True):
            _both(out, dict(id=f"layer_bwd_L{L}_J{J}{'_bias' if bias else ''}", entry="fused_shs_stacked_layer_bwd", dtype="float",
                            log2d=L, J=J, bias=bias), i)
            i += 1
    return out


CASES = _build_cases()


def reached():
    """family -> the set of symbols the case list launches."""
    out = {f: set() for f in FAMILIES}
    for case in CASES:
        for sym in launch(case).symbols:
            out[family(sym)].add(sym)
    return out


def main():
    for c in CASES:
        la = launch(c)
        print(f"{c['id']:36s} {la.symbol:72s} S {c['S']} B {c['B']:7d} grid {la.grid:5d} tiles/wave {la.tiles_per_wave:2d} "
              f"last slab {last_slab_rows(c['S'], c['B'], c['log2d']):4d} {'nt' if la.nt else '  '} "
              f"{streamed_bytes(c) / 2 ** 20:7.1f} MiB")
    print(f"{len(CASES)} cases; " + ", ".join(f"{f}: {len(s)}" for f, s in reached().items()))


if __name__ == "__main__":
    main()
