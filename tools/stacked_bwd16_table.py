#!/usr/bin/env python3
"""tools/stacked_bwd16_table.py -- the one-launch backward of the rectangular fastfood layer on 16-bit activations
(whvi_fused_shs_stacked_bwd_f16 / _bf16, whvi_amd/csrc/fused_stacked_bwd16.hpp): which instantiation of
``fused_stacked_bwd16_kernel`` each launch runs, and a case list that takes every shipped one past one tile per wave -- once
cached, once streaming.  The geometry is tools/slab_table.py's (fused_bwd_geom, tiles_per_wave, ragged, one_tile_rows); this file
adds the entry's support rule, its streamed-byte rule and its cases, so slab_table's pinned list stays as it is.

``CASES`` holds two cases per shipped (dtype, log2 D, J):
    walk   : cached (NT = false), at least three tiles per wave, S = 3 samples, the last slab of every sample shorter than the
             others and -- where a tile has several rows -- ending inside a tile;
    stream : S = 3 and the smallest batch that crosses the 256 MiB rule (NT = true) with at least two tiles per wave and such a
             ragged last slab: less than 1.5 times the threshold.
``shared``, ``need_x`` and ``poison`` are spread over the cases by index, the stream case of an instantiation taking the next
index's, so that each takes both values in both regimes.  tests/test_fastfood_stacked_bwd16_host.py checks the list against the
built library; tests/test_fastfood_stacked_bwd16_gpu.py runs every case against float64.  Pure Python: no torch, no GPU.

    python tools/stacked_bwd16_table.py        # every case with its symbol, grid, tiles per wave and streamed MiB"""
import os
import sys

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
from slab_table import (NT_MIN_BYTES, Launch, fused_bwd_geom, fused_bwd_k, fused_bwd_tile_rows, last_slab_rows,  # noqa: E402
                        one_tile_rows, ragged, tiles_per_wave)

ENTRY = "fused_shs_stacked_bwd16"
KERNEL = "fused_stacked_bwd16_kernel"
FINISH = "fused_stacked_bwd16_finish_kernel"
DTYPES = ("__half", "__hip_bfloat16")
SUFFIX = {"__half": "f16", "__hip_bfloat16": "bf16"}
SAMPLES = 3
SHIPPED_LJ = [(L, J) for L in range(6, 11) for J in (2, 3, 4)] + [(11, 2)]


def supported(log2d, J):
    """whvi_fused_shs_stacked_bwd16_supported: the float32 launch's rule."""
    return (6 <= log2d <= 10 and 2 <= J <= 4) or (log2d == 11 and J == 2)


def row_bytes(case):
    """Streamed bytes per (sample, row): the J segments of grad_y, x unless shared, grad_x unless skipped, 2 bytes an element."""
    return (2 << case["log2d"]) * (case["J"] + (0 if case["shared"] else 1) + (1 if case["need_x"] else 0))


def streamed_bytes(case):
    return case["S"] * case["B"] * row_bytes(case)


def launch(case):
    """The mirror's answer for one case: the symbol whvi_last_kernel names, every symbol the call launches, the grid, nt and
    the tiles the busiest wave walks."""
    L, J, S, B = case["log2d"], case["J"], case["S"], case["B"]
    if not supported(L, J):
        raise ValueError(f"{ENTRY}: log2(D) = {L}, J = {J}")
    nt = streamed_bytes(case) > NT_MIN_BYTES
    sym = f"whvi::{KERNEL}<{case['dtype']}, {L}, {fused_bwd_k(L, 8)}, {J}, {'true' if nt else 'false'}>"
    return Launch(sym, (sym, "whvi::" + FINISH), S * fused_bwd_geom(S, B, L)[0], nt, tiles_per_wave(S, B, L))


def sized(case, regime):
    """The case at the batch size of its regime (slab_table.sized's rule).  walk: the largest cached batch up to 4106 tiles'
    rows (less 15 rows where a tile has several) with at least three tiles per wave and a ragged last slab.  stream: the
    smallest batch whose streamed bytes cross NT_MIN_BYTES, raised to the next ragged one with at least two tiles per wave."""
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
    """(shared, need_x, poison) by index."""
    return i % 2 == 0, i % 3 != 0, i % 5 == 0


def _build_cases():
    out, i = [], 0
    for T in DTYPES:
        for L, J in SHIPPED_LJ:
            for regime, k in (("walk", i), ("stream", i + 1)):
                shared, need_x, poison = _spread(k)
                out.append(sized(dict(id=f"stacked_bwd16_{SUFFIX[T]}_L{L}_J{J}_{regime}", entry=ENTRY, dtype=T, log2d=L, J=J,
                                      shared=shared, need_x=need_x, poison=poison), regime))
            i += 1
    return out


CASES = _build_cases()


def reached():
    """The set of symbols the case list launches."""
    return {sym for case in CASES for sym in launch(case).symbols}


def main():
    for c in CASES:
        la = launch(c)
        print(f"{c['id']:36s} {la.symbol:66s} S {c['S']} B {c['B']:7d} grid {la.grid:5d} tiles/wave {la.tiles_per_wave:2d} "
              f"last slab {last_slab_rows(c['S'], c['B'], c['log2d']):4d} {'nt' if la.nt else '  '} "
              f"{streamed_bytes(c) / 2 ** 20:7.1f} MiB  one tile: {one_tile_rows(c['log2d'])} rows"
              f"{' shared' if c['shared'] else ''}{' need_x' if c['need_x'] else ''}{' poison' if c['poison'] else ''}")
    print(f"{len(CASES)} cases reach {len(reached())} symbols")


if __name__ == "__main__":
    main()
