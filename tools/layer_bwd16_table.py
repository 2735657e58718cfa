#!/usr/bin/env python3
"""tools/layer_bwd16_table.py -- the one-launch backward of the rectangular fastfood layer with its epilogue on 16-bit
activations (whvi_fused_shs_stacked_layer_bwd_f16 / _bf16, whvi_amd/csrc/fused_stacked_layer_bwd16.hpp): which instantiation of
``fused_layer_bwd16_kernel`` each launch runs, and a case list that takes every shipped one past one tile per wave -- once
cached, once streaming.  The geometry is tools/slab_table.py's (fused_bwd_geom, tiles_per_wave, ragged, one_tile_rows); this file
adds the entry's support rule, its streamed-byte rule and its cases, so slab_table's pinned list stays as it is.

``CASES`` holds two cases per shipped (dtype, log2 D, J, bias):
    walk   : cached (NT = false), at least three tiles per wave, S = 3 samples, the last slab of every sample shorter than the
             others and -- where a tile has several rows -- ending inside a tile;
    stream : S = 3 and the smallest batch that crosses the 256 MiB rule (NT = true) with at least two tiles per wave and such a
             ragged last slab: less than 1.5 times the threshold.
``shared``, ``need_x``, ``relu_in``, ``relu_out``, a narrowed ``n_cols``, a pitch wider than ``n_cols`` and ``poison`` are spread
over the cases by index, the stream case of an instantiation taking the next index's, so that each takes both values in both
regimes.  tests/test_fastfood_stacked_layer_bwd16_host.py checks the list against the built library;
tests/test_fastfood_stacked_layer_bwd16_gpu.py runs every case against float64 and against the composed route.  Pure Python: no
torch, no GPU.

    python tools/layer_bwd16_table.py        # every case with its symbol, grid, tiles per wave and streamed MiB"""
import itertools
import os
import sys

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
from slab_table import (NT_MIN_BYTES, Launch, fused_bwd_geom, fused_bwd_k, fused_bwd_tile_rows, last_slab_rows,  # noqa: E402
                        one_tile_rows, ragged, tiles_per_wave)

ENTRY = "fused_shs_stacked_layer_bwd16"
KERNEL = "fused_layer_bwd16_kernel"
FINISH = "fused_layer_bwd16_finish_kernel"
DTYPES = ("__half", "__hip_bfloat16")
SUFFIX = {"__half": "f16", "__hip_bfloat16": "bf16"}
SAMPLES = 3
SHIPPED_LJ = [(L, J) for L in range(6, 11) for J in (2, 3, 4)] + [(11, 2)]
OPTIONS = ("shared", "need_x", "relu_in", "relu_out", "narrowed", "wider", "poison")


def supported(log2d, J, bias=False):
    """whvi_fused_shs_stacked_layer_bwd16_supported: the 16-bit backward's rule, with and without a bias."""
    return (6 <= log2d <= 10 and 2 <= J <= 4) or (log2d == 11 and J == 2)


def _b(v):
    return "true" if v else "false"


def row_bytes(case):
    """Streamed bytes per (sample, row): the n_cols columns of grad_y (and of y), x unless shared, grad_x unless skipped, 2 bytes
    an element."""
    D = 1 << case["log2d"]
    return 2 * (case["n_cols"] * (2 if case["relu_out"] else 1) + (0 if case["shared"] else D) + (D if case["need_x"] else 0))


def streamed_bytes(case):
    return case["S"] * case["B"] * row_bytes(case)


def launch(case):
    """The mirror's answer for one case: the symbol whvi_last_kernel names, every symbol the call launches, the grid, nt and
    the tiles the busiest wave walks."""
    L, J, S, B = case["log2d"], case["J"], case["S"], case["B"]
    if not supported(L, J, case["bias"]):
        raise ValueError(f"{ENTRY}: log2(D) = {L}, J = {J}")
    nt = streamed_bytes(case) > NT_MIN_BYTES
    sym = f"whvi::{KERNEL}<{case['dtype']}, {L}, {fused_bwd_k(L, 8)}, {J}, {_b(case['bias'])}, {_b(nt)}>"
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


# a walk case that cannot walk three tiles per wave and stay cached gives up the fewest of its byte-adding options, tried in
# this order, that let it fit (slab_table._fitted's rule)
_RELAX = (("need_x", False), ("shared", True), ("relu_out", False))


def _fitted(c, regime):
    have = [(k, v) for k, v in _RELAX if c[k] != v]
    for n in range(len(have) + 1):
        for drop in itertools.combinations(have, n):
            try:
                return sized(dict(c, **dict(drop)), regime)
            except AssertionError:
                if regime != "walk":
                    raise
    raise AssertionError(f"{c['id']}: no option set fits the {regime} regime")


def _spread(i):
    """(shared, need_x, relu_in, relu_out, narrowed, wider, poison) by index."""
    return i % 2 == 0, i % 3 != 0, i % 4 == 1, i % 4 >= 2, (i // 2) % 2 == 1, i % 3 == 1, i % 5 == 0


def layer_cols(log2d, J, narrowed, wider):
    """n_cols ends inside the last block and is a multiple of 8; the pitch is n_cols or sixteen elements more."""
    D = 1 << log2d
    n_cols = (J - 1) * D + D // 2 + 8 if narrowed else J * D
    return n_cols, n_cols + (16 if wider else 0)


def _build_cases():
    out, i = [], 0
    for T in DTYPES:
        for L, J in SHIPPED_LJ:
            for bias in (False, True):
                for regime, k in (("walk", i), ("stream", i + 1)):
                    c = dict(zip(OPTIONS, _spread(k)))
                    c["n_cols"], c["ld"] = layer_cols(L, J, c["narrowed"], c["wider"])
                    c.update(id=f"layer_bwd16_{SUFFIX[T]}_L{L}_J{J}{'_bias' if bias else ''}_{regime}", entry=ENTRY, dtype=T,
                             log2d=L, J=J, bias=bias)
                    out.append(_fitted(c, regime))
                i += 1
    return out


CASES = _build_cases()


def reached():
    """The set of symbols the case list launches."""
    return {sym for case in CASES for sym in launch(case).symbols}


def main():
    for c in CASES:
        la = launch(c)
        print(f"{c['id']:40s} {la.symbol:72s} S {c['S']} B {c['B']:7d} grid {la.grid:5d} tiles/wave {la.tiles_per_wave:2d} "
              f"last slab {last_slab_rows(c['S'], c['B'], c['log2d']):4d} {'nt' if la.nt else '  '} "
              f"{streamed_bytes(c) / 2 ** 20:7.1f} MiB  n_cols {c['n_cols']} ld {c['ld']}  one tile: {one_tile_rows(c['log2d'])} rows "
              + " ".join(o for o in OPTIONS if c[o]))
    print(f"{len(CASES)} cases reach {len(reached())} symbols")


if __name__ == "__main__":
    main()
