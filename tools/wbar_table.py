#!/usr/bin/env python3
"""tools/wbar_table.py -- the weight-construction kernels (whvi_amd/csrc/wbar_fwd.hpp, wbar_bwd.hpp): which instantiation each
call of whvi_wbar_fwd / whvi_wbar_fwd_mean / whvi_wbar_bwd runs, and a case list that launches every instantiation a
public argument can reach.

The mirrors restate launch_wbar_fwd (the inline-mean branch and xcd_blocks_for included) and launch_wbar_bwd in Python:
pick_k, the quarter-size tile KS, the mean form's KM, the three byte rules with the comparison operators the sources have
(see ``THRESHOLDS``), LDS_OK, the flag word of whvi_wbar_bwd and the supported ranges.  ``launch(case)`` returns

    symbol      what whvi_last_kernel reports.  The forward's note names four template arguments (type, log2 D, K, NT); the
                shipped symbol has a fifth (INLINE_MEAN), so
    shipped     is the demangled name in the library -- the same text for the backward and the mean form;
    grid, nt, k and, for the forward, xcd_blocks (blocks per matrix / 8 when the XCD-sliced block bijection is on, else 0) and
    reorder     whether the plain XCD-contiguous reorder of a streaming grid (grid % 8 == 0) applies; for the backward
    policy      "lds" or "dpp", the butterfly network.

``CASES`` holds at least one smallest case per reachable instantiation; S, J, R and the switches rotate over the list by index
(they are not crossed).  A streaming case is the smallest row count that crosses its entry's rule with a last tile that is not
full, a tile count that is no multiple of 4 and a grid on the side of the reorder condition the rotation asks for (``_sized``).  Every streaming forward instantiation whose D is large enough gets a second case that is a whole number of 8 x 4-tile
groups per matrix with ``base``: the XCD-sliced order.  ``kind == "boundary"`` cases sit on the byte thresholds.
``UNREACHABLE`` lists the shipped instantiations no argument of the public entries can launch, with the reason.
tests/test_wbar_table_host.py checks the list against the built library; tests/test_wbar_table_gpu.py runs every case.
Pure Python: no torch, no GPU.

    python tools/wbar_table.py        # every case with its symbol, grid and MiB"""
import os
import sys
from collections import namedtuple

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
from kernel_table import NT_MIN_BYTES, pick_k  # noqa: E402

LDS_MAX_BYTES = 128 << 20                      # launch_wbar_bwd: use_lds = !no_lds && bytes <= 128 MiB
WBAR_MEAN, WBAR_NO_LDS, WBAR_SMALL_TILES, WBAR_BIG_TILES = 1, 2, 4, 8          # include/whvi_hip.h
POLICY_DPP, POLICY_LDS = 0, 2                  # fwht_tile.hpp
SIZE = {"float": 4, "double": 8}
NAMES = {"float": "f32", "double": "f64"}

# The byte rules as the sources have them (bytes = J S R D sizeof(T), the matrices' size):
THRESHOLDS = {
    "wbar_fwd, KS < K: quarter tiles, cached": "bytes <= 256 MiB",
    "wbar_fwd, KS < K: otherwise 16 KiB tiles, NT": "bytes >= 256 MiB (so: > 256 MiB -- the cached 16 KiB tile is never taken)",
    "wbar_fwd, KS == K: NT": "bytes >= 256 MiB",
    "wbar_bwd, KS < K: quarter tiles, cached": "SMALL_TILES, or no BIG_TILES and bytes <= 256 MiB",
    "wbar_bwd, 16 KiB tiles: NT": "bytes > 256 MiB",
    "wbar_bwd, 16 KiB tiles: LDS network": "LDS_OK and no NO_LDS and bytes <= 128 MiB",
}

Launch = namedtuple("Launch", "symbol shipped grid nt k xcd_blocks reorder policy", defaults=(0, False, None))


def _b(v):
    return "true" if v else "false"


def _cdiv(a, b):
    return -(-a // b)


def lv(dtype):
    return 2 if dtype == "float" else 1


def min_log2d(dtype):
    return lv(dtype)


def max_single_pass_log2d(dtype):              # dispatch.hpp
    return 13 if dtype == "float" else 12


def multi_pass_low_log2d(dtype):               # dispatch.hpp: 64-register tiles; the one-launch mean form's limit
    return 12 if dtype == "float" else 11


def log2ds(dtype, entry="wbar_fwd"):
    top = multi_pass_low_log2d(dtype) if entry == "wbar_fwd_mean" else max_single_pass_log2d(dtype)
    return range(min_log2d(dtype), top + 1)


def small_k(dtype, log2d):
    """KS: a quarter of the 16 KiB tile, never less than one row."""
    need = 1 << (log2d - lv(dtype) - 6) if log2d > lv(dtype) + 6 else 1
    return max(need, 4)


def mean_k(dtype, log2d):
    """KM of the one-launch mean form."""
    return min(small_k(dtype, log2d), pick_k(dtype, log2d))


def tile_vgprs(dtype, k):
    return k * (16 // SIZE[dtype]) * SIZE[dtype] // 4


def lds_ok(dtype, log2d):
    """LDS_OK: 32-bit arithmetic, a 64-register tile, rows of at least 64 chunks."""
    return dtype == "float" and pick_k(dtype, log2d) * 4 == 64 and log2d >= 8


def _geom(nbytes, k):
    tiles = _cdiv(nbytes // 16, 64 * k)
    return tiles, _cdiv(tiles, 4)


def nbytes(case):
    return case["J"] * case["S"] * case["R"] * (SIZE[case["dtype"]] << case["log2d"])


def ragged(case):
    """The last tile of the launch is not full."""
    return (nbytes(case) // 16) % (64 * launch(case).k) != 0


def tiles(case):
    return _geom(nbytes(case), launch(case).k)[0]


def wbar_fwd(dtype, log2d, J, S, R, base=False, inline_mean=False):
    """launch_wbar_fwd behind wbar_fwd_dispatch's checks."""
    D = 1 << log2d
    if not min_log2d(dtype) <= log2d <= max_single_pass_log2d(dtype):
        raise ValueError(f"whvi_wbar_fwd: log2(D) = {log2d} for {dtype}")
    if inline_mean and log2d > multi_pass_low_log2d(dtype):
        raise ValueError(f"whvi_wbar_fwd_mean: log2(D) = {log2d} for {dtype}")
    if min(J, S, R) <= 0 or R > D or J * S * R >= 1 << 32:
        raise ValueError("whvi_wbar_fwd: sizes")
    n_chunks = J * S * R * D * SIZE[dtype] // 16
    K, KS = pick_k(dtype, log2d), small_k(dtype, log2d)
    if inline_mean:
        km = mean_k(dtype, log2d)
        assert tile_vgprs(dtype, km) <= 64
        sym = f"whvi::wbar_fwd_kernel<{dtype}, {log2d}, {km}, false, true>"
        return Launch(sym, sym, _geom(n_chunks * 16, km)[1], False, km)

    def xcd_blocks_for(k, streaming):
        per_matrix, group = R * D * SIZE[dtype] // 16, 64 * k * 4 * 8
        if not streaming or not base or per_matrix % group or n_chunks % per_matrix:
            return 0
        return per_matrix // group

    if KS < K and n_chunks * 16 <= NT_MIN_BYTES:
        k, nt = KS, False
    else:
        k, nt = K, n_chunks * 16 >= NT_MIN_BYTES
    grid = _geom(n_chunks * 16, k)[1]
    xb = xcd_blocks_for(k, nt)
    sym = f"whvi::wbar_fwd_kernel<{dtype}, {log2d}, {k}, {_b(nt)}"
    return Launch(sym + ">", sym + ", false>", grid, nt, k, xb, xb == 0 and nt and grid % 8 == 0)


def bwd_flags(mean=False, no_lds=False, tiles=None):
    return (WBAR_MEAN if mean else 0) | (WBAR_NO_LDS if no_lds else 0) | {None: 0, "small": WBAR_SMALL_TILES,
                                                                         "big": WBAR_BIG_TILES}[tiles]


def wbar_bwd(dtype, log2d, J, S, R, flags=0):
    """launch_wbar_bwd behind wbar_bwd_dispatch's checks."""
    D = 1 << log2d
    if flags & ~(WBAR_MEAN | WBAR_NO_LDS | WBAR_SMALL_TILES | WBAR_BIG_TILES):
        raise ValueError("whvi_wbar_bwd: unknown flags")
    if not min_log2d(dtype) <= log2d <= max_single_pass_log2d(dtype):
        raise ValueError(f"whvi_wbar_bwd: log2(D) = {log2d} for {dtype}")
    if min(J, S, R) <= 0 or R > D or J * S * R >= 1 << 32:
        raise ValueError("whvi_wbar_bwd: sizes")
    mean, no_lds = bool(flags & WBAR_MEAN), bool(flags & WBAR_NO_LDS)
    small_tiles = 1 if flags & WBAR_SMALL_TILES else (-1 if flags & WBAR_BIG_TILES else 0)
    nb = J * S * R * D * SIZE[dtype]
    K, KS = pick_k(dtype, log2d), small_k(dtype, log2d)
    if KS < K and (small_tiles > 0 or (small_tiles == 0 and nb <= NT_MIN_BYTES)):
        sym = f"whvi::wbar_bwd_kernel<{dtype}, {log2d}, {KS}, false, {_b(mean)}, {POLICY_DPP}>"
        return Launch(sym, sym, _geom(nb, KS)[1], False, KS, policy="dpp")
    use_lds = lds_ok(dtype, log2d) and not no_lds and nb <= LDS_MAX_BYTES
    nt = nb > NT_MIN_BYTES
    grid = _geom(nb, K)[1]
    sym = f"whvi::wbar_bwd_kernel<{dtype}, {log2d}, {K}, {_b(nt)}, {_b(mean)}, {POLICY_LDS if use_lds else POLICY_DPP}>"
    return Launch(sym, sym, grid, nt, K, reorder=nt and grid % 8 == 0, policy="lds" if use_lds else "dpp")


def launch(case):
    """The mirror's answer for one case."""
    a = (case["dtype"], case["log2d"], case["J"], case["S"], case["R"])
    if case["entry"] == "wbar_fwd":
        return wbar_fwd(*a, base=case["base"])
    if case["entry"] == "wbar_fwd_mean":
        return wbar_fwd(*a, inline_mean=True)
    return wbar_bwd(*a, bwd_flags(case["mean"], case["no_lds"], case["tiles"]))


# ---- every instantiation the two dispatch functions make, and the ones no public argument reaches
def instantiated():
    """family -> the shipped symbols the dispatch instantiates, read off launch_wbar_fwd / launch_wbar_bwd."""
    fwd, bwd = set(), set()
    for T in SIZE:
        for L in log2ds(T):
            K, KS = pick_k(T, L), small_k(T, L)
            if L <= multi_pass_low_log2d(T):
                fwd.add(f"whvi::wbar_fwd_kernel<{T}, {L}, {mean_k(T, L)}, false, true>")
            if KS < K:
                fwd.add(f"whvi::wbar_fwd_kernel<{T}, {L}, {KS}, false, false>")
            for nt in (False, True):
                fwd.add(f"whvi::wbar_fwd_kernel<{T}, {L}, {K}, {_b(nt)}, false>")
            for mean in (False, True):
                if KS < K:
                    bwd.add(f"whvi::wbar_bwd_kernel<{T}, {L}, {KS}, false, {_b(mean)}, {POLICY_DPP}>")
                for nt in (False, True):
                    for pol in (POLICY_DPP,) + ((POLICY_LDS,) if lds_ok(T, L) else ()):
                        bwd.add(f"whvi::wbar_bwd_kernel<{T}, {L}, {K}, {_b(nt)}, {_b(mean)}, {pol}>")
    return {"wbar_fwd_kernel": fwd, "wbar_bwd_kernel": bwd}


def _unreachable():
    out = {}
    for T in SIZE:
        for L in log2ds(T):
            K, KS = pick_k(T, L), small_k(T, L)
            if KS < K:
                out[f"whvi::wbar_fwd_kernel<{T}, {L}, {K}, false, false>"] = (
                    "KS < K: up to 256 MiB takes the quarter tile, and what is left (> 256 MiB) satisfies >= 256 MiB: NT")
            if lds_ok(T, L):
                for mean in (False, True):
                    out[f"whvi::wbar_bwd_kernel<{T}, {L}, {K}, true, {_b(mean)}, {POLICY_LDS}>"] = (
                        "NT needs > 256 MiB, the LDS network <= 128 MiB")
    return out


UNREACHABLE = _unreachable()


# ---- the case list
CACHED_TILES = 9                               # cached cases: at least 9 of the 16 KiB (32 KiB) tiles = 3 blocks


def _sized(case, min_bytes, strict, reorder=None, cap=None):
    """The case at the smallest row count J S R whose matrices hold min_bytes (strict: more than) such that the tile count is
    no multiple of 4, the last tile is not full (where a row is shorter than a tile) and a streaming grid is on the asked side
    of the reorder condition -- conditions given up in that order, from the last, where no size has them all.  The row count
    splits into the case's J (else J = 1), S >= 2 where that is possible, and R: D where the case says so, otherwise the largest
    R up to the case's and above D / 2, so that every bit of the row index is set in some row.  Cached cases aim at 2 J (else J,
    else one) matrices under 64 MiB and stay under ``cap`` (default 255 MiB), streaming ones under 1.3 x 256 MiB and off the
    XCD-sliced order; a case whose R == D cannot fit takes an R < D."""
    D = 1 << case["log2d"]
    row = D * SIZE[case["dtype"]]
    stream = case["regime"] == "stream"
    cap = NT_MIN_BYTES * 13 // 10 if stream else (cap or 255 << 20)
    full = case["R"] == D
    short_rows = row < 64 * pick_k(case["dtype"], case["log2d"]) * 16
    tries = [(short_rows, reorder, True), (False, reorder, True), (False, None, True), (False, None, False)]
    for r_top in [case["R"]] + ([_less_than_d(D, 0)] if full and D > 1 else []):
        r_min = r_top if r_top == D else min(D // 2 + 1, r_top)
        rows0 = max(min_bytes // row + 1 if strict else _cdiv(min_bytes, row), r_min)
        if not stream:
            rows0 = max(rows0, next((n * r_min for n in (2 * case["J"], case["J"]) if n * r_min * row <= 64 << 20), r_min))
        top = min(cap // row, rows0 + max(6000, 2 * case["J"] * r_top))
        cands = sorted({(n * R, J != case["J"], -R, J, n // J, R)
                        for R in range(r_min, r_top + 1) for J in {case["J"], 1}
                        for n in range(_cdiv(_cdiv(rows0, R), J) * J, top // R + 1, J)})
        for need_ragged, side, off4 in tries:
            for min_s in (2, 1):
                for rows, _, _, J, S, R in cands:
                    if S < min_s:
                        continue
                    c = dict(case, J=J, S=S, R=R)
                    la = launch(c)
                    n_tiles, rag = _geom(rows * row, la.k)[0], (rows * row // 16) % (64 * la.k) != 0
                    if (off4 and n_tiles % 4 == 0) or (need_ragged and not rag) or (stream and (not la.nt or la.xcd_blocks)) or \
                            (side is not None and la.nt and la.reorder != side):
                        continue
                    return c
    raise AssertionError(f"{case['id']}: no size fits")


def _less_than_d(D, i):
    """An R < D: odd where D allows, and not a whole number of tiles."""
    return max(1, D - 1 - 2 * (i % 3)) if D > 8 else max(1, D - 1)


def _fwd_opts(i):
    """(first, spare rows behind the last one read, base) by index."""
    return i % 3, (i // 3) % 2, i % 2 == 1


def _build_cases():
    out = []
    i = 0
    for T in SIZE:
        n = NAMES[T]
        # ---- whvi_wbar_fwd
        for L in log2ds(T):
            D, K, KS = 1 << L, pick_k(T, L), small_k(T, L)
            row = D * SIZE[T]
            # cached: the quarter tile where it exists, else the 16 KiB (32 KiB) tile below 256 MiB
            first, spare, base = _fwd_opts(i)
            c = dict(id=f"fwd_{n}_L{L}_cached", entry="wbar_fwd", dtype=T, log2d=L, J=1 + i % 3, R=D if i % 2 else _less_than_d(D, i),
                     first=first, spare=spare, base=base, regime="cached", kind="inst")
            out.append(_sized(c, CACHED_TILES * 64 * K * 16, False))
            i += 1
            # streaming, not sliced: R < D so that no matrix is a whole number of groups
            first, spare, base = _fwd_opts(i)
            c = dict(id=f"fwd_{n}_L{L}_stream", entry="wbar_fwd", dtype=T, log2d=L, J=1 + i % 3, R=_less_than_d(D, i),
                     first=first, spare=spare, base=base, regime="stream", kind="inst")
            out.append(_sized(c, NT_MIN_BYTES, KS < K, reorder=i % 4 < 2))
            i += 1
            # streaming, XCD-sliced: every matrix a whole number of 8 x 4-tile groups, with base
            group = 64 * K * 4 * 8 * 16
            if D * row >= group:
                R = D // 2 if (D // 2) * row % group == 0 and i % 2 else D
                first, spare, _ = _fwd_opts(i)
                per_matrix = R * row
                mats = max(NT_MIN_BYTES // per_matrix + (1 if KS < K else 0), 2)
                J = 3 if mats >= 6 else 1
                S = _cdiv(mats, J)
                out.append(dict(id=f"fwd_{n}_L{L}_stream_sliced", entry="wbar_fwd", dtype=T, log2d=L, J=J, S=S, R=R, first=first,
                                spare=spare, base=True, regime="stream", kind="inst"))
                i += 1
        # ---- whvi_wbar_fwd_mean: one instantiation per D, R == D and R < D each
        for L in log2ds(T, "wbar_fwd_mean"):
            D = 1 << L
            for full in (True, False):
                c = dict(id=f"mean_{n}_L{L}_{'full' if full else 'short'}", entry="wbar_fwd_mean", dtype=T, log2d=L, J=1 + i % 3,
                         R=D if full else _less_than_d(D, i), regime="cached", kind="inst")
                out.append(_sized(c, CACHED_TILES * 64 * pick_k(T, L) * 16, False))
                i += 1
        # ---- whvi_wbar_bwd
        for L in log2ds(T):
            D, K, KS = 1 << L, pick_k(T, L), small_k(T, L)
            for mean in (False, True):
                def add(tag, regime, min_bytes, strict, no_lds, tl, short):
                    nonlocal i
                    c = dict(id=f"bwd_{n}_L{L}_{tag}{'_mean' if mean else ''}", entry="wbar_bwd", dtype=T, log2d=L, J=1 + i % 3,
                             R=_less_than_d(D, i) if short else D, mean=mean, no_lds=no_lds, tiles=tl, regime=regime, kind="inst")
                    out.append(_sized(c, min_bytes, strict, reorder=i % 4 < 2, cap=LDS_MAX_BYTES if tag == "big_lds" else None))
                    i += 1
                cached = CACHED_TILES * 64 * K * 16
                if KS < K:
                    add("small", "cached", cached, False, i % 2 == 0, "small" if i % 3 == 0 else None, i % 2 == 1)
                if lds_ok(T, L):
                    add("big_lds", "cached", cached, False, False, "big" if KS < K or i % 2 else None, i % 2 == 0)
                    add("big_dpp", "cached", cached, False, True, "big" if KS < K or i % 2 else None, i % 2 == 1)
                else:
                    add("big_dpp", "cached", cached, False, i % 2 == 0, "big" if KS < K or i % 2 else None, i % 2 == 1)
                add("stream", "stream", NT_MIN_BYTES, True, i % 2 == 0, "big" if i % 3 == 0 else None, True)
    return out + _boundary_cases()


def _rows_case(c, rows):
    """J = 1 and (S, R) with S R = rows, R the largest divisor of rows up to D."""
    D = 1 << c["log2d"]
    R = next(r for r in range(min(D, rows), 0, -1) if rows % r == 0)
    return dict(c, J=1, S=rows // R, R=R)


def _boundary_cases():
    """On the byte thresholds: exactly on, one row above (and, where `>=` decides, one row below)."""
    out = []
    for T, L_small, L_one in (("float", 10, 12), ("double", 9, 11)):
        n = NAMES[T]
        for L, entry in ((L_small, "wbar_fwd"), (L_one, "wbar_fwd"), (L_small, "wbar_bwd")):
            rows0 = NT_MIN_BYTES // (SIZE[T] << L)
            for tag, rows in (("below", rows0 - 1), ("exact", rows0), ("above", rows0 + 1)):
                if entry == "wbar_fwd":
                    if tag == "below" and L == L_small:
                        continue
                    c = dict(id=f"fwd_{n}_L{L}_256MiB_{tag}", entry=entry, dtype=T, log2d=L, first=1, spare=1, base=False)
                    out.append(_rows_case(dict(c, regime="boundary", kind="boundary"), rows))
                elif tag != "below":
                    for tl in (None, "big"):
                        c = dict(id=f"bwd_{n}_L{L}_256MiB_{tag}{'_big' if tl else ''}", entry=entry, dtype=T, log2d=L,
                                 mean=tag == "above", no_lds=True, tiles=tl)
                        out.append(_rows_case(dict(c, regime="boundary", kind="boundary"), rows))
    # the LDS / DPP switch of the 16 KiB tiles: exactly 128 MiB, and one tile (four rows of D = 1024) above
    rows0 = LDS_MAX_BYTES // (4 << 10)
    for tag, rows in (("exact", rows0), ("above", rows0 + 4)):
        c = dict(id=f"bwd_f32_L10_128MiB_{tag}_big", entry="wbar_bwd", dtype="float", log2d=10, mean=tag == "exact", no_lds=False,
                 tiles="big", regime="boundary", kind="boundary")
        out.append(_rows_case(c, rows))
    return out


CASES = _build_cases()


def reached():
    """The shipped symbols the case list launches."""
    return {launch(c).shipped for c in CASES}


def network(case):
    """"fwd" for the forward entries, else the backward's butterfly network."""
    return launch(case).policy or "fwd"


def nonfinite_cases():
    """One cached and one streaming case per (entry, type, network): the D = 512 one where the network exists there."""
    best = {}
    for c in CASES:
        if c["kind"] != "inst":
            continue
        key = (c["entry"], c["dtype"], network(c), launch(c).nt)
        if key not in best or (c["log2d"] == 9 and best[key]["log2d"] != 9):
            best[key] = c
    return list(best.values())


# Roundings on the longest path from an operand to a result of the backward, per butterfly network, read off wbar_bwd_kernel:
# grad_u / part_s2: the s1 scaling (1), one addition per stage of the transform (log2 D; fwht_tile and fwht_tile_lds both run
# log2 D stages of one add / sub each -- the LDS form only moves the lane-bit stages into registers), one per stage of the pruned
# butterfly (log2 D), the final product (1) and, for part_s2 under MEAN, the rounded sum u_k + u_mean (+1).  part_s1: u s2 (1),
# D . (exact), the product with the diagonal element (1), under MEAN the same rounded sum (+1).
def roundings(policy, log2d, mean):
    assert policy in ("lds", "dpp")
    return {"grad_u": 2 * log2d + 2, "part_s2": 2 * log2d + 2 + (1 if mean else 0), "part_s1": 2 + (1 if mean else 0)}


def main():
    for c in CASES:
        la = launch(c)
        print(f"{c['id']:34s} {la.shipped:58s} J {c['J']} S {c['S']:8d} R {c['R']:5d} grid {la.grid:7d} "
              f"{'nt' if la.nt else '  '} xcd {la.xcd_blocks:4d} {'reorder' if la.reorder else '       '} "
              f"{'ragged' if ragged(c) else '      '} {nbytes(c) / 2 ** 20:8.2f} MiB")
    for rule, op in THRESHOLDS.items():
        print(f"{rule:48s} {op}")
    inst = instantiated()
    print(f"{len(CASES)} cases; reached {len(reached())}, unreachable {len(UNREACHABLE)}, instantiated "
          f"{sum(len(s) for s in inst.values())}")


if __name__ == "__main__":
    main()
