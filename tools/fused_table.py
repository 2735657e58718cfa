#!/usr/bin/env python3
"""tools/fused_table.py -- the fused forward whvi_fused_shs_* (fused_shs_kernel in whvi_amd/csrc/kernels.hpp, fused_shs16_kernel
in fused16.hpp): which instantiation each launch runs, how the kernel turns blockIdx.x into tiles, and a case list that reaches
every shipped instantiation under every block map the dispatch can give it.

The mirror restates, in Python, fused_plan of whvi_amd/csrc/dispatch.hpp -- the one host function launch_fused, launch_fused16
and the query whvi_fused_shs_plan call: pick_k, VEC, n_chunks, n_tiles, the 64-register tile test, ``big`` (32 tiles per CU,
16 for the 128-register tile), the streamed-byte rule (bytes counted once in place, with a NULL source and with a shared one),
rows per block, one-sample blocks, both same_sample_blocks rules, the stage choice, the SHARED / ONE template split and the
fused_small_kernel route for rows shorter than one 16-byte chunk.  ``launch(case, cus)`` returns the demangled symbol
``whvi_last_kernel`` reports, the grid, ``nt``, ``stage``, ``mode`` (same_sample_blocks) and the block map by name:

    plain            block b owns tiles 4 b .. 4 b + 3;
    xcd              streaming launch, grid a multiple of 8: XCD x owns a contiguous eighth of the blocks;
    sample-fastest   mode 2, a shared source with whole 8-block groups per sample: the sample index runs fastest within an XCD;
    ...+wave-strided mode 1, one 128-register row per tile, rows in (batch, sample, D) order and per-sample a / c: the four
                     waves of a block take rows n_samples apart, on top of plain or xcd.

``CASES`` holds one case per shipped symbol of fused_shs_kernel<float | double, ...> and fused_shs16_kernel<__half |
__hip_bfloat16, ...>, its block map rotating over what the symbol's class allows, plus the cases that complete the
(instantiation class x block map) matrix ``MATRIX`` and the mode-1 launches.  Each is the smallest shape of its regime at 256
CUs -- ``sized(case, cus)`` rescales it for another CU count:

    cached   three blocks;
    big      just past 32 tiles per CU (16 for the 128-register tile), cache-resident: the staged instantiations;
    stream   just past 256 MiB of working set (out of place: 128 MiB each way) and past ``big``.

Every case ends ragged -- rows past the last whole block, a partial last tile where a tile holds several rows -- except the
mode-1 and mode-2 launches, whose rules demand whole blocks, and five near misses of those rules (``whole_blocks``); every case has 3, 5 or 7 samples (the FastDiv
maps); in place / out of place, a / b / c present or NULL, per-sample a / c, the row order and group_rows are spread over the
cases by index.  tests/test_fused_table_host.py checks the list against the built library and the mirror against
whvi_fused_shs_plan; tests/test_fused_table_gpu.py runs every case, whole output, bit for bit.  Pure Python: no torch, no GPU.

    python tools/fused_table.py [--cus N]     # every case with its symbol, grid, nt, stage, mode, block map and MiB"""
import os
import sys
from collections import namedtuple

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
from kernel_table import NT_MIN_BYTES, family  # noqa: E402,F401
from kernel_table import pick_k as _pick_k_f32_f64  # noqa: E402

FAMILIES = ("fused_shs_kernel", "fused_shs16_kernel")
SIZE = {"float": 4, "double": 8, "__half": 2, "__hip_bfloat16": 2}
ACC_SIZE = {"float": 4, "double": 8, "__half": 4, "__hip_bfloat16": 4}          # Elem<T>::acc: the arithmetic type
DTYPE_CODE = {"float": 0, "double": 1, "__half": 2, "__hip_bfloat16": 4}         # include/whvi_hip.h: WHVI_F32 ...
NAMES = {"float": "f32", "double": "f64", "__half": "f16", "__hip_bfloat16": "bf16"}
MAX_LOG2D = {"float": 13, "double": 12, "__half": 13, "__hip_bfloat16": 13}      # max_single_pass_log2d
AXIS_ROW, AXIS_COL = 0, 1
A_PER_SAMPLE, C_PER_SAMPLE, SRC_SHARED, ONE_TRANSFORM = 1, 2, 4, 8
STAGE_NONE, STAGE_AC, STAGE_ABC = 0, 1, 3
MAPS = ("plain", "xcd", "sample-fastest", "plain+wave-strided", "xcd+wave-strided")
REF_SLAB_BYTES = 32 << 20          # the GPU test forms its reference chain a slab of rows at a time: at most this much per temporary
REF_TEMPORARIES = 6
MEMORY_CAP = 1 << 30

Launch = namedtuple("Launch", "symbol grid nt stage mode map big n_tiles")


def _b(v):
    return "true" if v else "false"


def _cdiv(a, b):
    return -(-a // b)


def vec(dtype):
    return 16 // SIZE[dtype]


def log2_vec(dtype):
    return vec(dtype).bit_length() - 1


def pick_k(dtype, log2d):
    """dispatch.hpp pick_k / fused_k: 16-byte chunks per lane -- one row, never below the 64-data-register streaming tile."""
    if SIZE[dtype] >= 4:
        return _pick_k_f32_f64(dtype, log2d)
    lv = log2_vec(dtype)
    need = 1 << (log2d - lv - 6) if log2d > lv + 6 else 1
    return max(need, 64 // (vec(dtype) * ACC_SIZE[dtype] // 4))


def small_tile(dtype, log2d):
    """tile_vgprs<T, K>() <= 64."""
    return pick_k(dtype, log2d) * vec(dtype) * ACC_SIZE[dtype] // 4 <= 64


def tile_rows(dtype, log2d):
    """Rows of one wave tile (1 once a row fills the tile)."""
    return max(1, (64 * pick_k(dtype, log2d) * vec(dtype)) >> log2d)


def rows_per_block(dtype, log2d):
    return (4 * 64 * pick_k(dtype, log2d) * vec(dtype)) >> log2d


def big_tiles(dtype, log2d, cus):
    return (32 if small_tile(dtype, log2d) else 16) * cus


def flags_of(case):
    return ((A_PER_SAMPLE if case["a_ps"] else 0) | (C_PER_SAMPLE if case["c_ps"] else 0) | (SRC_SHARED if case["shared"] else 0) |
            (ONE_TRANSFORM if case["one"] else 0))


def block_map(nt, grid, mode):
    """What the kernels do with blockIdx.x (kernels.hpp, fused16.hpp)."""
    if mode == 2:
        return "sample-fastest"
    return ("xcd" if nt and grid % 8 == 0 else "plain") + ("+wave-strided" if mode == 1 else "")


def plan(dtype, log2d, rows, n_samples, sample_stride, axis, flags, src_null, in_place, cus):
    """fused_plan (dispatch.hpp): (n_tiles, grid, big, nt, stage, mode)."""
    k, v = pick_k(dtype, log2d), vec(dtype)
    n_chunks = (rows << log2d) // v
    n_tiles = _cdiv(n_chunks, 64 * k)
    grid = _cdiv(n_tiles, 4)
    big = n_tiles >= big_tiles(dtype, log2d, cus)
    once = in_place or src_null or bool(flags & SRC_SHARED)
    nt = big and (n_chunks * 16 if once else 2 * n_chunks * 16) > NT_MIN_BYTES
    rpb = rows_per_block(dtype, log2d)
    per_sample_ac = bool(flags & (A_PER_SAMPLE | C_PER_SAMPLE))
    stage, mode = STAGE_NONE, 0
    if SIZE[dtype] == 2:
        one_sample = log2d >= 9 and (n_samples == 1 or sample_stride % rpb == 0)
        if log2d >= 9 and big:
            if one_sample and log2d <= 12:
                stage = STAGE_ABC
            elif one_sample or not per_sample_ac:
                stage = STAGE_AC
        return n_tiles, grid, big, nt, stage, mode
    one_sample = rpb >= 1 and sample_stride % rpb == 0
    if (flags & SRC_SHARED and rpb >= 1 and sample_stride % rpb == 0 and rows == n_samples * sample_stride and
            (sample_stride // rpb) % 8 == 0 and n_samples > 1):
        mode = 2
    if big:
        if one_sample or not per_sample_ac:
            stage = STAGE_AC
        elif (not small_tile(dtype, log2d) and rpb == 4 and sample_stride == 1 and n_samples > 1 and axis == AXIS_COL and
              not src_null and rows % (4 * n_samples) == 0 and n_tiles == rows):
            stage, mode = STAGE_AC, 1
    if not (axis == AXIS_COL and not src_null and 9 <= log2d <= 12 and big):
        stage = STAGE_NONE              # only the tuned column-axis launch has staged instantiations
    return n_tiles, grid, big, nt, stage, mode


def launch(case, cus):
    """The mirror's answer for one sized case."""
    T, L = case["dtype"], case["log2d"]
    lv = log2_vec(T)
    if not 0 <= L <= MAX_LOG2D[T] or (SIZE[T] == 2 and L < lv):
        raise ValueError(f"fused_shs: log2(D) = {L} for {T}")
    axis = AXIS_ROW if case["eye"] else case["axis"]
    if L < lv:                          # rows shorter than one chunk: a thread per row, no plan
        sym = f"whvi::fused_small_kernel<{T}, {L}, {axis}, {_b(case['eye'])}>"
        return Launch(sym, _cdiv(case["rows"], 256), False, STAGE_NONE, 0, "plain", False, 0)
    n_tiles, grid, big, nt, stage, mode = plan(T, L, case["rows"], case["n_samples"], case["sample_stride"], axis, flags_of(case),
                                               case["eye"], case["in_place"], cus)
    k = pick_k(T, L)
    if SIZE[T] == 2:
        sym = f"whvi::fused_shs16_kernel<{T}, {L}, {k}, {_b(nt)}, 0, {stage}, 256>"
    else:
        sym = (f"whvi::fused_shs_kernel<{T}, {L}, {k}, {axis}, {_b(case['eye'])}, {_b(nt)}, 256, 0, {stage}, {_b(case['shared'])}, "
               f"{_b(case['one'])}>")
    return Launch(sym, grid, nt, stage, mode, block_map(nt, grid, mode), big, n_tiles)


# ---- the shipped set, as the dispatch instantiates it
def classes(dtype, log2d):
    """The instantiation classes (axis, eye, nt, stage, shared, one) the dispatch instantiates for one (dtype, log2d)."""
    out = []
    if SIZE[dtype] == 2:
        stages = (STAGE_NONE, STAGE_AC, STAGE_ABC) if 9 <= log2d <= 12 else ((STAGE_NONE, STAGE_AC) if log2d == 13 else (STAGE_NONE,))
        return [(AXIS_COL, False, nt, st, False, False) for nt in (False, True) for st in stages]
    for eye in (False, True):
        out += [(AXIS_ROW, eye, nt, STAGE_NONE, False, False) for nt in (False, True)]
    halves = log2d - log2_vec(dtype) >= 6                # SRC_SHARED / ONE_TRANSFORM: rows of at least 64 chunks
    for nt in (False, True):
        for st in ((STAGE_NONE, STAGE_AC) if 9 <= log2d <= 12 else (STAGE_NONE,)):
            for shared, one in (((False, False), (False, True), (True, False), (True, True)) if halves else ((False, False),)):
                out.append((AXIS_COL, False, nt, st, shared, one))
    return out


def log2d_range(dtype):
    return range(log2_vec(dtype), MAX_LOG2D[dtype] + 1)


def symbol_of(dtype, log2d, cls):
    axis, eye, nt, st, shared, one = cls
    k = pick_k(dtype, log2d)
    if SIZE[dtype] == 2:
        return f"whvi::fused_shs16_kernel<{dtype}, {log2d}, {k}, {_b(nt)}, 0, {st}, 256>"
    return f"whvi::fused_shs_kernel<{dtype}, {log2d}, {k}, {axis}, {_b(eye)}, {_b(nt)}, 256, 0, {st}, {_b(shared)}, {_b(one)}>"


def maps_of(dtype, log2d, cls):
    """The block maps the dispatch can give one instantiation."""
    axis, eye, nt, st, shared, one = cls
    out = ["xcd", "plain"] if nt else ["plain"]
    staged_range = SIZE[dtype] >= 4 and 9 <= log2d <= 12
    # mode 2 needs whole blocks per sample, so a big launch of D = 512 .. 4096 stages a / c: never stage 0 and streaming there
    if shared and not (staged_range and nt and st == STAGE_NONE):
        out.append("sample-fastest")
    # mode 1: a big column launch of one-128-register-row tiles with per-sample a / c (f64 D = 4096 staged, f32 D = 8192 not)
    if (SIZE[dtype] >= 4 and axis == AXIS_COL and not eye and not small_tile(dtype, log2d) and not shared and not one and
            st == (STAGE_AC if staged_range else STAGE_NONE)):
        out += ["xcd+wave-strided", "plain+wave-strided"] if nt else ["plain+wave-strided"]
    return out


# A symbol the library ships that no argument list reaches.  None: every class of ``classes`` has a launch at every CU count up
# to 512 (beyond that, 32 tiles of 16 KiB per CU exceed the 256 MiB a cached launch may hold, and the big-but-cached staged
# forms would go unreached).
UNREACHABLE = ()


# ---- the case list
def _spread(i):
    """Options spread over the cases by index: (in_place, a, b, c present, a_ps, c_ps, n_samples, layout, group_rows kind)."""
    return (i % 2 == 0, i % 4 != 3, i % 3 != 0, i % 5 != 4, i % 3 != 1, i % 4 < 2, (3, 5, 7)[i % 3], ("batch", "sample", "odd")[i % 3],
            ("one", "odd", "D")[(i // 2) % 3])


def _spec(dtype, log2d, cls, want_map, i, tag=""):
    """One case before sizing: the options of index i, bent where the class demands it."""
    axis, eye, nt, st, shared, one = cls
    in_place, a, b, c, a_ps, c_ps, S, layout, gr = _spread(i)
    half = SIZE[dtype] == 2
    staged_range = 9 <= log2d <= 12 or (half and log2d == 13)
    regime = "stream" if nt else ("big" if st != STAGE_NONE or "wave" in want_map else "cached")
    mode = 1 if "wave" in want_map else (2 if want_map == "sample-fastest" else 0)
    if eye or shared:
        in_place = False
    if one:
        c = False
    if mode == 1:                       # rows in (batch, sample, D) order, per-sample a / c
        layout, a, c, a_ps, c_ps = "batch", True, not one, True, not one
    elif mode == 2:
        layout = "sample"
    elif axis == AXIS_COL and not eye and staged_range and regime != "cached":
        # which vectors are staged is decided by per-sample a / c against the row order
        if half and st == STAGE_ABC:
            layout = "sample"
        elif half and st == STAGE_AC and log2d <= 12:
            layout, a_ps, c_ps = ("batch" if layout == "sample" else layout), False, False
        elif st == STAGE_AC:
            if layout != "sample":
                a_ps = c_ps = False
        else:                           # stage 0 on a big launch: blocks that straddle samples, a per-sample vector
            layout = "batch" if layout == "sample" else layout
            a, a_ps = True, True
            if half:
                c_ps = c_ps and c
    a_ps, c_ps = a_ps and a, c_ps and c
    if in_place:
        b = True                        # y != x everywhere: an untouched tile shows in the bit compare
    cid = f"{NAMES[dtype]}_L{log2d}_{'eye' if eye else ('row' if axis == AXIS_ROW else 'col')}"
    if not half:
        cid += ("_shared" if shared else "") + ("_one" if one else "")
    cid += f"_st{st}_{'nt' if nt else 'c'}_{want_map.replace('+wave-strided', '_ws').replace('sample-fastest', 'sf')}{tag}"
    return dict(id=cid, dtype=dtype, log2d=log2d, axis=axis, eye=eye, shared=shared, one=one, regime=regime, want_map=want_map,
                want_symbol=symbol_of(dtype, log2d, cls), whole_blocks=mode != 0, n_samples=S, layout=layout, gr=gr,
                in_place=in_place, a=a, b=b, c=c, a_ps=a_ps, c_ps=c_ps)


def sized(case, cus):
    """The case at the smallest size of its regime on a device of ``cus`` CUs: rows, sample_stride and group_rows set, the grid
    moved (a block at a time, at most 16) to the side of the XCD condition the case's block map names.  A big-but-cached case
    that would stream out of place runs in place."""
    c = dict(case)
    T, L, S = c["dtype"], c["log2d"], c["n_samples"]
    D, rpb, tr = 1 << L, rows_per_block(T, L), tile_rows(T, L)
    row_bytes = D * SIZE[T]
    thr = big_tiles(T, L, cus)
    rag = 1 if tr == 1 else tr + 1                 # rows past the last whole block: one more tile, partial where tr > 1
    mode = 1 if "wave" in c["want_map"] else (2 if c["want_map"] == "sample-fastest" else 0)
    want_xcd = c["want_map"].startswith("xcd")
    c["group_rows"] = {"one": 1, "odd": 3 if D >= 3 else 1, "D": D}[c["gr"]] if (c["axis"] == AXIS_ROW or c["eye"]) else 1
    if c["regime"] == "big" and not (c["eye"] or c["shared"]) and 2 * (_cdiv(thr, 4) * rpb + rag) * row_bytes > NT_MIN_BYTES:
        c["in_place"], c["b"] = True, True
    once = c["in_place"] or c["eye"] or c["shared"]
    nt_rows = NT_MIN_BYTES // (row_bytes * (1 if once else 2)) + 1
    near = c.get("near_miss")
    for step in range(17):
        if near == "mode2":                         # whole blocks per sample, a multiple of FOUR per sample but not of eight
            m = 0 if c["regime"] == "cached" else max(_cdiv(thr, 32 * S), _cdiv(nt_rows, S * 8 * rpb))
            c["sample_stride"] = rpb * (8 * (m + step) + 4)
            c["rows"] = S * c["sample_stride"]
        elif near == "mode1":                       # one row per tile, whole blocks, but not whole groups of 4 S rows
            least = thr if c["regime"] == "big" else max(thr, nt_rows)
            c["rows"] = (_cdiv(least, 4 * S) + step) * 4 * S + 4
            c["sample_stride"] = 1
        elif mode == 2:                               # whole 8-block groups per sample, rows = S * stride
            groups = {"cached": 1, "big": _cdiv(thr, 32 * S), "stream": max(_cdiv(thr, 32 * S), _cdiv(nt_rows, S * 8 * rpb))}[c["regime"]]
            c["sample_stride"] = 8 * rpb * (groups + step)
            c["rows"] = S * c["sample_stride"]
        elif mode == 1:                             # one row per tile, whole groups of 4 S rows
            least = thr if c["regime"] == "big" else max(thr, nt_rows)
            c["rows"] = (_cdiv(least, 4 * S) + step) * 4 * S
            c["sample_stride"] = 1
        else:
            blocks = {"cached": 2, "big": _cdiv(thr, 4), "stream": max(_cdiv(thr, 4), nt_rows // rpb)}[c["regime"]] + step
            c["rows"] = blocks * rpb + rag
            if c["regime"] == "stream" and c["rows"] < nt_rows:
                continue
            per_sample = _cdiv(c["rows"], S)
            c["sample_stride"] = {"batch": 1, "sample": _cdiv(per_sample, rpb) * rpb,
                                  "odd": per_sample + (1 if per_sample % rpb == 0 else 0)}[c["layout"]]
        la = launch(c, cus)
        if not la.nt or mode == 2 or (la.grid % 8 == 0) == want_xcd:
            break
    else:
        raise AssertionError(f"{c['id']}: no size within 16 steps lands on {c['want_map']}")
    assert la.symbol == c["want_symbol"], (c["id"], cus, la.symbol, c["want_symbol"])
    assert la.map == c["want_map"], (c["id"], cus, la.map)
    return c


def in_regime(case, cus):
    """The case's shape is in the regime its id names: the wanted symbol under the wanted block map, with a first, a middle and
    a last block."""
    la = launch(case, cus)
    if case.get("near_miss") == "mode2" and case["rows"] != case["n_samples"] * case["sample_stride"]:
        return False
    if case.get("near_miss") == "mode1" and not (la.big and case["rows"] % 4 == 0):
        return False
    return la.symbol == case["want_symbol"] and la.map == case["want_map"] and la.grid >= 3


def halved(case):
    """The case at half its row count (the row order kept: sample_stride halves with the rows where it is the batch size)."""
    c = dict(case, rows=case["rows"] // 2)
    return c


def block_tiles(la, n_samples, block):
    """The tiles the four waves of block ``blockIdx.x == block`` own under the launch's block map, as the kernels compute them
    (tiles past n_tiles are idle waves)."""
    if la.mode == 2:
        xcd, i = block & 7, block >> 3
        q, smp = divmod(i, n_samples)
        blk = smp * (la.grid // n_samples) + q * 8 + xcd
    elif la.nt and la.grid % 8 == 0:
        blk = (block & 7) * (la.grid >> 3) + (block >> 3)
    else:
        blk = block
    if la.mode == 1:
        q, smp = divmod(blk, n_samples)
        return [(q * 4 + w) * n_samples + smp for w in range(4)]
    return [blk * 4 + w for w in range(4)]


def ragged(case):
    """Rows past the last whole block, and a partial last tile where a tile holds several rows."""
    T, L = case["dtype"], case["log2d"]
    tr = tile_rows(T, L)
    return case["rows"] % rows_per_block(T, L) != 0 and (tr == 1 or case["rows"] % tr != 0)


def io_bytes(case):
    """(source bytes, destination bytes) the launch touches."""
    row = (1 << case["log2d"]) * SIZE[case["dtype"]]
    dst = case["rows"] * row
    src = 0 if case["eye"] or case["in_place"] else (case["sample_stride"] if case["shared"] else case["rows"]) * row
    return src, dst


def held_bytes(case):
    """Device memory tests/test_fused_table_gpu.py holds at once for the case: source, destination, the source's copy of an
    in-place launch, the float32 reference launch of a 16-bit case (in place on the upcast input when the case is), and the
    slab-sized temporaries of the reference chain."""
    src, dst = io_bytes(case)
    if SIZE[case["dtype"]] == 2:     # and float32: the upcast input (which stands in for the source's copy), its output unless in place
        total = src + dst + 2 * dst + (0 if case["in_place"] else 2 * dst)
    else:
        total = src + dst + (dst if case["in_place"] else 0)
    return total + REF_TEMPORARIES * REF_SLAB_BYTES


def _build_specs():
    out, turn = [], {}
    for T in ("float", "double", "__half", "__hip_bfloat16"):
        for L in log2d_range(T):
            for cls in classes(T, L):
                maps = [m for m in maps_of(T, L, cls) if "wave" not in m]
                n = turn.get((SIZE[T] == 2, cls), 0)
                turn[(SIZE[T] == 2, cls)] = n + 1
                out.append(_spec(T, L, cls, maps[n % len(maps)], len(out)))
    # the (instantiation class x block map) pairs the rotation left out, and the mode-1 launches: each on the first
    # (dtype, log2d) that allows the pair
    have = {((SIZE[s["dtype"]] == 2,) + _class_of(s), s["want_map"]) for s in out}
    for T in ("float", "double", "__half", "__hip_bfloat16"):
        for L in log2d_range(T):
            for cls in classes(T, L):
                for m in maps_of(T, L, cls):
                    key = ((SIZE[T] == 2,) + cls, m)
                    if key not in have or ("wave" in m and not any(s["want_symbol"] == symbol_of(T, L, cls) and s["want_map"] == m for s in out)):
                        have.add(key)
                        out.append(_spec(T, L, cls, m, len(out), "_x"))
    # near misses of the two same_sample_blocks rules, on whole blocks: four blocks per sample short of mode 2's eight (cached,
    # streaming, streaming and staged), and rows that are a multiple of 4 but not of 4 n_samples where mode 1 would apply
    C = AXIS_COL
    for T, L, cls, m, over in (
            ("float", 10, (C, False, False, STAGE_NONE, True, False), "plain", dict(near_miss="mode2")),
            ("float", 8, (C, False, True, STAGE_NONE, True, True), "plain", dict(near_miss="mode2")),
            ("double", 11, (C, False, True, STAGE_AC, True, False), "plain", dict(near_miss="mode2")),
            ("double", 12, (C, False, False, STAGE_NONE, False, False), "plain", dict(near_miss="mode1", regime="big")),
            ("float", 13, (C, False, True, STAGE_NONE, False, False), "xcd", dict(near_miss="mode1"))):
        sp = _spec(T, L, cls, m, len(out), "_near_" + over["near_miss"])
        sp.update(over, whole_blocks=True, n_samples=3)
        if over["near_miss"] == "mode1":
            sp.update(layout="batch", a=True, c=True, a_ps=True, c_ps=True)
        out.append(sp)
    return out


def _class_of(spec):
    sym = spec["want_symbol"]
    args = sym[sym.index("<") + 1:-1].split(", ")
    if "16_kernel" in sym:
        return (AXIS_COL, False, args[3] == "true", int(args[5]), False, False)
    return (int(args[3]), args[4] == "true", args[5] == "true", int(args[8]), args[9] == "true", args[10] == "true")


def matrix():
    """{(16-bit?, class): set of block maps}: what the dispatch can produce."""
    out = {}
    for T in SIZE:
        for L in log2d_range(T):
            for cls in classes(T, L):
                out.setdefault((SIZE[T] == 2,) + cls, set()).update(maps_of(T, L, cls))
    return out


MATRIX = matrix()
SPECS = _build_specs()
CASES = [sized(s, 256) for s in SPECS]


def shipped():
    """Every symbol of the two families the dispatch instantiates."""
    return {symbol_of(T, L, cls) for T in SIZE for L in log2d_range(T) for cls in classes(T, L)}


def reached(cus=256):
    """The symbols the case list launches on a device of ``cus`` CUs."""
    return {launch(sized(s, cus), cus).symbol for s in SPECS}


def covered(cus=256):
    """{(16-bit?, class): set of block maps} the case list exercises."""
    out = {}
    for s in SPECS:
        out.setdefault((SIZE[s["dtype"]] == 2,) + _class_of(s), set()).add(launch(sized(s, cus), cus).map)
    return out


def main():
    cus = int(sys.argv[sys.argv.index("--cus") + 1]) if "--cus" in sys.argv else 256
    for s in SPECS:
        c = sized(s, cus)
        la = launch(c, cus)
        src, dst = io_bytes(c)
        print(f"{c['id']:44s} {la.symbol:88s} rows {c['rows']:8d} S {c['n_samples']} stride {c['sample_stride']:7d} grid {la.grid:7d} "
              f"{'nt' if la.nt else '  '} stage {la.stage} mode {la.mode} {la.map:18s} {'in place ' if c['in_place'] else ''}"
              f"{'whole blocks ' if c['whole_blocks'] else ''}{(src + dst) / 2 ** 20:7.1f} MiB")
    got = reached(cus)
    print(f"{len(SPECS)} cases at {cus} CUs reach {len(got)} of {len(shipped())} symbols; "
          f"{sum(len(v) for v in covered(cus).values())} of {sum(len(v) for v in MATRIX.values())} (class, block map) pairs")
    print("unreachable: " + (", ".join(UNREACHABLE) if UNREACHABLE else "none"))
    for sym in sorted(shipped() - got - set(UNREACHABLE)):
        print("NOT REACHED:", sym)


if __name__ == "__main__":
    main()
