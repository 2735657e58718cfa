#!/usr/bin/env python3
"""tools/kernel_table.py -- which template instantiation of the regression network's kernels each launch runs, and a case
list that reaches every one the library ships.

The dispatch (whvi_amd/csrc/layer_apply.hpp, diag_apply.hpp, mlp_apply.hpp, mlp_apply_bwd.hpp) picks an instantiation by
streamed bytes, by tile geometry and by tuning flags; the block order of the non-temporal (NT) launches also depends on the
grid, and so on the CU count.  The mirrors below restate those rules in Python: each takes shape, flags and CU count and
returns the demangled symbol ``whvi_last_kernel`` reports, every symbol the call launches (finishing kernels included), the
grid, whether the XCD-contiguous block order is on and, for diag_apply's forward, the block order as
whvi_diag_apply_order names it.  tests/test_kernel_table_host.py checks that ``CASES`` reaches exactly the shipped set of
each family; tests/test_kernel_table_gpu.py runs every case against float64 and checks the mirror against
``whvi_last_kernel``.  Pure Python: no torch, no GPU.

``ORDER_CASES`` are the launches of diag_apply's forward that tests/test_diag_apply_orders_gpu.py runs: each names the block
order (plain, XCD-contiguous, sample-fastest within an XCD) it must take.

    python tools/kernel_table.py [--cus N]        # every case with its symbol, grid and block order"""
import sys
from collections import namedtuple

NT_MIN_BYTES = 256 << 20            # dispatch.hpp: streaming launches beyond this many bytes
LONG_STREAM_BYTES = 4 << 30         # diag_apply_bwd_dispatch: XCD order + write-through grad_x stores from this many up
DIAG_X_SHARED, DIAG_MEAN_PLUS, DIAG_RELU_IN, DIAG_RELU_OUT = 1, 2, 4, 8           # include/whvi_hip.h
DIAG_TUNE_NT, DIAG_TUNE_CACHED, DIAG_TUNE_PLAIN_ORDER, DIAG_TUNE_BIG_TILES = 16, 32, 64, 128
MLP_MAX_LDS = 64 * 1024

FAMILIES = ("small_k_apply_kernel", "row_dot_kernel", "diag_apply_kernel", "diag_apply_bwd_kernel",
            "diag_apply_bwd_finish_kernel", "mlp_apply_kernel", "mlp_apply_bwd_kernel", "mlp_apply_bwd_finish_kernel")

# symbol: what whvi_last_kernel reports; symbols: every kernel the call launches; xcd: XCD-contiguous block order;
# order: diag_apply's forward only -- ORDER_PLAIN / ORDER_XCD / ORDER_SAMPLE_FASTEST, the values of whvi_diag_apply_order
Launch = namedtuple("Launch", "symbol symbols grid nt xcd order", defaults=(None,))
ORDER_PLAIN, ORDER_XCD, ORDER_SAMPLE_FASTEST = 0, 1, 2
ORDER_NAMES = ("plain", "xcd", "sample-fastest")

_SIZE = {"float": 4, "double": 8}


def family(symbol):
    """"whvi::row_dot_kernel<float, 10, true>" -> "row_dot_kernel"."""
    return symbol.split("<")[0].replace("whvi::", "")


def _b(v):
    return "true" if v else "false"


def _cdiv(a, b):
    return -(-a // b)


def _ilog2(n):
    return n.bit_length() - 1


def pick_k(dtype, log2d):
    """dispatch.hpp pick_k: 16-byte chunks per lane -- one row, but never fewer than the 64-register streaming tile."""
    size = _SIZE[dtype]
    vec = 16 // size
    lv = _ilog2(vec)
    need = 1 << (log2d - lv - 6) if log2d > lv + 6 else 1
    stream = 64 // (vec * size // 4)
    return max(need, stream)


def small_k_apply(S, B, N, log2k, cus):
    """small_k_apply_dispatch: column groups per thread from N, slabs of ~8 blocks per CU, NT above NT_MIN_BYTES."""
    cpr = N // 4
    tpr = 1
    while tpr < 256 and tpr * 2 <= cpr and cpr % (tpr * 2) == 0:
        tpr *= 2
    cpt = cpr // tpr
    if log2k not in (2, 3) or N % 4 or cpt > 4:
        raise ValueError(f"small_k_apply: unsupported K = 2^{log2k}, N = {N}")
    n_rg = 256 // tpr
    n_slabs = min(_cdiv(8 * cus, S), _cdiv(B, n_rg * 8))
    n_slabs = max(n_slabs, 1)
    slab_rows = _cdiv(B, n_slabs)
    n_slabs = _cdiv(B, slab_rows)
    grid = n_slabs * S
    nt = S * B * N * 4 > NT_MIN_BYTES
    sym = f"whvi::small_k_apply_kernel<float, {log2k}, {cpt}, {_b(nt)}>"
    return Launch(sym, (sym,), grid, nt, nt and grid % 8 == 0)


def row_dot(S, B, log2d):
    """row_dot_dispatch: 64 x 16-chunk tiles, four per block; NT above NT_MIN_BYTES of input."""
    if not 2 <= log2d <= 12:
        raise ValueError(f"row_dot: log2(D) = {log2d}")
    rows = S * B
    n_chunks = (rows << log2d) // 4
    grid = _cdiv(_cdiv(n_chunks, 64 * pick_k("float", log2d)), 4)
    nt = (rows << log2d) * 4 > NT_MIN_BYTES
    sym = f"whvi::row_dot_kernel<float, {log2d}, {_b(nt)}>"
    return Launch(sym, (sym,), grid, nt, nt and grid % 8 == 0)


def diag_max_log2d(dtype):
    return 12 if dtype == "float" else 11


def diag_apply(dtype, S, B, log2d, flags, in_place=False):
    """diag_apply_launch (diag_apply.hpp): NT by TUNE_NT / TUNE_CACHED or by the bytes streamed (x counted unless it is
    shared or the launch is in place); at cache-resident sizes quarter-size tiles (K = 4) for rows of up to four of their
    chunks, unless TUNE_BIG_TILES.  Block order: sample-fastest within an XCD for a shared input on an NT launch with S > 1,
    no TUNE_PLAIN_ORDER and every sample a whole number of 8-block groups; else XCD-contiguous for an NT grid that is a
    multiple of 8; else plain."""
    size = _SIZE[dtype]
    lv = _ilog2(16 // size)
    if not lv <= log2d <= diag_max_log2d(dtype):
        raise ValueError(f"diag_apply: log2(D) = {log2d} for {dtype}")
    shared = bool(flags & DIAG_X_SHARED)
    rows = S * B
    nbytes = (rows << log2d) * size
    if flags & DIAG_TUNE_NT:
        nt = True
    elif flags & DIAG_TUNE_CACHED:
        nt = False
    else:
        nt = (nbytes if shared or in_place else 2 * nbytes) > NT_MIN_BYTES
    k = pick_k(dtype, log2d)
    need = 1 << (log2d - lv - 6) if log2d > lv + 6 else 1
    if need <= 4 < k and not nt and not flags & DIAG_TUNE_BIG_TILES:
        k = 4
    grid = _cdiv(_cdiv((rows << log2d) * size // 16, 64 * k), 4)
    sym = f"whvi::diag_apply_kernel<{dtype}, {log2d}, {k}, {_b(nt)}, {_b(shared)}>"
    blk_chunks, per_sample = 4 * 64 * k, (B << log2d) * size // 16
    if shared and nt and S > 1 and not flags & DIAG_TUNE_PLAIN_ORDER and per_sample % (8 * blk_chunks) == 0:
        order = ORDER_SAMPLE_FASTEST
    else:
        order = ORDER_XCD if nt and grid % 8 == 0 else ORDER_PLAIN
    return Launch(sym, (sym,), grid, nt, order == ORDER_XCD, order)


def diag_apply_bwd_slabs(dtype, S, B, log2d, cus):
    """whvi_diag_apply_bwd_slabs: ~8 blocks per CU over the samples, at least 8 row steps per block."""
    cpr = 1 << (log2d - _ilog2(16 // _SIZE[dtype]))
    rg = 256 // cpr if cpr < 256 else 1
    n = max(min(_cdiv(8 * cus, S), _cdiv(B, rg * 8)), 1)
    slab_rows = _cdiv(B, n)
    return _cdiv(B, slab_rows)


def diag_apply_bwd(dtype, S, B, log2d, flags, need_grad_x, cus):
    """diag_apply_bwd_dispatch: NT by the tuning flags or by the bytes streamed (g and x, grad_x when wanted); the XCD order
    only on the long-stream path (from 4 GiB) of a grid that is a multiple of 8; then the finishing kernel."""
    size = _SIZE[dtype]
    nbytes = ((S * B) << log2d) * size * (3 if need_grad_x else 2)
    if flags & DIAG_TUNE_NT:
        nt = True
    elif flags & DIAG_TUNE_CACHED:
        nt = False
    else:
        nt = nbytes > NT_MIN_BYTES
    grid = diag_apply_bwd_slabs(dtype, S, B, log2d, cus) * S
    long_stream = nbytes >= LONG_STREAM_BYTES and not flags & DIAG_TUNE_PLAIN_ORDER
    sym = f"whvi::diag_apply_bwd_kernel<{dtype}, {log2d}, {_b(nt)}, {_b(flags & DIAG_X_SHARED)}, {_b(need_grad_x)}>"
    return Launch(sym, (sym, f"whvi::diag_apply_bwd_finish_kernel<{dtype}>"), grid, nt, nt and long_stream and grid % 8 == 0)


def mlp_supported(kin, n_mid, log2d):
    return kin in (1, 4, 8) and 1 <= n_mid <= 4 and 6 <= log2d <= 11 and (4 << log2d) * (kin + 2 + 2 * n_mid) <= MLP_MAX_LDS


def mlp_bwd_supported(kin, n_mid, log2d):
    return mlp_supported(kin, n_mid, log2d) and n_mid <= 2 and log2d <= 10


def mlp_apply(kin, n_mid, log2d):
    """mlp_apply_dispatch: one instantiation per (D, first-layer kind) inside the LDS range; the depth is a kernel argument."""
    if not mlp_supported(kin, n_mid, log2d):
        raise ValueError(f"mlp_apply: kin = {kin}, n_mid = {n_mid}, log2(D) = {log2d}")
    sym = f"whvi::mlp_apply_kernel<float, {log2d}, {kin}>"
    return Launch(sym, (sym,), None, False, False)


def mlp_apply_bwd(kin, n_mid, log2d):
    """mlp_apply_bwd_dispatch: one instantiation per (D, first-layer kind, depth), then the finishing kernel."""
    if not mlp_bwd_supported(kin, n_mid, log2d):
        raise ValueError(f"mlp_apply_bwd: kin = {kin}, n_mid = {n_mid}, log2(D) = {log2d}")
    sym = f"whvi::mlp_apply_bwd_kernel<float, {log2d}, {kin}, {n_mid}>"
    return Launch(sym, (sym, "whvi::mlp_apply_bwd_finish_kernel"), None, False, False)


# ---- the case list
# Every case is a dict with "id" and "family" (the entry point) and that entry point's arguments.  The NT launches of
# small_k_apply and row_dot have no forcing flag: their cases stream just over NT_MIN_BYTES, and "xcd" asks for one side of
# the grid % 8 == 0 condition -- sized() moves B up until the grid, for the CU count at hand, lands on that side.

def _spread(i):
    """Options spread over the cases by index: (mean_plus, bias, relu_in, relu_out, poisoned rows)."""
    return i % 2 == 0, i % 3 != 0, i % 4 == 1, i % 4 >= 2, (3 if i % 5 == 0 else 0)


def _small_k_cases():
    out = []
    # cache-resident: every (K, column groups per thread) -- N = 4 .. 4096
    for i, (k, n) in enumerate([(4, 4), (4, 2048), (4, 48), (4, 4096), (8, 1024), (8, 2048), (8, 3072), (8, 4096)]):
        out.append(dict(id=f"small_k_K{k}_N{n}", family="small_k_apply", K=k, N=n, S=1 + i % 3, B=37 + 29 * i,
                        bias=i % 2 == 0, relu_out=i % 3 == 1, xcd=None))
    # streaming, just over 256 MiB written: every (K, column groups) once, the two sides of the XCD condition alternating
    for i, (k, n) in enumerate([(4, 1024), (4, 2048), (4, 3072), (4, 4096), (8, 1024), (8, 2048), (8, 3072), (8, 4096)]):
        xcd = i % 2 == 0
        s = 8 if xcd else 3
        out.append(dict(id=f"small_k_nt_K{k}_N{n}", family="small_k_apply", K=k, N=n, S=s, B=_cdiv(NT_MIN_BYTES, s * n * 4) + 1,
                        bias=i % 3 != 0, relu_out=i % 2 == 1, xcd=xcd))
    # config 4's first layer exactly: 16 samples x 45 730 rows, K = 4 -> 1024, bias, ReLU behind (3.0 GB written)
    out.append(dict(id="small_k_config4", family="small_k_apply", K=4, N=1024, S=16, B=45730, bias=True, relu_out=True, xcd=None))
    return out


def _row_dot_cases():
    out = []
    for log2d in range(2, 13):
        out.append(dict(id=f"row_dot_L{log2d}", family="row_dot", log2d=log2d, S=3, B=29 + 5 * log2d, bias=log2d % 2 == 0,
                        relu_in=log2d % 3 == 0, poison=log2d % 4 == 0, xcd=None))
    for log2d in range(2, 13):
        s = 2 + log2d % 2
        out.append(dict(id=f"row_dot_nt_L{log2d}", family="row_dot", log2d=log2d, S=s, B=_cdiv(NT_MIN_BYTES, s * (4 << log2d)) + 1,
                        bias=log2d % 2 == 1, relu_in=log2d % 3 != 0, poison=log2d % 4 == 1, xcd=log2d % 2 == 0))
    # config 4's output layer exactly: 16 x 45 730 rows of D = 1024 (3.0 GB read), no ReLU in front (it is fused behind the
    # square layer), the bias added outside
    out.append(dict(id="row_dot_config4", family="row_dot", log2d=10, S=16, B=45730, bias=False, relu_in=False, poison=False,
                    xcd=None))
    return out


def _diag_cases():
    fwd, bwd = [], []
    i = 0
    for dtype in ("float", "double"):
        lv = 2 if dtype == "float" else 1
        for log2d in range(lv, diag_max_log2d(dtype) + 1):
            need = 1 << (log2d - lv - 6) if log2d > lv + 6 else 1
            quarter = need <= 4 < pick_k(dtype, log2d)
            tunes = [("default", 0), ("nt", DIAG_TUNE_NT)] + ([("big", DIAG_TUNE_CACHED | DIAG_TUNE_BIG_TILES)] if quarter else [])
            for name, tune in tunes:
                for shared in (False, True):
                    mean_plus, bias, relu_in, relu_out, poison = _spread(i)
                    S, B = 1 + i % 4, max(1, (24 << 10) // (1 << log2d)) + 3 * i % 17
                    fwd.append(dict(id=f"diag_{dtype}_L{log2d}_{name}{'_shared' if shared else ''}", family="diag_apply",
                                    dtype=dtype, log2d=log2d, S=S, B=B, shared=shared, mean_plus=mean_plus, bias=bias,
                                    relu_in=relu_in, relu_out=relu_out, poison=0 if shared else poison, tune=tune))
                    i += 1
            for tname, tune in (("cached", DIAG_TUNE_CACHED), ("nt", DIAG_TUNE_NT)):
                for shared in (False, True):
                    for gx in (False, True):
                        mean_plus, bias, relu_in, relu_out, poison = _spread(i)
                        S, B = 1 + i % 3, max(2, (16 << 10) // (1 << log2d)) + 5 * i % 23
                        bwd.append(dict(id=f"diag_bwd_{dtype}_L{log2d}_{tname}{'_shared' if shared else ''}{'_gx' if gx else ''}",
                                        family="diag_apply_bwd", dtype=dtype, log2d=log2d, S=S, B=B, shared=shared,
                                        mean_plus=mean_plus, bias=bias, relu_in=relu_in, relu_out=relu_out,
                                        poison=0 if shared else poison, need_grad_x=gx, tune=tune))
                        i += 1
    return fwd, bwd


def _order_cases():
    """diag_apply's forward on each of its three block orders (tests/test_diag_apply_orders_gpu.py).  "order" is the order
    the launch must take; "grid" the grid the comments of that suite quote.  Options are spread so that bias on / off, no
    mean row, relu_in and relu_out each occur under each order."""
    P, X, F = ORDER_PLAIN, ORDER_XCD, ORDER_SAMPLE_FASTEST
    NT = DIAG_TUNE_NT
    rows = [
        # id, dtype, log2d, S, B, shared, tune, order, grid, mean_plus, bias, relu_in, relu_out
        # ---- forced with DIAG_TUNE_NT, a few MiB each
        ("nt_L10_S3_one_group", "float", 10, 3, 128, True, NT, F, 24, True, True, False, False),      # one group per sample, odd S
        ("nt_L10_S7", "float", 10, 7, 128, True, NT, F, 56, False, False, True, False),
        ("nt_L12_S5_three_groups", "float", 12, 5, 96, True, NT, F, 120, True, True, False, True),
        ("nt_L9_S3", "float", 9, 3, 768, True, NT, F, 72, True, False, True, True),
        ("nt_L2_S2_shortest_rows", "float", 2, 2, 32768, True, NT, F, 16, False, True, False, False),
        ("nt_f64_L11_S5", "double", 11, 5, 64, True, NT, F, 80, True, True, True, False),
        ("nt_L10_S3_plain_order_flag", "float", 10, 3, 128, True, NT | DIAG_TUNE_PLAIN_ORDER, X, 24, False, True, False, True),
        ("nt_L10_S1_guard", "float", 10, 1, 128, True, NT, X, 8, True, False, True, False),              # the S > 1 guard
        ("nt_L10_S8_straddling", "float", 10, 8, 129, True, NT, P, 65, False, False, True, True),        # blocks straddle samples
        ("nt_L10_S3_per_sample", "float", 10, 3, 128, False, NT, X, 24, True, True, False, False),
        ("nt_L10_S3_per_sample_odd", "float", 10, 3, 130, False, NT, P, 25, True, True, False, False),
        # ---- dispatched by size (no tuning flag): 512 MiB .. 4 GiB written
        ("size_L10_S16_B8192", "float", 10, 16, 8192, True, 0, F, 8192, True, True, False, True),        # tools/diag_apply_rate.py
        ("size_L9_S32_B8192", "float", 9, 32, 8192, True, 0, F, 8192, True, False, True, False),         # config 2's width
        ("size_L11_S64_B8192", "float", 11, 64, 8192, True, 0, F, 65536, True, True, False, False),      # the bench's module leg
        ("size_f64_L11_S3_B16384", "double", 11, 3, 16384, True, 0, F, 12288, False, True, True, True),
        ("size_L10_S16_B8200", "float", 10, 16, 8200, True, 0, X, 8200, True, True, True, True),         # boundaries off samples
        ("size_L10_S16_B8192_per_sample", "float", 10, 16, 8192, False, 0, X, 8192, True, False, False, True),
    ]
    keys = ("id", "dtype", "log2d", "S", "B", "shared", "tune", "order", "grid", "mean_plus", "bias", "relu_in", "relu_out")
    out = []
    for r in rows:
        c = dict(zip(keys, r), family="diag_apply", poison=5)
        c["id"] = "order_" + c["id"]
        c["in_place_too"] = c["id"] == "order_size_L10_S16_B8192_per_sample"
        out.append(c)
    return out


ORDER_CASES = _order_cases()


def _mlp_cases():
    fwd, bwd = [], []
    i = 0
    for log2d in range(6, 12):
        for kin in (1, 4, 8):
            n_mid = next((n for n in (1 + i % 4, 3, 2, 1) if mlp_supported(kin, n, log2d)), None)
            if n_mid is not None:
                fwd.append(dict(id=f"mlp_L{log2d}_K{kin}_mid{n_mid}", family="mlp_apply", kin=kin, n_mid=n_mid, log2d=log2d,
                                S=1 + i % 5, B=300 + 97 * i % 900, relu=(5 * i + 3) % (1 << (n_mid + 1)),
                                mid_bias=(3 * i + 1) % (1 << n_mid), b_in=i % 3 != 1, b_out=i % 2 == 0, poison=i % 4 == 2))
            for n_mid in (1, 2):
                if mlp_bwd_supported(kin, n_mid, log2d):
                    bwd.append(dict(id=f"mlp_bwd_L{log2d}_K{kin}_mid{n_mid}", family="mlp_apply_bwd", kin=kin, n_mid=n_mid,
                                    log2d=log2d, S=1 + i % 4, B=100 + 131 * i % 700, relu=(3 * i + 1) % (1 << (n_mid + 1)),
                                    biases=tuple((i >> j) % 2 == 0 for j in range(n_mid + 2)), need_grad_x=i % 3 != 2))
            i += 1
    return fwd, bwd


def _build_cases():
    diag_fwd, diag_bwd = _diag_cases()
    mlp_fwd, mlp_bwd = _mlp_cases()
    return _small_k_cases() + _row_dot_cases() + diag_fwd + diag_bwd + mlp_fwd + mlp_bwd


CASES = _build_cases()


def launch(case, cus):
    """The mirror's answer for one case at its concrete size."""
    f = case["family"]
    if f == "small_k_apply":
        return small_k_apply(case["S"], case["B"], case["N"], _ilog2(case["K"]), cus)
    if f == "row_dot":
        return row_dot(case["S"], case["B"], case["log2d"])
    if f == "diag_apply":
        flags = case["tune"] | (DIAG_X_SHARED if case["shared"] else 0)
        return diag_apply(case["dtype"], case["S"], case["B"], case["log2d"], flags, case.get("in_place", False))
    if f == "diag_apply_bwd":
        flags = case["tune"] | (DIAG_X_SHARED if case["shared"] else 0)
        return diag_apply_bwd(case["dtype"], case["S"], case["B"], case["log2d"], flags, case["need_grad_x"], cus)
    if f == "mlp_apply":
        return mlp_apply(case["kin"], case["n_mid"], case["log2d"])
    if f == "mlp_apply_bwd":
        return mlp_apply_bwd(case["kin"], case["n_mid"], case["log2d"])
    raise ValueError(f)


def sized(case, cus):
    """The case at the size it runs at on a device with ``cus`` CUs: B moved up (by at most a thousand steps) until the grid
    lands on the side of the XCD condition the case asks for."""
    if case.get("xcd") is None:
        return dict(case)
    c = dict(case)
    # (row_dot's grid moves once per block of 4 x 64 x 16 chunks: step B by that many rows)
    step = _cdiv(max(1, (1 << 14) >> case["log2d"]), case["S"]) if case["family"] == "row_dot" else 1
    for _ in range(1000):
        got = launch(c, cus)
        assert got.nt, (c["id"], "the case must stream")
        if got.xcd == c["xcd"]:
            return c
        c["B"] += step
    raise AssertionError(f"{case['id']}: no batch size within 1000 steps gives xcd = {case['xcd']} on {cus} CUs")


def reached(cus=256):
    """family -> the set of shipped symbols the case list launches."""
    out = {f: set() for f in FAMILIES}
    for case in CASES:
        for sym in launch(sized(case, cus), cus).symbols:
            out[family(sym)].add(sym)
    return out


def main():
    cus = int(sys.argv[sys.argv.index("--cus") + 1]) if "--cus" in sys.argv else 256
    for case in CASES + ORDER_CASES:
        c = sized(case, cus)
        la = launch(c, cus)
        order = ORDER_NAMES[la.order] if la.order is not None else ("xcd" if la.xcd else "")
        print(f"{c['id']:40s} {la.symbol:62s} grid {la.grid} {order}")
    print(f"{len(CASES)} cases; " + ", ".join(f"{f}: {len(s)}" for f, s in reached(cus).items()))


if __name__ == "__main__":
    main()
