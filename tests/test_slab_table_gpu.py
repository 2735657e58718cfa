"""Every shipped instantiation of the slab-walking kernels past one tile per wave, cached and streaming: the case list of
tools/slab_table.py (tests/test_slab_table_host.py checks that it reaches exactly the shipped set) against float64.

The six templates on fused_bwd_geom -- fused_shs_bwd_kernel, fused_shs_stacked_kernel, fused_stacked16_kernel,
fused_shs_stacked_bwd_kernel, fused_shs_stacked_layer_kernel, fused_shs_stacked_layer_bwd_kernel -- and their three finishing
kernels.  A ``walk`` case is cached with at least three tiles per wave, a ``stream`` case is the smallest launch that takes the
NT = true instantiation (at least two tiles per wave); both have S = 3 and a last slab that ends inside a tile.

Each case writes into output buffers with sentinel margins whose interior is prefilled with a NaN payload no arithmetic makes
(tests/test_kernel_table_gpu.py's _guarded / _intact / _unwritten; 16-bit twins here).  The forward entries run through their
``_hip`` wrappers (``out=``); the backward entries through the C ABI the wrappers call, so that the parameter gradients, which
the wrappers allocate themselves, are guarded too.  Common to every launch: whvi_last_kernel is the mirror's symbol, every output
element is written (the columns past n_cols of a padded pitch keep the fill), every margin is intact; in test (a) also: the
inputs are unchanged and a second call gives the same bits.

(a) test_integer_operands_exact.  a, b, c are seeded +-1, x has exactly three seeded +-1 per row, grad_y is +-1 (three +-1 per
    row for 16-bit activations: |grad_x| <= 3 D stays finite in fp16), the bias holds integers in [-3, 3].  Every product and
    partial sum is then an integer, so the float32 result does not depend on summation order, tiling, slab count or contraction
    as long as no partial sum leaves +-2^24.  That is asserted on the reference: for every parameter gradient A64, the float64
    sum of the absolute values of the element's terms, is below 2^24 (it bounds every partial sum in any order), and so is the
    row sum of |v| that bounds the butterflies of the last transform.  It is a condition of the test, not a tolerance.  Every
    output must then EQUAL the float64 reference (after + 0.0; 16-bit outputs equal ref64.to(dtype), the one rounding the
    kernel is specified to make): y, grad_x, grad_a / b / c, grad_bias, with relu_in, relu_out, the bias and the narrowing
    applied in the reference.  A lost, repeated or misplaced row anywhere in a slab changes an integer.

(b) test_gaussian_operands_against_one_tile_slices.  Seeded randn operands (1 / sqrt(D) on a and b for 16 bits, as
    tests/test_fastfood_stacked16_gpu.py).  The forward output and grad_x are functions of their own row, so they must have the
    bits of the same entry point called on row slices -- one sample and at most slab_table.one_tile_rows(log2d) rows per call,
    which the mirror confirms is cached with one tile per wave: the regime the older tests hold to float64 and to the oracle.
    Compared as tests/test_fastfood_stacked_gpu.py::_assert_same does: values after + 0.0, NaN and inf positions.  Cases with
    ``poison`` repeat this with +-inf and NaN planted in two rows of x, one in the first tile of a wave and one in the next tile
    of the same wave.  The parameter gradients are held to the rule of
    tests/test_fastfood_stacked_bwd_gpu.py::test_gradients_against_float64: max|got - ref64| <= 1e-5 max|ref64| per tensor, the
    ratio of the sliced calls' gradients added in float32 printed beside the launch's; a tensor on which the sliced route
    itself misses the bound is reported and not charged to the launch.  The worst ratios are recorded in DESIGN.md 5.2j.

References are float64 autograd of the dense product with build_H(D), formed on the device one sample at a time."""
import os
import sys

import pytest
import torch

from whvi_amd import _hip

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, HERE)
sys.path.insert(0, os.path.join(os.path.dirname(HERE), "tools"))
import slab_table as st  # noqa: E402
from test_batched_bwd_gpu import PAD  # noqa: E402
from test_fastfood_stacked_gpu import _assert_same  # noqa: E402
from test_kernel_table_gpu import _guarded, _intact, _unwritten  # noqa: E402

pytestmark = pytest.mark.gpu
DEV = "cuda"
F32 = torch.float32
DT = {"float": torch.float32, "__half": torch.float16, "__hip_bfloat16": torch.bfloat16}
FILL16 = {torch.float16: 0x7E5A, torch.bfloat16: 0x7FDA}       # quiet NaNs with a payload no conversion makes
SENT16 = -776.0                                                 # exact in both 16-bit types
BOUND = 1e-5                                                    # tests/test_fastfood_stacked_bwd_gpu.py: BOUND
LIMIT = float(1 << 24)
ROW_OUTPUTS = ("out", "gx")
SUMS = ("ga", "gb", "gc", "gbias")
_H = {}

cases = pytest.mark.parametrize("case", st.CASES, ids=lambda c: c["id"])


def _h(D):
    if D not in _H:
        from whvi_amd.utils import build_H
        _H[D] = build_H(D, torch.device(DEV)).double()
    return _H[D]


# ---- guarded buffers, both widths
def _new(shape, dtype):
    if dtype == F32:
        return _guarded(shape, dtype)
    n = 1
    for v in shape:
        n *= v
    buf = torch.full((n + 2 * PAD,), SENT16, device=DEV, dtype=dtype)
    buf[PAD:PAD + n].view(torch.int16).fill_(FILL16[dtype])
    return buf, buf[PAD:PAD + n].view(shape)


def _margins_intact(buf, view):
    if buf.dtype == F32:
        return _intact(buf, view)
    return bool((buf[:PAD] == SENT16).all()) and bool((buf[PAD + view.numel():] == SENT16).all())


def _holes(view):
    """Elements that still hold the fill."""
    if view.dtype == F32:
        return _unwritten(view)
    return int((view.view(torch.int16) == FILL16[view.dtype]).sum())


def _raw(t):
    return t.view(torch.int32 if t.dtype == F32 else torch.int16)


# ---- operands
def _dims(case):
    J = case.get("J", 1)
    D = 1 << case["log2d"]
    return case["S"], case["B"], J, D, case.get("n_cols", J * D), case.get("ld", J * D)


def _pm1(shape, g, dtype=F32):
    return (torch.randint(0, 2, shape, device=DEV, generator=g) * 2 - 1).to(dtype)


def _three_per_row(rows, D, g, dtype):
    """Exactly three +-1 per row at seeded, distinct columns, zero elsewhere."""
    out = torch.zeros(rows, D, device=DEV, dtype=dtype)
    p = torch.randint(0, D, (rows, 1), device=DEV, generator=g)
    o = torch.randint(1, D // 2, (rows, 2), device=DEV, generator=g)          # two steps of 1 .. D/2 - 1: no column twice
    pos = torch.cat([p, p + o[:, :1], p + o[:, :1] + o[:, 1:]], dim=1) % D
    out.scatter_(1, pos, _pm1((rows, 3), g, dtype))
    assert int((out != 0).sum()) == 3 * rows
    return out


def _pitched(rows, n_cols, ld, dtype=F32):
    """(the whole (rows, ld) buffer, its first n_cols columns): the gap columns hold NaN and must never be read."""
    full = torch.full((rows, ld), float("nan"), device=DEV, dtype=dtype)
    return full, full[:, :n_cols]


def _operands(case, integer):
    """x, a (J, D), b (J, S, D), c (J, D); bias (J D) for the layer entries; gy (rows, n_cols) at pitch ld for the backward
    entries; for fused_shs_stacked_layer_bwd also y_full / y, filled in later (relu_out reads it)."""
    S, B, J, D, n_cols, ld = _dims(case)
    e, dt, rows = case["entry"], DT[case["dtype"]], S * B
    g = torch.Generator(device=DEV).manual_seed(7919 * st.CASES.index(case) + (1 if integer else 2))
    xr = B if case["shared"] else rows
    t = {}
    if integer:
        t["x"] = _three_per_row(xr, D, g, dt)
        t["a"], t["c"], t["b"] = _pm1((J, D), g), _pm1((J, D), g), _pm1((J, S, D), g)
    else:
        scale = 1.0 if dt == F32 else 1.0 / D ** 0.5
        t["x"] = torch.randn(xr, D, device=DEV, generator=g).to(dt)
        t["a"] = torch.randn(J, D, device=DEV, generator=g) * scale
        t["b"] = torch.randn(J, S, D, device=DEV, generator=g) * scale
        t["c"] = torch.randn(J, D, device=DEV, generator=g)
    if e.startswith("fused_shs_stacked_layer"):
        # the backward's forward always has a bias (y is only an input there); the forward case has one when it says so
        if e.endswith("_bwd") or case["bias"]:
            t["bias"] = (torch.randint(-3, 4, (J * D,), device=DEV, generator=g).float() if integer
                         else torch.randn(J * D, device=DEV, generator=g))
    if e.endswith("_bwd"):
        t["gy_full"], t["gy"] = _pitched(rows, n_cols, ld, dt)
        if integer:
            t["gy"].copy_(_pm1((rows, n_cols), g, dt) if dt == F32 else _three_per_row(rows, n_cols, g, dt))
        else:
            t["gy"].copy_(torch.randn(rows, n_cols, device=DEV, generator=g).to(dt))
        if case.get("relu_out"):
            t["y_full"], t["y"] = _pitched(rows, n_cols, ld)
    return t


# ---- one launch
def _run(case, t, s=None, r0=0, r1=None):
    """The case's entry point on its operands -- or, with ``s``, on rows r0 .. r1 - 1 of sample ``s`` alone (S = 1).  Returns
    (outputs by name, [(buffer, guarded view)], the kernel whvi_last_kernel names)."""
    S, B, J, D, n_cols, ld = _dims(case)
    e, dt, L = case["entry"], DT[case["dtype"]], case["log2d"]
    shared = case["shared"]
    x, a, b, c, bias, gy, y = t["x"], t["a"], t["b"], t["c"], t.get("bias"), t.get("gy"), t.get("y")
    if s is not None:
        x = x[r0:r1] if shared else x[s * B + r0:s * B + r1]
        b = b[:, s:s + 1].contiguous()
        gy = None if gy is None else gy[s * B + r0:s * B + r1]
        y = None if y is None else y[s * B + r0:s * B + r1]
        S, B = 1, r1 - r0
    rows = S * B
    bufs, outs = [], {}

    def new(name, shape, width=None):
        buf, full = _new(shape, dt if name in ROW_OUTPUTS else F32)
        bufs.append((buf, full))
        outs[name] = full if width is None else full[:, :width]
        return outs[name]

    flags = ((_hip.FUSED_SRC_SHARED if shared else 0) | (_hip.FUSED_RELU_IN if case.get("relu_in") else 0)
             | (_hip.FUSED_RELU_OUT if case.get("relu_out") else 0))
    lib = _hip.lib()
    if e == "fused_shs_stacked":
        _hip.fused_shs_stacked(x, a, b, c, S, B, shared=shared, out=new("out", (rows, J * D)))
    elif e == "fused_shs_stacked16":
        _hip.fused_shs_stacked16(x, a, b, c, S, B, shared=shared, out=new("out", (rows, J * D)))
    elif e == "fused_shs_stacked_layer":
        _hip.fused_shs_stacked_layer(x, a, b, c, S, B, bias=bias, n_cols=n_cols, relu_in=case["relu_in"], relu_out=case["relu_out"],
                                     shared=shared, out=new("out", (rows, ld), n_cols))
    else:
        gx = new("gx", (rows, D)) if case["need_x"] else None
        ga, gb, gc = new("ga", (J, D)), new("gb", (J, S, D)), new("gc", (J, D))
        gxp = None if gx is None else gx.data_ptr()
        if e == "fused_shs_bwd":
            work = torch.empty((max(int(lib.whvi_fused_shs_bwd_workspace(S, B, L)), 16),), dtype=torch.uint8, device=DEV)
            fn = getattr(lib, "whvi_fused_shs_bwd_" + _hip._DTYPE_SUFFIX[dt])
            rc = fn(gxp, ga.data_ptr(), gb.data_ptr(), gc.data_ptr(), work.data_ptr(), gy.data_ptr(), x.data_ptr(), a.data_ptr(),
                    b.data_ptr(), c.data_ptr(), S, B, L, flags, None)
        elif e == "fused_shs_stacked_bwd":
            work = torch.empty((max(int(lib.whvi_fused_shs_stacked_bwd_workspace(S, B, L, J)), 16),), dtype=torch.uint8, device=DEV)
            rc = lib.whvi_fused_shs_stacked_bwd_f32(gxp, ga.data_ptr(), gb.data_ptr(), gc.data_ptr(), work.data_ptr(), gy.data_ptr(),
                                                    x.data_ptr(), a.data_ptr(), b.data_ptr(), c.data_ptr(), J, S, B, L, flags, None)
        else:
            gbias = new("gbias", (J * D,)) if case["bias"] else None
            n = int(lib.whvi_fused_shs_stacked_layer_bwd_workspace(S, B, L, J, int(case["bias"])))
            work = torch.empty((max(n, 16),), dtype=torch.uint8, device=DEV)
            rc = lib.whvi_fused_shs_stacked_layer_bwd_f32(gxp, ga.data_ptr(), gb.data_ptr(), gc.data_ptr(),
                                                          None if gbias is None else gbias.data_ptr(), work.data_ptr(), gy.data_ptr(),
                                                          None if y is None else y.data_ptr(), x.data_ptr(), a.data_ptr(),
                                                          b.data_ptr(), c.data_ptr(), J, S, B, L, n_cols, ld, flags, None)
        assert rc == 0, _hip.last_error()
    kernel = _hip.last_kernel()
    torch.cuda.synchronize()
    return outs, bufs, kernel


def _common(case, outs, bufs, kernel, sub=None):
    """whvi_last_kernel is the mirror's symbol; every output element written but the gap of a padded pitch; margins intact."""
    want = st.launch(case if sub is None else sub)
    assert kernel == want.symbol, (kernel, want.symbol)
    for buf, full in bufs:
        assert _margins_intact(buf, full), "a byte outside an output changed"
    _, _, J, D, n_cols, ld = _dims(case)
    for name, view in outs.items():
        assert _holes(view) == 0, (name, "elements never written", _holes(view))
    if "out" in outs and ld > n_cols:
        gap = [full for _, full in bufs if full.data_ptr() == outs["out"].data_ptr()][0][:, n_cols:]
        assert _holes(gap) == gap.numel(), "columns past n_cols of the padded pitch were written"
    return want


# ---- the float64 reference, one sample at a time
def _reference(case, t, exact, rows_too=True):
    """float64 autograd of the dense product from the case's float32 / 16-bit operands.  Returns the expected outputs by name:
    ``out`` / ``gx`` in the storage type (``rows_too``), the parameter gradients in float64.  relu_out masks by ``t['y']`` where
    the operands bring one (the backward of the layer reads the forward's y), else by the reference's own sign -- and writes the
    reference's y there first when ``exact``.  ``exact``: also the conditions of test (a) -- every float32 result is the
    reference exactly and every sum of absolute terms is below 2^24."""
    S, B, J, D, n_cols, ld = _dims(case)
    e, dt = case["entry"], DT[case["dtype"]]
    bwd, shared = e.endswith("_bwd"), case["shared"]
    relu_in, relu_out, need_x = bool(case.get("relu_in")), bool(case.get("relu_out")), bool(case.get("need_x"))
    H = _h(D)
    ref = {}
    if rows_too and not bwd:
        ref["out"] = torch.empty(S * B, n_cols, device=DEV, dtype=dt)
    if bwd:
        if rows_too and need_x:
            ref["gx"] = torch.empty(S * B, D, device=DEV, dtype=dt)
        ref["ga"], ref["gc"] = (torch.zeros(J, D, device=DEV, dtype=torch.float64) for _ in range(2))
        ref["gb"] = torch.zeros(J, S, D, device=DEV, dtype=torch.float64)
        if case.get("bias"):
            ref["gbias"] = torch.zeros(J * D, device=DEV, dtype=torch.float64)
    A = {k: torch.zeros_like(v) for k, v in ref.items() if k in SUMS}
    chain = 0.0

    def stored(v64, what):
        v = v64.to(dt)
        if exact and dt == F32:
            assert torch.equal(v.double(), v64), (what, "the reference is not a float32 integer")
        return v

    for s in range(S):
        sl = slice(s * B, (s + 1) * B)
        xs = (t["x"][:B] if shared else t["x"][sl]).double().requires_grad_(bwd and need_x)
        a, c, b = (t["a"].double().requires_grad_(bwd), t["c"].double().requires_grad_(bwd),
                   t["b"][:, s].double().requires_grad_(bwd))
        bias = t["bias"].double().requires_grad_(bwd) if "bias" in t else None
        xin = torch.relu(xs) if relu_in else xs
        t1 = [(c[j] * xin) @ H for j in range(J)]
        u = [(b[j] * t1[j]) @ H for j in range(J)]
        pre = torch.cat([a[j] * u[j] for j in range(J)], dim=1)[:, :n_cols]
        if bias is not None:
            pre = pre + bias[:n_cols]
        mask = None
        if relu_out:
            if bwd and exact:
                t["y"][sl] = stored(torch.relu(pre.detach()), "y")
            mask = ((t["y"][sl] if bwd else pre.detach()) > 0).double()
        yv = pre * mask if relu_out else pre
        if not bwd:
            if rows_too:
                ref["out"][sl] = stored(yv.detach(), "y")
            continue
        gy = t["gy"][sl].double()
        leaves = [a, b, c] + ([bias] if "gbias" in ref else []) + ([xs] if need_x else [])
        grads = torch.autograd.grad((yv * gy).sum(), leaves)
        ref["ga"] += grads[0]
        ref["gb"][:, s] = grads[1]
        ref["gc"] += grads[2]
        if "gbias" in ref:
            ref["gbias"] += grads[3]
        if rows_too and need_x:
            ref["gx"][sl] = stored(grads[-1], "grad_x")
        if not exact:
            continue
        # A64: the sums of the absolute values of each parameter gradient's terms, and of the last transform's inputs
        with torch.no_grad():
            g = gy * mask if relu_out else gy
            if n_cols < J * D:
                g = torch.nn.functional.pad(g, (0, J * D - n_cols))
            for j in range(J):
                gj = g[:, j * D:(j + 1) * D]
                v = (a[j] * gj) @ H
                w = (b[j] * v) @ H
                A["ga"][j] += (gj.abs() * u[j].abs()).sum(dim=0)
                A["gb"][j, s] = (v.abs() * t1[j].abs()).sum(dim=0)
                A["gc"][j] += (w.abs() * xin.abs()).sum(dim=0)
                chain = max(chain, J * float(v.abs().sum(dim=1).max()))
            if "gbias" in A:
                A["gbias"] += g.abs().sum(dim=0)
    if exact and bwd:
        worst = {k: float(v.max()) for k, v in A.items()}
        print(f"slab {case['id']}: rows {S * B}, A64 " + " ".join(f"{k}={v:.2e}" for k, v in worst.items()) + f" chain={chain:.2e}")
        assert max(worst.values()) < LIMIT and chain < LIMIT, ("a partial sum could leave the exact float32 integers", worst, chain)
    return ref


def _equal(got, want, what):
    """Values after + 0.0, no tolerance: the reference is an exact integer (rounded once for 16-bit storage)."""
    want = want.to(got.dtype)
    assert got.shape == want.shape, (what, got.shape, want.shape)
    bad = (got + 0.0) != (want + 0.0)
    if bool(bad.any()):
        where = bad.reshape(bad.size(0), -1).any(dim=1).nonzero().flatten()
        first = int(where[0])
        raise AssertionError((what, f"{int(bad.sum())} of {bad.numel()} elements differ, {where.numel()} rows, the first row {first}",
                              got.reshape(bad.size(0), -1)[first][:8].tolist(), want.reshape(bad.size(0), -1)[first][:8].tolist()))


# ---- (a)
@cases
def test_integer_operands_exact(case, hip_lib):
    S, B, J, D, n_cols, ld = _dims(case)
    t = _operands(case, integer=True)
    ref = _reference(case, t, exact=True)
    before = {k: v.clone() for k, v in t.items() if k not in ("gy", "y")}
    outs, bufs, kernel = _run(case, t)
    la = _common(case, outs, bufs, kernel)
    assert la.nt == (case["regime"] == "stream") and la.tiles_per_wave >= (3 if case["regime"] == "walk" else 2)
    assert set(outs) == set(ref), (sorted(outs), sorted(ref))
    for k, v in before.items():
        assert torch.equal(_raw(v), _raw(t[k])), (k, "an input changed")
    for name in sorted(outs):
        if name in SUMS:
            assert torch.equal(ref[name].float().double(), ref[name])
        _equal(outs[name], ref[name], (case["id"], name))
    if "gbias" in outs:                                      # +0.0 exactly from n_cols on
        assert torch.equal(_raw(outs["gbias"][n_cols:]), torch.zeros(J * D - n_cols, dtype=torch.int32, device=DEV))
    again, bufs2, kernel2 = _run(case, t)
    assert kernel2 == kernel
    for name in outs:
        assert torch.equal(_raw(outs[name]), _raw(again[name])), (name, "the second call gives other bits")


# ---- (b)
def _sliced(case, t):
    """The case through one-tile launches: per sample, rows in pieces of at most one_tile_rows.  Returns the row outputs put
    together and the parameter gradients added in float32, in launch order."""
    S, B, J, D, n_cols, ld = _dims(case)
    per = st.one_tile_rows(case["log2d"])
    full, calls = {}, 0
    for s in range(S):
        for r0 in range(0, B, per):
            r1 = min(B, r0 + per)
            sub = dict(case, S=1, B=r1 - r0)
            la = st.launch(sub)
            assert la.nt is False and la.tiles_per_wave == 1, (sub, la)
            outs, bufs, kernel = _run(case, t, s=s, r0=r0, r1=r1)
            _common(case, outs, bufs, kernel, sub=sub)
            calls += 1
            for name, v in outs.items():
                if name in ROW_OUTPUTS:
                    full.setdefault(name, torch.empty(S * B, v.size(1), device=DEV, dtype=v.dtype))[s * B + r0:s * B + r1] = v
                elif name == "gb":
                    full.setdefault(name, torch.zeros(J, S, D, device=DEV))[:, s] += v[:, 0]
                else:
                    full[name] = full[name] + v if name in full else v.clone()
    return full, calls


def _ratio(got, ref):
    return float((got.double() - ref).abs().max()) / float(ref.abs().max())


def _poisoned(case, t):
    """The operands with +-inf and NaN in two rows of one slab -- the first row of wave 0's first tile and the first of its
    second tile -- of x and, for a backward entry, of grad_y as well (grad_x depends on grad_y alone)."""
    S, B, J, D, n_cols, ld = _dims(case)
    step = 4 * st.fused_bwd_tile_rows(case["log2d"])
    assert st.fused_bwd_geom(S, B, case["log2d"])[1] > step
    t = dict(t, x=t["x"].clone())
    planted = [(t["x"], 0 if case["shared"] else B, D)]      # sample 1's first slab (every sample's, for a shared x)
    if "gy" in t:
        t["gy_full"] = t["gy_full"].clone()
        t["gy"] = t["gy_full"][:, :n_cols]
        planted.append((t["gy"], B, n_cols))
    for v, base, width in planted:
        v[base, 3], v[base, width - 2] = float("inf"), float("-inf")
        v[base + step, 0], v[base + step, width // 2] = float("nan"), float("inf")
    return t


@cases
def test_gaussian_operands_against_one_tile_slices(case, hip_lib):
    S, B, J, D, n_cols, ld = _dims(case)
    e = case["entry"]
    t = _operands(case, integer=False)
    if "y" in t:                                             # the forward launch's y: the mask relu_out reads
        _hip.fused_shs_stacked_layer(t["x"], t["a"], t["b"], t["c"], S, B, bias=t["bias"], n_cols=n_cols, relu_in=case["relu_in"],
                                     relu_out=True, shared=case["shared"], out=t["y"])
    outs, bufs, kernel = _run(case, t)
    _common(case, outs, bufs, kernel)
    want, calls = _sliced(case, t)
    assert set(want) == set(outs) and calls >= S
    for name in ROW_OUTPUTS:
        if name in outs:
            assert bool(torch.isfinite(want[name]).all()), name
            _assert_same(outs[name], want[name])
    if e.endswith("_bwd"):
        ref = _reference(case, t, exact=False, rows_too=False)
        ratios = {name: (_ratio(outs[name], ref[name]), _ratio(want[name], ref[name])) for name in SUMS if name in outs}
        print(f"slab {case['id']}: rows {S * B}, {calls} slices, ratios (launch / slices): " +
              " ".join(f"{k}={v[0]:.2e}/{v[1]:.2e}" for k, v in ratios.items()))
        for name, (new, old) in ratios.items():
            if old > BOUND:
                print(f"slab {case['id']}: WAIVED {name}: the sliced route itself misses the bound ({old:.2e}); the launch gives {new:.2e}")
                continue
            assert new <= BOUND, (case["id"], name, new, old)
    if case["poison"]:
        t = _poisoned(case, t)
        outs, bufs, kernel = _run(case, t)
        _common(case, outs, bufs, kernel)
        want, _ = _sliced(case, t)
        for name in ROW_OUTPUTS:
            if name in outs:
                assert bool(torch.isnan(want[name]).any()) and bool(torch.isfinite(want[name]).any()), name
                _assert_same(outs[name], want[name])
