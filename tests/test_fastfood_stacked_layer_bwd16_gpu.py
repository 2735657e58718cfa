"""The one-launch backward of the rectangular fastfood layer with its epilogue on 16-bit activations, on the GPU
(whvi_fused_shs_stacked_layer_bwd_f16 / _bf16, ``FastfoodStackedLayer16Function(..., fused_backward=True, fused_backward16=True,
fused_epilogue_backward16=True)``).

The reference for ``grad_x, grad_a, grad_b, grad_c`` is the composed route called by hand -- ``threshold_backward`` in 16 bits,
``F.pad`` to ``J * D`` columns, ``torch.relu(x)``, ``_hip.fused_shs_stacked_bwd16``, ``threshold_backward`` on ``grad_x`` --
compared bit for bit (``torch.equal``; with non-finite inputs NaN positions and all other values).  The reference for
``grad_bias`` is the float64 column sum of the masked 16-bit gradient, within ``1e-5 * max|ref64|`` (the bound
tests/test_fastfood_stacked_layer_bwd_gpu.py and tests/test_fastfood_stacked_layer16_gpu.py hold this sum to); it is exactly
``+0.0`` from ``n_cols`` on.  Then non-finite inputs, every shipped instantiation past one tile per wave (cached and streaming,
integer operands against float64 exactly and Gaussian operands against the composed route), the Function's routing, the Module,
a network, one graph capture and the allocator's peak."""
import pytest
import torch
import torch.nn as nn
import torch.nn.functional as F

import test_slab_table_gpu as sg
from test_fastfood_stacked16_gpu import _operands
from test_fastfood_stacked_host import MODE, make_layer
from test_fused_bwd16_gpu import TYPE_NAME, _assert_same

import layer_bwd16_table as tb  # noqa: E402  (tools/ is on sys.path once test_slab_table_gpu is imported)

pytestmark = pytest.mark.gpu

DEV = "cuda"
BOUND = 1e-5
NAN = float("nan")
DTYPES = (torch.float16, torch.bfloat16)
SENTINEL = -776.0                                                 # exact in both storage types
GUARD = 2048                                                      # elements on each side of grad_x
SHAPES = ((1, 1), (3, 5), (2, 777), (4, 64))
SHIPPED = [(log2d, J) for log2d in range(6, 11) for J in (2, 3, 4)] + [(11, 2)]
KERNEL = "fused_layer_bwd16_kernel"
K16 = {6: 2, 7: 2, 8: 2, 9: 2, 10: 2, 11: 4}
dtypes = pytest.mark.parametrize("dtype", DTYPES, ids=("f16", "bf16"))
FLAGS = ("keep_half", "fused_epilogue", "fused_epilogue16", "fused_backward", "fused_backward16", "fused_epilogue_backward16")


def _pitched(rows, n_cols, ld, dtype):
    """``(rows, n_cols)`` view at pitch ``ld`` inside a NaN-filled buffer: the gap columns and the surroundings hold NaN."""
    big = torch.full((GUARD + rows * ld + GUARD,), NAN, dtype=dtype, device=DEV)
    return big[GUARD:GUARD + rows * ld].view(rows, ld)[:, :n_cols]


def _inputs(dtype, log2d, J, S, B, shared, n_cols, ld, relu_in=True, relu_out=True, seed=0):
    """``x, a, b, c, grad_y, y``: ``grad_y`` and ``y`` slices of NaN-filled buffers, ``y`` written by the 16-bit forward launch."""
    from whvi_amd import _hip
    D = 1 << log2d
    x, a, b, c = _operands(dtype, log2d, J, S, B, shared, DEV, seed=seed)
    bias = torch.randn(J * D, generator=torch.Generator().manual_seed(7 + log2d + J + seed)).to(DEV)
    gy = _pitched(S * B, n_cols, ld, dtype)
    gy.copy_(torch.randn(S * B, n_cols, generator=torch.Generator().manual_seed(11 * log2d + J + S + B + seed)).to(dtype).to(DEV))
    y = _hip.fused_shs_stacked_layer16(x, a, b, c, S, B, bias=bias, n_cols=n_cols, relu_in=relu_in, relu_out=relu_out,
                                       shared=shared, out=_pitched(S * B, n_cols, ld, dtype))
    return x, a, b, c, gy, y


def _reference(gy, y, x, a, b, c, S, B, shared, relu_in, relu_out, need_x):
    """The composed route by hand: ``(grad_x | None, grad_a, grad_b, grad_c, masked zero-padded 16-bit g)``."""
    from whvi_amd import _hip
    J, D = a.shape
    g = (torch.ops.aten.threshold_backward(gy, y, 0) if relu_out else gy).contiguous()
    if g.size(1) < J * D:
        g = F.pad(g, (0, J * D - g.size(1)))
    xin = torch.relu(x) if relu_in else x
    gx, ga, gb, gc = _hip.fused_shs_stacked_bwd16(g, xin, a, b, c, S, B, shared=shared, need_x=need_x)
    if relu_in and gx is not None:
        gx = torch.ops.aten.threshold_backward(gx, xin, 0)
    return gx, ga, gb, gc, g


def _launch(gy, y, x, a, b, c, S, B, shared, relu_in, relu_out, need_x, need_bias):
    """The new call, ``grad_x`` written into a guarded slice of a sentinel-filled buffer; the guards must be intact."""
    from whvi_amd import _hip
    rows, D = S * B, a.size(1)
    big = torch.full((GUARD + rows * D + GUARD,), SENTINEL, dtype=x.dtype, device=DEV)
    dst = big[GUARD:GUARD + rows * D].view(rows, D)
    _hip.fwht_rows(torch.zeros(1, 4, device=DEV))                           # (another kernel's name in the note)
    out = _hip.fused_shs_stacked_layer_bwd16(gy, y if relu_out else None, x, a, b, c, S, B, n_cols=gy.size(1), relu_in=relu_in,
                                             relu_out=relu_out, shared=shared, need_x=need_x, need_bias=need_bias,
                                             grad_x=dst if need_x else None)
    assert bool((big[:GUARD] == SENTINEL).all()) and bool((big[GUARD + rows * D:] == SENTINEL).all()), "a guard was written"
    if need_x:
        assert out[0].data_ptr() == dst.data_ptr() and out[0].dtype == x.dtype
    else:
        assert out[0] is None and bool((dst == SENTINEL).all())
    assert all(t.dtype == torch.float32 for t in out[1:] if t is not None)
    assert (out[4] is not None) == need_bias
    return out


def _check_bias(got, g, n_cols, what):
    ref = g.double().sum(dim=0)
    ratio = float((got.double() - ref).abs().max()) / float(ref.abs().max())
    assert got.shape == ref.shape and got.dtype == torch.float32
    assert torch.equal(got[n_cols:].view(torch.int32), torch.zeros_like(got[n_cols:]).view(torch.int32)), what     # +0.0 exactly
    assert ratio <= BOUND, (what, ratio)
    return ratio


def _bits(t):
    return t.view(torch.int32 if t.dtype == torch.float32 else torch.int16)


# ---- 1. the raw call -----------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("log2d,J", SHIPPED)
@dtypes
def test_raw_call_bit_equal_to_the_composed_route(dtype, log2d, J, hip_lib):
    from whvi_amd import _hip
    D = 1 << log2d
    worst = 0.0
    assert _hip.fused_shs_stacked_layer_bwd16_supported(dtype, D, J, True)
    n_cols = (J - 1) * D + D // 2 + 8
    for S, B in SHAPES:
        for shared in (False, True):
            need_x = not shared
            x, a, b, c, gy, y = _inputs(dtype, log2d, J, S, B, shared, n_cols, n_cols + 16)
            assert gy.stride(0) == y.stride(0) == n_cols + 16
            gy0, y0, x0 = gy.clone(), y.clone(), x.clone()
            got = _launch(gy, y, x, a, b, c, S, B, shared, True, True, need_x, True)
            assert _hip.last_kernel() == f"whvi::{KERNEL}<{TYPE_NAME[dtype]}, {log2d}, {K16[log2d]}, {J}, true, false>"
            for u, v in ((gy, gy0), (y, y0), (x, x0)):
                assert torch.equal(_bits(u), _bits(v)), "an input changed"
            want = _reference(gy, y, x, a, b, c, S, B, shared, True, True, need_x)
            assert bool(torch.isfinite(want[4]).all()) and bool((want[4] == 0).any()) and bool((want[4] != 0).any())
            for name, u, v in zip(("grad_x", "grad_a", "grad_b", "grad_c"), got, want):
                assert (u is None and v is None) or torch.equal(u, v), (name, J, S, B, shared)
            worst = max(worst, _check_bias(got[4], want[4], n_cols, (J, S, B, shared)))
            again = _launch(gy, y, x, a, b, c, S, B, shared, True, True, need_x, True)
            for u, v in zip(got, again):
                assert (u is None and v is None) or torch.equal(_bits(u), _bits(v))
            if (S, B) != (3, 5):
                continue
            for cols in (J * D, J * D - 8, (J - 1) * D + 8):
                for relu_in in (False, True):
                    for relu_out in (False, True):
                        x, a, b, c, gy, y = _inputs(dtype, log2d, J, S, B, shared, cols, cols, relu_in, relu_out)
                        for with_x in ((False, True) if not shared else (False,)):
                            want = _reference(gy, y, x, a, b, c, S, B, shared, relu_in, relu_out, with_x)
                            for need_bias in (False, True):
                                got = _launch(gy, y, x, a, b, c, S, B, shared, relu_in, relu_out, with_x, need_bias)
                                what = (J, cols, relu_in, relu_out, with_x, need_bias, shared)
                                assert f"{KERNEL}<" in _hip.last_kernel(), what
                                assert f"{J}, {'true' if need_bias else 'false'}, false>" in _hip.last_kernel(), what
                                for u, v in zip(got[:4], want):
                                    assert (u is None and v is None) or torch.equal(u, v), what
                                if need_bias:
                                    worst = max(worst, _check_bias(got[4], want[4], cols, what))
            # no option, no bias, n_cols == ld == J D: the 16-bit launch without an epilogue
            x, a, b, c, gy, y = _inputs(dtype, log2d, J, S, B, shared, J * D, J * D, False, False)
            got = _hip.fused_shs_stacked_layer_bwd16(gy, None, x, a, b, c, S, B, shared=shared, need_x=need_x)
            want = _hip.fused_shs_stacked_bwd16(gy, x, a, b, c, S, B, shared=shared, need_x=need_x)
            assert got[4] is None
            for u, v in zip(got[:4], want):
                assert (u is None and v is None) or torch.equal(_bits(u), _bits(v))
    print(f"layer_bwd16 {TYPE_NAME[dtype]} log2(D) = {log2d} J = {J}: worst bias gradient error / max|ref64| = {worst:.3e}")


@dtypes
def test_back_to_back_16_bit_buffers_are_no_overlap(dtype, hip_lib):
    """grad_y, y, x and grad_x directly behind one another: extents counted at 4 bytes an element would reach into the next."""
    from whvi_amd import _hip
    log2d, J, S, B = 9, 2, 2, 2
    D, rows = 1 << log2d, S * B
    n_cols, ld = 1000, 1008
    x, a, b, c, gy, y = _inputs(dtype, log2d, J, S, B, False, n_cols, ld)
    ny, nx = rows * ld, rows * D
    buf = torch.zeros(2 * ny + 2 * nx, dtype=dtype, device=DEV)
    gy1, y1 = buf[:ny].view(rows, ld)[:, :n_cols], buf[ny:2 * ny].view(rows, ld)[:, :n_cols]
    x1, gx1 = buf[2 * ny:2 * ny + nx].view(rows, D), buf[2 * ny + nx:].view(rows, D)
    gy1.copy_(gy)
    y1.copy_(y)
    x1.copy_(x)
    want = _hip.fused_shs_stacked_layer_bwd16(gy, y, x, a, b, c, S, B, relu_in=True, relu_out=True, need_bias=True)
    got = _hip.fused_shs_stacked_layer_bwd16(gy1, y1, x1, a, b, c, S, B, relu_in=True, relu_out=True, need_bias=True, grad_x=gx1)
    assert got[0].data_ptr() == gx1.data_ptr()
    for u, v in zip(got, want):
        assert torch.equal(_bits(u), _bits(v))


# ---- 2. non-finite inputs ------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("log2d", [6, 9, 10, 11])
@dtypes
def test_non_finite_inputs(dtype, log2d, hip_lib):
    D = 1 << log2d
    J, S, B = (2 if log2d == 11 else 3), 3, 5
    n_cols = (J - 1) * D + D // 2 + 8
    inf = float("inf")
    x, a, b, c, gy, y = _inputs(dtype, log2d, J, S, B, False, n_cols, n_cols + 16, seed=7)
    rows = S * B
    x[1, 3], x[1, D - 2], x[rows - 1, 0], x[rows - 1, D // 2] = inf, -inf, NAN, inf
    gy[2, 5], gy[2, n_cols - 1], gy[rows - 2, 0], gy[rows - 2, D + 1] = inf, -inf, NAN, inf
    y[4, 7], y[4, 9], y[rows - 2, 0], y[2, 5] = NAN, -0.0, -0.0, 1.0                 # (a NaN y passes grad_y; -0.0 masks it)
    got = _launch(gy, y, x, a, b, c, S, B, False, True, True, True, True)
    want = _reference(gy, y, x, a, b, c, S, B, False, True, True, True)
    g = want[4]
    assert float(g[4, 7]) == float(gy[4, 7]) and float(g[4, 9]) == 0.0 and float(g[rows - 2, 0]) == 0.0 and float(g[2, 5]) == inf
    assert bool(torch.isnan(want[0]).any()) and bool(torch.isfinite(want[0]).any())
    for name, u, v in zip(("grad_x", "grad_a", "grad_b", "grad_c"), got, want):
        _assert_same(u, v, name)
    ref = g.double().sum(dim=0)
    assert torch.equal(torch.isnan(got[4]), torch.isnan(ref)) and torch.equal(torch.isinf(got[4]), torch.isinf(ref))
    fin = torch.isfinite(ref)
    assert float((got[4].double() - ref)[fin].abs().max()) <= BOUND * float(ref[fin].abs().max())
    again = _launch(gy, y, x, a, b, c, S, B, False, True, True, True, True)
    for name, u, v in zip(("grad_x", "grad_a", "grad_b", "grad_c", "grad_bias"), got, again):
        _assert_same(u, v, name)


# ---- 3. every instantiation past one tile per wave -----------------------------------------------------------------------------
cases = pytest.mark.parametrize("case", tb.CASES, ids=lambda c: c["id"])


def _as_slab(case):
    """The case as tests/test_slab_table_gpu.py's float64 reference reads it: the layer's backward entry."""
    return dict(case, entry="fused_shs_stacked_layer_bwd")


def _table_operands(case, integer):
    S, B, J, D = case["S"], case["B"], case["J"], 1 << case["log2d"]
    n_cols, ld = case["n_cols"], case["ld"]
    dt, rows = sg.DT[case["dtype"]], S * B
    g = torch.Generator(device=DEV).manual_seed(7919 * tb.CASES.index(case) + (1 if integer else 2))
    xr = B if case["shared"] else rows
    t = {}
    if integer:
        t["x"] = sg._three_per_row(xr, D, g, dt)
        t["a"], t["c"], t["b"] = sg._pm1((J, D), g), sg._pm1((J, D), g), sg._pm1((J, S, D), g)
        t["bias"] = torch.randint(-3, 4, (J * D,), device=DEV, generator=g).float()
    else:
        scale = 1.0 / D ** 0.5
        t["x"] = torch.randn(xr, D, device=DEV, generator=g).to(dt)
        t["a"] = torch.randn(J, D, device=DEV, generator=g) * scale
        t["b"] = torch.randn(J, S, D, device=DEV, generator=g) * scale
        t["c"] = torch.randn(J, D, device=DEV, generator=g)
        t["bias"] = torch.randn(J * D, device=DEV, generator=g)
    t["gy_full"], t["gy"] = sg._pitched(rows, n_cols, ld, dt)
    if integer:
        t["gy"].copy_(sg._three_per_row(rows, n_cols, g, dt))     # |grad_x| <= 3 D: finite in fp16
    else:
        t["gy"].copy_(torch.randn(rows, n_cols, device=DEV, generator=g).to(dt))
    if case["relu_out"]:
        t["y_full"], t["y"] = sg._pitched(rows, n_cols, ld, dt)
    return t


def _run(case, t):
    """The entry through the C ABI on the case's operands into guarded, prefilled outputs.  Returns (outputs by name, [(buffer,
    guarded view)], the kernel whvi_last_kernel names)."""
    from whvi_amd import _hip
    S, B, J, L = case["S"], case["B"], case["J"], case["log2d"]
    D, dt, shared = 1 << L, sg.DT[case["dtype"]], case["shared"]
    rows = S * B
    bufs, outs = [], {}

    def new(name, shape):
        buf, view = sg._new(shape, dt if name == "gx" else torch.float32)
        bufs.append((buf, view))
        outs[name] = view
        return view

    gx = new("gx", (rows, D)) if case["need_x"] else None
    ga, gb, gc = new("ga", (J, D)), new("gb", (J, S, D)), new("gc", (J, D))
    gbias = new("gbias", (J * D,)) if case["bias"] else None
    lib = _hip.lib()
    n = int(lib.whvi_fused_shs_stacked_layer_bwd_workspace(S, B, L, J, int(case["bias"])))
    work = torch.empty((max(n, 16),), dtype=torch.uint8, device=DEV)
    flags = ((_hip.FUSED_SRC_SHARED if shared else 0) | (_hip.FUSED_RELU_IN if case["relu_in"] else 0)
             | (_hip.FUSED_RELU_OUT if case["relu_out"] else 0))
    fn = getattr(lib, "whvi_fused_shs_stacked_layer_bwd_" + tb.SUFFIX[case["dtype"]])
    rc = fn(None if gx is None else gx.data_ptr(), ga.data_ptr(), gb.data_ptr(), gc.data_ptr(),
            None if gbias is None else gbias.data_ptr(), work.data_ptr(), t["gy"].data_ptr(),
            t["y"].data_ptr() if case["relu_out"] else None, t["x"].data_ptr(), t["a"].data_ptr(), t["b"].data_ptr(),
            t["c"].data_ptr(), J, S, B, L, case["n_cols"], case["ld"], flags, None)
    assert rc == 0, _hip.last_error()
    kernel = _hip.last_kernel()
    torch.cuda.synchronize()
    return outs, bufs, kernel


def _common(case, outs, bufs, kernel):
    """whvi_last_kernel is the mirror's symbol; every output element written; margins intact."""
    want = tb.launch(case)
    assert kernel == want.symbol, (kernel, want.symbol)
    assert kernel.endswith("true>" if want.nt else "false>")
    for buf, view in bufs:
        assert sg._margins_intact(buf, view), "a byte outside an output changed"
    for name, view in outs.items():
        assert sg._holes(view) == 0, (name, "elements never written", sg._holes(view))
    return want


@cases
def test_integer_operands_exact(case, hip_lib):
    """Small-integer operands: every sum of absolute terms stays below 2^24 (asserted and printed by the reference), so all five
    gradients equal float64 exactly -- grad_x as ``ref64.to(dtype)`` -- whatever the order of the bias sum."""
    J, D, n_cols = case["J"], 1 << case["log2d"], case["n_cols"]
    t = _table_operands(case, integer=True)
    ref = sg._reference(_as_slab(case), t, exact=True)           # (writes the reference's y where relu_out reads it)
    before = {k: v.clone() for k, v in t.items()}
    outs, bufs, kernel = _run(case, t)
    la = _common(case, outs, bufs, kernel)
    assert la.nt == (case["regime"] == "stream") and la.tiles_per_wave >= (3 if case["regime"] == "walk" else 2)
    assert set(outs) == set(ref), (sorted(outs), sorted(ref))
    for k, v in before.items():
        assert torch.equal(sg._raw(v), sg._raw(t[k])), (k, "an input changed")
    for name in sorted(outs):
        if name in sg.SUMS:
            assert torch.equal(ref[name].float().double(), ref[name])
        sg._equal(outs[name], ref[name], (case["id"], name))
    if "gbias" in outs:                                          # +0.0 exactly from n_cols on
        assert torch.equal(sg._raw(outs["gbias"][n_cols:]), torch.zeros(J * D - n_cols, dtype=torch.int32, device=DEV))
    again, _, kernel2 = _run(case, t)
    assert kernel2 == kernel
    for name in outs:
        assert torch.equal(sg._raw(outs[name]), sg._raw(again[name])), (name, "the second call gives other bits")


@cases
def test_gaussian_operands_against_the_composed_route(case, hip_lib):
    from whvi_amd import _hip
    S, B, J, D, n_cols = case["S"], case["B"], case["J"], 1 << case["log2d"], case["n_cols"]
    t = _table_operands(case, integer=False)
    if case["relu_out"]:                                         # the 16-bit forward launch's y: the mask relu_out reads
        _hip.fused_shs_stacked_layer16(t["x"], t["a"], t["b"], t["c"], S, B, bias=t["bias"], n_cols=n_cols, relu_in=case["relu_in"],
                                       relu_out=True, shared=case["shared"], out=t["y"])
    if case["poison"]:
        step = 4 * sg.st.fused_bwd_tile_rows(case["log2d"])
        for v, base, width in ((t["x"], 0 if case["shared"] else B, D), (t["gy"], B, n_cols)):
            v[base, 3], v[base, width - 2] = float("inf"), float("-inf")
            v[base + step, 0], v[base + step, width // 2] = NAN, float("inf")
    outs, bufs, kernel = _run(case, t)
    _common(case, outs, bufs, kernel)
    want = _reference(t["gy"], t.get("y"), t["x"], t["a"], t["b"], t["c"], S, B, case["shared"], case["relu_in"],
                      case["relu_out"], case["need_x"])
    assert ("gx" in outs) == case["need_x"] == (want[0] is not None)
    for name, v in zip(("gx", "ga", "gb", "gc"), want):
        if v is None:
            continue
        if case["poison"]:
            _assert_same(outs[name], v, (case["id"], name))
        else:
            assert bool(torch.isfinite(v).all()), name
            assert torch.equal(outs[name], v), (case["id"], name)
    if case["bias"]:
        ref = want[4].double().sum(dim=0)
        got = outs["gbias"]
        assert torch.equal(sg._raw(got[n_cols:]), torch.zeros(J * D - n_cols, dtype=torch.int32, device=DEV))
        fin = torch.isfinite(ref)
        assert torch.equal(torch.isnan(got), torch.isnan(ref)) and torch.equal(torch.isinf(got), torch.isinf(ref))
        ratio = float((got.double() - ref)[fin].abs().max()) / float(ref[fin].abs().max())
        print(f"layer_bwd16 table {case['id']}: rows {S * B}, bias gradient error / max|ref64| = {ratio:.3e}")
        assert ratio <= BOUND, (case["id"], ratio)


# ---- 4. routing ----------------------------------------------------------------------------------------------------------------
def _set_flags(sub, **off):
    for name in FLAGS:
        setattr(sub, name, name not in off)


def _backward(layer, x, S, want_x=True, hook_on=None, relu_in=True, relu_out=True):
    """``(kernel named when the gradient of x -- or of hook_on -- is produced, y, x.grad, parameter gradients)`` of
    ``relu(layer(relu(x)))`` under seed 5 with the flags as they are set on the layer."""
    from whvi_amd import _hip
    seen = []
    x = x.detach().clone().requires_grad_(want_x)
    handle = (x if hook_on is None else hook_on).register_hook(lambda grad: seen.append(_hip.last_kernel()))
    layer.zero_grad()
    torch.manual_seed(5)
    _hip.fwht_rows(torch.zeros(1, 4, device=x.device))                      # (another kernel's name in this thread's note)
    y = layer.forward_mc(x, S, relu_in=relu_in, relu_out=relu_out)
    w = torch.randn(y.shape, generator=torch.Generator().manual_seed(6)).to(y)
    (y * w).sum().backward()
    handle.remove()
    assert len(seen) == 1, seen
    return seen[0], y.detach(), x.grad, [p.grad.clone() for p in layer.parameters() if p.grad is not None]


def _same(u, v):
    assert torch.equal(u[1], v[1])
    assert (u[2] is None and v[2] is None) or torch.equal(u[2], v[2])
    assert len(u[3]) == len(v[3])
    for p, q in zip(u[3], v[3]):
        assert torch.equal(p, q)


@dtypes
def test_routing_names_the_kernel(dtype, hip_lib):
    S, B = 3, 7
    gen = torch.Generator().manual_seed(9)
    for n_in, n_out, tag in ((128, 512, "7, 2, 4, true, false>"), (128, 200, "7, 2, 2, true, false>")):
        layer = make_layer(n_in, n_out, bias=True).to(DEV)
        sub = layer.weight_submodule
        _set_flags(sub)
        s1 = sub.weight_matrices[0].s1
        x3 = torch.randn(S, B, n_in, generator=gen).to(dtype).to(DEV)
        x2 = torch.randn(B, n_in, generator=gen).to(dtype).to(DEV)
        assert f"{KERNEL}<{TYPE_NAME[dtype]}, {tag}" in _backward(layer, x3, S)[0]
        # a 2-D input that is data takes the launch
        assert f"{KERNEL}<{TYPE_NAME[dtype]}, {tag}" in _backward(layer, x2, S, want_x=False, hook_on=s1)[0]


def test_routing_refusals_keep_the_route(hip_lib):
    dtype = torch.float16
    S, B = 3, 7
    gen = torch.Generator().manual_seed(9)
    for n_in, n_out in ((128, 512), (128, 200)):
        layer = make_layer(n_in, n_out, bias=True).to(DEV)
        sub = layer.weight_submodule
        x3 = torch.randn(S, B, n_in, generator=gen).to(dtype).to(DEV)
        x2 = torch.randn(B, n_in, generator=gen).to(dtype).to(DEV)
        # a 2-D input that wants a gradient keeps the composed backward
        _set_flags(sub)
        off = _backward(layer, x2, S)
        assert KERNEL not in off[0]
        _set_flags(sub, fused_epilogue_backward16=False)
        _same(off, _backward(layer, x2, S))
        # any one of the six flags off
        for name in FLAGS:
            _set_flags(sub, **{name: False})
            got = _backward(layer, x3, S)
            assert KERNEL not in got[0], name
            _set_flags(sub, **{name: False, "fused_epilogue_backward16": False})
            _same(got, _backward(layer, x3, S))
    # a bias and nothing else to fold (no ReLU, n_out == D_out): the composed backward
    layer = make_layer(128, 512, bias=True).to(DEV)
    sub = layer.weight_submodule
    x3 = torch.randn(S, B, 128, generator=gen).to(dtype).to(DEV)
    _set_flags(sub)
    got = _backward(layer, x3, S, relu_in=False, relu_out=False)
    assert KERNEL not in got[0]
    _set_flags(sub, fused_epilogue_backward16=False)
    _same(got, _backward(layer, x3, S, relu_in=False, relu_out=False))
    # refused with every flag on: five blocks of 512, one block, float32 input, 16-bit parameters
    for n_in, n_out, x_dtype, half_params in ((512, 2560, dtype, False), (128, 128, dtype, False), (128, 512, torch.float32, False),
                                              (128, 512, dtype, True)):
        layer = make_layer(n_in, n_out, bias=True).to(DEV)
        if half_params:
            layer = layer.half()
        sub = layer.weight_submodule
        assert sub.stack == -(-n_out // n_in)
        x = torch.randn(S, B, n_in, generator=gen).to(x_dtype).to(DEV)
        _set_flags(sub)
        got = _backward(layer, x, S)
        assert KERNEL not in got[0], (n_in, n_out, x_dtype, half_params)
        _set_flags(sub, fused_epilogue_backward16=False)
        _same(got, _backward(layer, x, S))


def test_routing_keeps_the_cached_full_grid_case_composed(hip_lib):
    """(128, 512) at S = 64, B = 1000 -- four blocks, the bias sum, 1024 blocks of the grid, 164 MB: the shape at which the launch
    measured slower than the composed backward.  The kernel is not named and the bits are the flag-off route's; the
    same layer without its bias wanted (frozen) takes the launch."""
    S, B = 64, 1000
    layer = make_layer(128, 512, bias=True).to(DEV)
    sub = layer.weight_submodule
    x = torch.randn(S, B, 128, generator=torch.Generator().manual_seed(17)).half().to(DEV)
    _set_flags(sub)
    got = _backward(layer, x, S)
    assert KERNEL not in got[0]
    _set_flags(sub, fused_epilogue_backward16=False)
    _same(got, _backward(layer, x, S))
    _set_flags(sub)
    sub.bias.requires_grad_(False)
    assert f"{KERNEL}<__half, 7, 2, 4, false, false>" in _backward(layer, x, S)[0]


@pytest.mark.parametrize("relu_out", [False, True])
@dtypes
def test_gradient_that_is_a_view_of_a_wider_one(dtype, relu_out, hip_lib):
    """``torch.cat`` behind the layer: autograd hands the backward a ``(S * B, 512)`` view with row stride 1024.  Without
    ``relu_out`` the launch reads it in place; with it the saved output has pitch 512 and the gradient is copied first.  Either
    way the launch runs and every gradient but the bias has the composed backward's bits (the bias: both routes are within
    ``BOUND`` of float64 at this shape, test_module_gradients, so within twice that of each other)."""
    from whvi_amd import _hip
    S, B = 3, 7
    gen = torch.Generator().manual_seed(13)
    layer = make_layer(128, 512, bias=True).to(DEV)
    sub = layer.weight_submodule
    x = torch.randn(S, B, 128, generator=gen).to(dtype).to(DEV)
    other = torch.randn(S, B, 512, generator=gen).to(dtype).to(DEV)
    w = torch.randn(S, B, 1024, generator=gen).to(dtype).to(DEV)
    out = {}
    for flag in (True, False):
        _set_flags(sub)
        sub.fused_epilogue_backward16 = flag
        xr = x.clone().requires_grad_()
        seen, strides = [], []
        xr.register_hook(lambda grad: seen.append(_hip.last_kernel()))
        layer.zero_grad()
        torch.manual_seed(5)
        _hip.fwht_rows(torch.zeros(1, 4, device=DEV))
        y = layer.forward_mc(xr, S, relu_in=True, relu_out=relu_out)
        y.register_hook(lambda grad: strides.append(grad.stride()))
        (torch.cat([y, other], dim=-1) * w).sum().backward()
        assert strides == [(B * 1024, 1024, 1)], strides
        assert (KERNEL in seen[0]) == flag, seen
        out[flag] = {"x": xr.grad, **{n: p.grad.clone() for n, p in layer.named_parameters()}}
    for n in out[True]:
        u, v = out[True][n], out[False][n]
        if n.endswith("bias"):
            assert float((u - v).abs().max()) <= 2 * BOUND * float(v.abs().max()), n
        else:
            assert torch.equal(u, v), n


# ---- 5. the Module -------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("n_in,n_out", [(128, 512), (128, 200), (100, 256), (1024, 4096)])
@dtypes
def test_module_gradients(dtype, n_in, n_out, hip_lib):
    """``x, s1, s2, g_mu, g_rho``: the bits of the route with only the new flag off.  The bias: max|got - ref64| <= 1e-5 *
    max|ref64| against the float64 column sum of the masked 16-bit gradient (``grad_y`` is ``w`` itself, the mask the output's)."""
    from whvi_amd import _hip
    S, B = 3, 65
    layer = make_layer(n_in, n_out, bias=True).to(DEV)
    sub = layer.weight_submodule
    names = [n for n, _ in sub.named_parameters()]
    x = torch.randn(S, B, n_in, generator=torch.Generator().manual_seed(8)).to(dtype).to(DEV)
    w = torch.randn(S, B, n_out, generator=torch.Generator().manual_seed(6)).to(dtype).to(DEV)
    grads = {}
    for flag in (False, True):
        _set_flags(sub)
        sub.fused_epilogue_backward16 = flag
        xr = x.clone().requires_grad_()
        seen = []
        xr.register_hook(lambda grad: seen.append(_hip.last_kernel()))
        torch.manual_seed(5)
        y = layer.forward_mc(xr, S, relu_in=True, relu_out=True)
        assert y.dtype == dtype
        grads[flag] = (y.detach(),) + torch.autograd.grad((y * w).sum(), [xr] + list(sub.parameters()))
        assert (KERNEL in seen[0]) == flag, seen
    assert torch.equal(grads[False][0], grads[True][0])
    for name, p, q in zip(["x"] + names, grads[False][1:], grads[True][1:]):
        assert p.shape == q.shape and p.dtype == q.dtype, name
        if name != "bias":
            assert torch.equal(p, q), name
    y = grads[True][0]
    g = torch.ops.aten.threshold_backward(w, y, 0)
    ref = F.pad(g.double().sum(dim=(0, 1)), (0, sub.D_out - n_out)).view(1, sub.D_out)
    got, off = grads[True][2 + names.index("bias")], grads[False][2 + names.index("bias")]
    ratio = float((got.double() - ref).abs().max()) / float(ref.abs().max())
    ratio_off = float((off.double() - ref).abs().max()) / float(ref.abs().max())
    print(f"layer_bwd16 module {TYPE_NAME[dtype]} ({n_in}, {n_out}): bias gradient error / max|ref64| = {ratio:.3e} "
          f"(the composed backward: {ratio_off:.3e})")
    assert got.shape == ref.shape == (1, sub.D_out) and got.dtype == torch.float32
    assert bool((got[0, n_out:] == 0).all())
    assert ratio <= BOUND


@dtypes
def test_network_one_training_step(dtype, hip_lib):
    """A three-layer 16-bit network (64 -> 128 -> 200 -> 8, ReLUs between) whose first two, rectangular layers take the launch:
    after one SGD step every gradient and every parameter but those two layers' biases has the bits of the network with
    ``fused_epilogue_backward16`` off."""
    from whvi_amd import _hip
    from whvi_amd.layers import WHVILinear
    from whvi_amd.networks import WHVIRegression
    S, B = 4, 33
    x = torch.randn(B, 64, generator=torch.Generator().manual_seed(1)).to(dtype).to(DEV)
    w = torch.randn(B, 8, S, generator=torch.Generator().manual_seed(2)).to(dtype).to(DEV)
    out = {}
    for flag in (False, True):
        torch.manual_seed(0)
        net = WHVIRegression([WHVILinear(64, 128, mode=MODE, bias=True), nn.ReLU(), WHVILinear(128, 200, mode=MODE, bias=True),
                              nn.ReLU(), WHVILinear(200, 8, mode=MODE, bias=False)], train_samples=S, eval_samples=S).to(DEV)
        subs = [m.weight_submodule for m in net.sequential if isinstance(m, WHVILinear)]
        assert len(subs) == 3 and all(type(s).__name__ == "WHVIFastfoodStackedMatrix" for s in subs)
        with torch.no_grad():
            for s in subs:                                        # parameters of order one, as make_layer's
                for m in s.weight_matrices:
                    m.g_mu.copy_(torch.randn(s.D_in, device=DEV) * 0.3)
                    m.s1.mul_(10.0)
                    m.s2.mul_(10.0)
                if s.bias is not None:
                    s.bias.copy_(torch.randn(1, s.D_out, device=DEV) * 0.1)
        for s in subs:
            _set_flags(s)
            s.fused_epilogue_backward16 = flag
        seen = []
        handle = subs[1].weight_matrices[0].s1.register_hook(lambda grad: seen.append(_hip.last_kernel()))
        opt = torch.optim.SGD(net.parameters(), lr=1e-3)
        opt.zero_grad()
        torch.manual_seed(3)
        y = net.forward_batched(x, S)
        assert y.shape == (B, 8, S) and y.dtype == dtype
        (y * w).sum().backward()
        handle.remove()
        assert len(seen) == 1 and (KERNEL in seen[0]) == flag, seen
        grads = {n: p.grad.clone() for n, p in net.named_parameters() if p.grad is not None}
        assert len(grads) == 4 * sum(s.stack for s in subs) + 2
        opt.step()
        biases = {n for n, p in net.named_parameters() if any(p is s.bias for s in subs[:2])}
        assert len(biases) == 2
        out[flag] = (y.detach(), grads, {n: p.detach().clone() for n, p in net.named_parameters()}, biases)
    assert bool(torch.isfinite(out[False][0].float()).all()) and torch.equal(out[False][0], out[True][0])
    assert out[False][1].keys() == out[True][1].keys() and len(out[True][1]) > 0
    skipped = 0
    for n in out[True][1]:
        if n in out[True][3]:                                          # (the launch's own summation order: test_module_gradients)
            skipped += 1
            continue
        assert torch.equal(out[False][1][n], out[True][1][n]), n
        assert torch.equal(out[False][2][n], out[True][2][n]), n
    assert skipped == 2


# ---- 6. graph capture and peak memory ------------------------------------------------------------------------------------------
def test_graph_capture_and_replay(hip_lib):
    from whvi_amd import _hip
    dtype, log2d, J, S, B = torch.float16, 10, 4, 2, 64               # the (1024, 4096) layer
    x, a, b, c, gy, y = _inputs(dtype, log2d, J, S, B, False, J << log2d, J << log2d)
    kw = dict(relu_in=True, relu_out=True, need_bias=True)
    eager = _hip.fused_shs_stacked_layer_bwd16(gy, y, x, a, b, c, S, B, **kw)
    want = _reference(gy, y, x, a, b, c, S, B, False, True, True, True)
    for u, v in zip(eager[:4], want):
        assert torch.equal(u, v)
    side = torch.cuda.Stream()
    side.wait_stream(torch.cuda.current_stream())
    with torch.cuda.stream(side):
        _hip.fused_shs_stacked_layer_bwd16(gy, y, x, a, b, c, S, B, **kw)
    torch.cuda.current_stream().wait_stream(side)
    graph = torch.cuda.CUDAGraph()
    with torch.cuda.graph(graph):
        captured = _hip.fused_shs_stacked_layer_bwd16(gy, y, x, a, b, c, S, B, **kw)
    for _ in range(2):
        for t in captured:
            t.zero_()
        graph.replay()
        torch.cuda.synchronize()
        for u, v in zip(captured, eager):
            assert torch.equal(_bits(u), _bits(v))


def test_peak_memory_of_the_backward(hip_lib):
    """D = 1024, J = 4, S = 8, B = 4096, float16, with a bias and both ReLUs: one (rows, D) activation is A = 64 MiB.  Above what
    is held before the backward the launch allocates grad_x, the workspace and the parameter gradients; the composed backward
    also holds the masked gradient (4 A), relu(x) and the unmasked grad_x."""
    from whvi_amd import _hip
    from whvi_amd.fastfood import FastfoodStackedLayer16Function
    D, J, S, B = 1024, 4, 8, 4096
    A = S * B * D * 2
    g = torch.Generator(device=DEV).manual_seed(3)
    x = torch.randn(S * B, D, device=DEV, generator=g).half()
    gy = torch.randn(S * B, J * D, device=DEV, generator=g).half()
    scale = 1.0 / D ** 0.5
    a, c = torch.randn(J, D, device=DEV, generator=g) * scale, torch.randn(J, D, device=DEV, generator=g)
    b = torch.randn(J, S, D, device=DEV, generator=g) * scale
    bias = torch.randn(1, J * D, device=DEV, generator=g)
    work = int(_hip.lib().whvi_fused_shs_stacked_layer_bwd_workspace(S, B, 10, J, 1))
    peaks = {}
    for flag in (True, False):
        leaves = [t.clone().requires_grad_() for t in (x, a, b, c, bias)]
        y = FastfoodStackedLayer16Function.apply(*leaves, J * D, True, True, S, B, False, True, True, flag)
        torch.cuda.synchronize()
        torch.cuda.reset_peak_memory_stats(DEV)
        held = torch.cuda.memory_allocated(DEV)
        y.backward(gy)
        torch.cuda.synchronize()
        peaks[flag] = torch.cuda.max_memory_allocated(DEV) - held
        del leaves, y
    print(f"layer_bwd16 memory: A = {A >> 20} MiB, workspace {work >> 20} MiB, peak launch {peaks[True] / A:.3f} A "
          f"({peaks[True] >> 20} MiB), composed {peaks[False] / A:.3f} A ({peaks[False] >> 20} MiB)")
    assert peaks[True] < peaks[False], peaks
