"""The rectangular fastfood layer on 16-bit activations with its epilogue in the one launch, on the GPU:
whvi_fused_shs_stacked_layer_f16 / _bf16 against the float32 layer launch on the exactly-upcast input, cast once --

    _hip.fused_shs_stacked_layer(x.float(), a, b, c, ..., bias, n_cols, relu_in, relu_out, shared).to(dtype)

-- with tests/test_fused16_gpu.py's ``_assert_same``: equal NaN positions, equal values after ``+ 0.0``, equal inf positions, no
tolerance (both storage types, every supported D, own and shared input, a pitch wider than n_cols inside a guarded buffer, every
combination of the three options, slabs walked past one tile per wave, the streaming instantiations, non-finite inputs,
repeatability); that the one rounding is closer to float64 than the separate passes' three; the Module's routing under
``keep_half`` + ``fused_epilogue`` + ``fused_epilogue16``; its gradients against the existing pieces called by hand (bit for bit)
and float64 (the bias); a network whose ReLU is folded; one graph capture and the allocator's peak.

Operands as in tests/test_fastfood_stacked16_gpu.py: ``x`` is seeded ``randn`` rounded to the dtype; ``a, b, c`` are float32
``randn`` with ``a`` and ``b`` scaled by 1 / sqrt(D), so that fp16 results stay finite; the bias is float32 ``randn``."""
import os
import sys

import pytest
import torch
import torch.nn as nn
import torch.nn.functional as F

from whvi_amd.layers import WHVILinear
from whvi_amd.networks import WHVIRegression

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, os.path.join(os.path.dirname(HERE), "tools"))
import slab_table as st  # noqa: E402
from test_fastfood_stacked16_gpu import DTYPES, GUARD, SENTINEL, _operands  # noqa: E402
from test_fastfood_stacked_host import MODE, make_layer  # noqa: E402
from test_fused16_gpu import _assert_same  # noqa: E402
from test_fused_bwd16_gpu import TYPE_NAME  # noqa: E402
from test_host import ReplayRandn  # noqa: E402

pytestmark = pytest.mark.gpu

NEW, PLAIN16, F32_LAYER = "fused_stacked16_layer_kernel<", "fused_stacked16_kernel<", "fused_shs_stacked_layer_kernel<float, "
K_OF = {6: 2, 7: 2, 8: 2, 9: 2, 10: 2, 11: 4}                      # fused_bwd_k(L, 8)
NT_MIN_BYTES = 256 << 20
dtypes = pytest.mark.parametrize("dtype", DTYPES, ids=("f16", "bf16"))


def _symbol(dtype, log2d, nt=False):
    return "whvi::fused_stacked16_layer_kernel<%s, %d, %d, %s>" % (TYPE_NAME[dtype], log2d, K_OF[log2d], "true" if nt else "false")


def _bias(J, D, dev, seed=0):
    return torch.randn(J * D, generator=torch.Generator().manual_seed(77 + 10 * J + D + seed)).to(dev)


def _want(x, a, b, c, S, B, shared, bias, n_cols, relu_in, relu_out):
    """The reference: the float32 layer launch on the exactly-upcast input, cast ONCE."""
    from whvi_amd import _hip
    return _hip.fused_shs_stacked_layer(x.float(), a, b, c, S, B, bias=bias, n_cols=n_cols, relu_in=relu_in, relu_out=relu_out,
                                        shared=shared).to(x.dtype)


def _layer_into_guarded(x, a, b, c, S, B, shared, bias, n_cols, ld, relu_in, relu_out):
    """The launch into rows of pitch ``ld`` inside a sentinel-filled buffer: the guards and the ``ld - n_cols`` gap columns of
    every row must still hold the sentinel."""
    from whvi_amd import _hip
    rows = S * B
    big = torch.full((GUARD + rows * ld + GUARD,), SENTINEL, dtype=x.dtype, device=x.device)
    pitched = big[GUARD:GUARD + rows * ld].view(rows, ld)
    dst = pitched[:, :n_cols]
    out = _hip.fused_shs_stacked_layer16(x, a, b, c, S, B, bias=bias, n_cols=n_cols, relu_in=relu_in, relu_out=relu_out,
                                         shared=shared, out=dst)
    assert out.data_ptr() == dst.data_ptr() and out.shape == (rows, n_cols) and out.dtype == x.dtype
    assert bool((big[:GUARD] == SENTINEL).all()) and bool((big[GUARD + rows * ld:] == SENTINEL).all()), "a guard was written"
    assert bool((pitched[:, n_cols:] == SENTINEL).all()), "a gap column was written"
    return dst


# ---- 1. the raw call
@pytest.mark.parametrize("log2d", [6, 7, 8, 9, 10, 11])
@dtypes
def test_raw_call_equals_the_float32_layer_launch_cast_once(dtype, log2d, hip_lib):
    from whvi_amd import _hip
    dev = torch.device("cuda")
    D = 1 << log2d
    most = 65536 // (16 * D)                     # the bias rule
    for J in sorted({j for j in (1, 2, 3, min(most, 5)) if j <= most}):
        assert _hip.fused_shs_stacked_layer16_supported(dtype, D, J, True)
        bias = _bias(J, D, dev)
        n_cols = (J - 1) * D + D // 2 + 8
        for S, B in ((1, 1), (3, 5), (2, 777), (4, 64)):
            for shared in (False, True):
                what = (J, S, B, shared)
                x, a, b, c = _operands(dtype, log2d, J, S, B, shared, dev)
                got = _layer_into_guarded(x, a, b, c, S, B, shared, bias, n_cols, n_cols + 16, True, True)
                assert _hip.last_kernel() == _symbol(dtype, log2d)
                want = _want(x, a, b, c, S, B, shared, bias, n_cols, True, True)
                assert bool(torch.isfinite(want).all()) and bool((want > 0).any()) and bool((want == 0).any())
                _assert_same(got, want, what)
                again = _layer_into_guarded(x, a, b, c, S, B, shared, bias, n_cols, n_cols + 16, True, True)
                assert torch.equal(got.contiguous().view(torch.int16), again.contiguous().view(torch.int16))
                if (S, B) != (3, 5):
                    continue
                for cols in (J * D, J * D - 8, (J - 1) * D + 8):
                    for with_bias in (False, True):
                        for relu_in in (False, True):
                            for relu_out in (False, True):
                                h = bias if with_bias else None
                                got = _layer_into_guarded(x, a, b, c, S, B, shared, h, cols, cols, relu_in, relu_out)
                                _assert_same(got, _want(x, a, b, c, S, B, shared, h, cols, relu_in, relu_out),
                                             what + (cols, with_bias, relu_in, relu_out))
                # no option at all: the bits of the launch without an epilogue
                plain = _hip.fused_shs_stacked_layer16(x, a, b, c, S, B, shared=shared)
                assert plain.shape == (S * B, J * D) and plain.is_contiguous() and plain.dtype == dtype
                assert torch.equal(plain.view(torch.int16), _hip.fused_shs_stacked16(x, a, b, c, S, B, shared=shared).view(torch.int16))


# ---- 2. past one tile per wave, and streaming
def _same_on_device(got, want, what):
    """``_assert_same``'s three conditions without the copy to the host (these outputs are hundreds of MiB)."""
    g, w = got.float() + 0.0, want.float() + 0.0
    gn, wn = torch.isnan(g), torch.isnan(w)
    assert torch.equal(gn, wn), (what, "NaN positions differ", int((gn != wn).sum()))
    bad = (g != w) & ~gn
    assert not bool(bad.any()), (what, int(bad.sum()), "first", g[bad][:4].tolist(), w[bad][:4].tolist())
    assert torch.equal(torch.isinf(g), torch.isinf(w)), what


def _slab_case(log2d, regime):
    """(J, B, n_cols) at S = 3 from tools/slab_table.py's mirror of fused_bwd_geom.  walk: J = 2 and the smallest batch with at
    least three tiles per wave and a ragged last slab (cached).  stream: the most blocks the bias rule allows up to 5 and the
    smallest ragged batch above the 256 MiB threshold of rows * 2 * (n_cols + D), at least two tiles per wave."""
    D, S = 1 << log2d, 3
    J = 2 if regime == "walk" else min(65536 // (16 * D), 5)
    n_cols = (J - 1) * D + D // 2 + 8
    per_row = 2 * (n_cols + D)
    first, need = (1, 3) if regime == "walk" else (NT_MIN_BYTES // (S * per_row) + 1, 2)
    for B in range(first, first + 200000):
        if st.tiles_per_wave(S, B, log2d) >= need and st.ragged(S, B, log2d):
            assert (S * B * per_row > NT_MIN_BYTES) == (regime == "stream")
            return J, B, n_cols
    raise AssertionError((log2d, regime))


@pytest.mark.parametrize("regime", ["walk", "stream"])
@pytest.mark.parametrize("log2d", [6, 7, 8, 9, 10, 11])
@dtypes
def test_slabs_past_one_tile_per_wave_and_streaming(dtype, log2d, regime, hip_lib):
    from whvi_amd import _hip
    dev = torch.device("cuda")
    D, S = 1 << log2d, 3
    J, B, n_cols = _slab_case(log2d, regime)
    g = torch.Generator(device=dev).manual_seed(100 * log2d + DTYPES.index(dtype))
    scale = 1.0 / D ** 0.5
    x = torch.randn(S * B, D, device=dev, generator=g).to(dtype)
    a = torch.randn(J, D, device=dev, generator=g) * scale
    b = torch.randn(J, S, D, device=dev, generator=g) * scale
    c = torch.randn(J, D, device=dev, generator=g)
    bias = torch.randn(J * D, device=dev, generator=g)
    got = _hip.fused_shs_stacked_layer16(x, a, b, c, S, B, bias=bias, n_cols=n_cols, relu_out=True)
    name = _hip.last_kernel()
    assert name == _symbol(dtype, log2d, nt=(regime == "stream")) and name.endswith("true>" if regime == "stream" else "false>")
    assert got.shape == (S * B, n_cols) and got.is_contiguous()
    want = _want(x, a, b, c, S, B, False, bias, n_cols, False, True)
    assert bool(torch.isfinite(want).all()) and bool((want > 0).any()) and bool((want == 0).any())
    _same_on_device(got, want, (log2d, regime, J, B))


# ---- 3. non-finite values
@pytest.mark.parametrize("log2d", [6, 9, 10, 11])
@dtypes
def test_non_finite_inputs(dtype, log2d, hip_lib):
    dev = torch.device("cuda")
    D = 1 << log2d
    J, S, B = min(65536 // (16 * D), 3), 3, 5
    n_cols = (J - 1) * D + D // 2 + 8
    for shared in (False, True):
        x, a, b, c = _operands(dtype, log2d, J, S, B, shared, dev, seed=7)
        bias = _bias(J, D, dev, seed=1)
        x[1, 3], x[1, D - 2], x[x.size(0) - 1, 0], x[x.size(0) - 1, D // 2] = float("inf"), float("-inf"), float("nan"), float("inf")
        bias[5] = float("nan")
        got = _layer_into_guarded(x, a, b, c, S, B, shared, bias, n_cols, n_cols + 16, True, True)
        want = _want(x, a, b, c, S, B, shared, bias, n_cols, True, True)
        assert bool(torch.isnan(want[:, 5]).all()) and bool(torch.isnan(want[1]).any()) and bool(torch.isfinite(want).any())
        _assert_same(got, want, (shared, "non-finite"))                    # (NaN survives both ReLUs where the reference has it)
        again = _layer_into_guarded(x, a, b, c, S, B, shared, bias, n_cols, n_cols + 16, True, True)
        _assert_same(again, got, (shared, "non-finite, second call"))


# ---- 4. one rounding, not three
@dtypes
def test_one_rounding_is_closer_to_float64_than_three(dtype, hip_lib):
    """Seeded Gaussian rows at D = 1024, J = 2 with a bias of order one.  float64 reference: the layer on the same 16-bit inputs
    (dense Hadamard products).  The launch rounds once; the flag-off route -- the 16-bit launch, ``+ bias.to(dtype)``,
    ``torch.relu`` -- rounds in the launch, in the bias cast and in the sum.  The launch is no further from float64 in the
    largest elementwise error and in RMS, and strictly closer in RMS."""
    from whvi_amd import _hip
    from whvi_amd.utils import build_H
    dev = torch.device("cuda")
    log2d, J, S, B = 10, 2, 3, 171
    D = 1 << log2d
    x, a, b, c = _operands(dtype, log2d, J, S, B, False, dev, seed=3)
    bias = _bias(J, D, dev, seed=2)
    folded = _hip.fused_shs_stacked_layer16(x, a, b, c, S, B, bias=bias, relu_out=True)
    assert _hip.last_kernel() == _symbol(dtype, log2d)
    unfolded = torch.relu(_hip.fused_shs_stacked16(x, a, b, c, S, B) + bias.to(dtype))
    H = build_H(D, dev).double()
    x64 = x.double().view(S, B, D)
    ref = torch.cat([a[j].double() * ((((c[j].double() * x64) @ H) * b[j].double().unsqueeze(1)) @ H) for j in range(J)], dim=-1)
    ref = torch.relu(ref + bias.double()).view(S * B, J * D)
    err = {name: (y.double() - ref).abs() for name, y in (("folded", folded), ("unfolded", unfolded))}
    worst = {k: float(v.max()) for k, v in err.items()}
    rms = {k: float((v * v).mean().sqrt()) for k, v in err.items()}
    print(f"{TYPE_NAME[dtype]}: max |y - ref64| folded {worst['folded']:.3e} unfolded {worst['unfolded']:.3e}; "
          f"RMS folded {rms['folded']:.3e} unfolded {rms['unfolded']:.3e}; max|ref64| {float(ref.max()):.3e}")
    assert bool(torch.isfinite(ref).all()) and float(ref.max()) > 1.0
    assert worst["folded"] <= worst["unfolded"]
    assert rms["folded"] < rms["unfolded"]


# ---- 5. routing through the Module
def _flags(sub, keep_half=True, fused_epilogue=True, fused_epilogue16=True):
    sub.keep_half, sub.fused_epilogue, sub.fused_epilogue16 = keep_half, fused_epilogue, fused_epilogue16


def _forward(layer, x, S, seed=31, **relus):
    """``(output, kernel named)`` of one batched pass under ``seed``, another kernel launched first."""
    from whvi_amd import _hip
    _hip.fwht_rows(torch.zeros(1, 4, device=x.device))                      # (another kernel's name in the note)
    torch.manual_seed(seed)
    with torch.no_grad():
        y = layer.forward_mc(x, S, **relus)
    return y, _hip.last_kernel()


@dtypes
def test_routing(dtype, hip_lib):
    dev = torch.device("cuda")
    S, B = 2, 9
    gen = torch.Generator().manual_seed(4)
    xs = lambda n_in, dt=dtype: [torch.randn(B, n_in, generator=gen).to(dev, dt),                        # noqa: E731
                                 torch.randn(S, B, n_in, generator=gen).to(dev, dt)]
    all_relus = ({}, {"relu_out": True}, {"relu_in": True, "relu_out": True})
    # folded: a bias at (128, 512); n_out = 200 written at pitch 200; n_out = 252 at pitch D_out behind the narrowing view
    for n_in, n_out in ((128, 512), (128, 200), (100, 252)):
        layer = make_layer(n_in, n_out).to(dev)
        sub = layer.weight_submodule
        for x in xs(n_in):
            for relus in all_relus:
                _flags(sub)
                assert layer.fuses_relu(x)
                y, name = _forward(layer, x, S, **relus)
                assert name == _symbol(dtype, 7), (n_in, n_out, name)
                assert y.shape == (S, B, n_out) and y.dtype == dtype
                if n_out % 8 == 0:
                    assert y.is_contiguous() and y.size(-1) == n_out and y.stride(1) == n_out
                else:
                    assert y.stride(1) == sub.D_out == 256 and not y.is_contiguous()
                # the float32 layer launch on the upcast input, cast once
                _flags(sub, keep_half=False)
                ref, ref_name = _forward(layer, x.float(), S, **relus)
                assert F32_LAYER in ref_name and ref.dtype == torch.float32
                _assert_same(y, ref.to(dtype), (n_in, n_out, tuple(x.shape), relus))
    # a narrowing alone is folded too (no bias, no ReLU, 200 % 8 == 0)
    layer = make_layer(128, 200, bias=False).to(dev)
    _flags(layer.weight_submodule)
    for x in xs(128):
        y, name = _forward(layer, x, S)
        assert NEW in name and y.is_contiguous() and y.shape == (S, B, 200)
    # not named, and the bits of today's route: any one of the three flags off ...
    layer = make_layer(128, 512).to(dev)
    sub = layer.weight_submodule
    for off in ("keep_half", "fused_epilogue", "fused_epilogue16"):
        for x in xs(128):
            for relus in all_relus:
                _flags(sub, **{off: False})
                assert not layer.fuses_relu(x)
                y, name = _forward(layer, x, S, **relus)
                assert NEW not in name, (off, name)
                _flags(sub, **{off: False, "fused_epilogue16": False})
                ref, _ = _forward(layer, x, S, **relus)
                assert y.dtype == ref.dtype == (torch.float32 if off == "keep_half" else dtype) and torch.equal(y, ref)
    # ... nothing to fold (no bias, no ReLU, n_out == D_out: the plain 16-bit launch) ...
    layer = make_layer(128, 512, bias=False).to(dev)
    sub = layer.weight_submodule
    for x in xs(128):
        _flags(sub)
        y, name = _forward(layer, x, S)
        assert NEW not in name and PLAIN16 + TYPE_NAME[dtype] in name
        _flags(sub, fused_epilogue16=False)
        assert torch.equal(y, _forward(layer, x, S)[0])
    # ... float32 input (the float32 layer launch), and five blocks of 1024 with a bias (beyond the LDS rule)
    for layer, inputs in ((make_layer(128, 512).to(dev), xs(128, torch.float32)), (make_layer(1024, 5120).to(dev), xs(1024))):
        sub = layer.weight_submodule
        for x in inputs:
            for relus in ({}, {"relu_in": True, "relu_out": True}):
                _flags(sub)
                y, name = _forward(layer, x, S, **relus)
                assert NEW not in name, name
                assert layer.fuses_relu(x) == (x.dtype == torch.float32)
                _flags(sub, fused_epilogue16=False)
                ref, _ = _forward(layer, x, S, **relus)
                assert y.dtype == ref.dtype == x.dtype and torch.equal(y, ref)


# ---- 6. gradients
@pytest.mark.parametrize("fused_backward", [False, True], ids=("loop", "one-launch"))
@pytest.mark.parametrize("n_out", [512, 200])
@dtypes
def test_gradients(dtype, n_out, fused_backward, monkeypatch, hip_lib):
    """``x, s1, s2, g_mu, g_rho``: the bits of the existing pieces called by hand on the launch's own ``y`` -- the mask of
    ``relu_out``, the zero padding, ``relu(x)``, ``_fastfood_stacked_backward`` with the same flags, the mask of ``relu_in`` --
    and autograd from ``a, b, c`` down to the parameters.  The bias: max|got - ref64| <= 1e-5 * max|ref64| against the float64
    column sum of the masked 16-bit gradient (the bound DESIGN 5.2g uses)."""
    from whvi_amd import _hip
    from whvi_amd.fastfood import _fastfood_stacked_backward
    dev = torch.device("cuda")
    S, B, n_in = 3, 65, 128
    layer = make_layer(n_in, n_out).to(dev)
    sub = layer.weight_submodule
    _flags(sub)
    sub.fused_backward = sub.fused_backward16 = fused_backward
    J, D = sub.stack, sub.D_in
    eps = torch.randn(J, S, D, generator=torch.Generator().manual_seed(5))
    names = [n for n, _ in sub.named_parameters()]
    params = list(sub.parameters())
    for shape in ((B, n_in), (S, B, n_in)):
        shared = len(shape) == 2
        x = torch.randn(shape, generator=torch.Generator().manual_seed(8)).to(dev, dtype)
        w = torch.randn(S, B, n_out, generator=torch.Generator().manual_seed(6)).to(dev, dtype)
        xr = x.clone().requires_grad_()
        monkeypatch.setattr(torch, "randn", ReplayRandn([eps.numpy()]))
        _hip.fwht_rows(torch.zeros(1, 4, device=dev))
        y = layer.forward_mc(xr, S, relu_in=True, relu_out=True)
        named = _hip.last_kernel()
        monkeypatch.undo()
        assert named == _symbol(dtype, 7) and y.dtype == dtype and y.shape == (S, B, n_out)
        got = torch.autograd.grad(y, [xr] + params, grad_outputs=w)
        # by hand, on the launch's own y
        s1, s2 = sub._stacked("s1"), sub._stacked("s2")
        g_mat = sub._stacked("g_mu").unsqueeze(1) + F.softplus(sub._stacked("g_rho")).unsqueeze(1) * eps.to(dev)
        gy = torch.ops.aten.threshold_backward(w.reshape(S * B, n_out), y.detach().reshape(S * B, n_out), 0).contiguous()
        ref64 = F.pad(gy.double().sum(dim=0), (0, J * D - n_out))
        gpad = F.pad(gy, (0, J * D - n_out)) if n_out < J * D else gy
        rows = x if shared else x.reshape(S * B, n_in)
        xin = torch.relu(rows)
        gx, ga, gb, gc = _fastfood_stacked_backward(gpad, xin, s1.detach(), g_mat.detach(), s2.detach(), S, B, shared, True,
                                                    fused_backward, (True, True, True, True), fused_backward)
        gx = torch.ops.aten.threshold_backward(gx, xin, 0)
        others = [p for n, p in zip(names, params) if n != "bias"]
        want = (gx.view(shape),) + torch.autograd.grad([s1, g_mat, s2], others, grad_outputs=[ga, gb, gc])
        assert got[0].dtype == dtype and got[0].shape == x.shape
        for name, p, q in zip(["x"] + [n for n in names if n != "bias"], [g for n, g in zip(["x"] + names, got) if n != "bias"], want):
            assert p.shape == q.shape and p.dtype == q.dtype, name
            assert bool(torch.isfinite(q.float()).all()), name
            assert torch.equal(p, q), name
        gbias = got[1 + names.index("bias")]
        ratio = float((gbias.double().flatten() - ref64).abs().max()) / float(ref64.abs().max())
        print(f"{TYPE_NAME[dtype]} n_out={n_out} fused_backward={fused_backward} x{tuple(shape)}: bias gradient error / max|ref64| = "
              f"{ratio:.3e}")
        assert gbias.shape == (1, sub.D_out) and gbias.dtype == torch.float32
        assert bool((gbias[0, n_out:] == 0).all())
        assert ratio <= 1e-5


# ---- 7. a three-layer network
@dtypes
def test_network_folds_the_relu(dtype, monkeypatch, hip_lib):
    from whvi_amd import _hip
    dev = torch.device("cuda")
    S, B = 4, 33
    torch.manual_seed(0)
    relus = [nn.ReLU(), nn.ReLU()]
    dims = ((64, 128, True), (128, 200, True), (200, 8, False))
    net = WHVIRegression([WHVILinear(64, 128, mode=MODE, bias=True), relus[0], WHVILinear(128, 200, mode=MODE, bias=True), relus[1],
                          WHVILinear(200, 8, mode=MODE, bias=False)], train_samples=S, eval_samples=S).to(dev)
    layers = [m for m in net.sequential if isinstance(m, WHVILinear)]
    subs = [m.weight_submodule for m in layers]
    assert len(subs) == 3 and all(type(s).__name__ == "WHVIFastfoodStackedMatrix" for s in subs)
    with torch.no_grad():
        for s in subs:                                        # parameters of order one, as make_layer's
            for m in s.weight_matrices:
                m.g_mu.copy_(torch.randn(s.D_in, device=dev) * 0.3)
                m.s1.mul_(10.0)
                m.s2.mul_(10.0)
            if s.bias is not None:
                s.bias.copy_(torch.randn(1, s.D_out, device=dev) * 0.1)
    for s in subs:
        _flags(s)
    mid = layers[1]
    x = torch.randn(B, 64, generator=torch.Generator().manual_seed(1)).to(dev, dtype)
    eps = [torch.randn(s.stack, S, s.D_in, generator=torch.Generator().manual_seed(40 + i)) for i, s in enumerate(subs)]
    calls, ran = [], [0, 0]
    real = mid.forward_mc
    monkeypatch.setattr(mid, "forward_mc", lambda h, n, **kw: (calls.append(kw), real(h, n, **kw))[1])
    for i, r in enumerate(relus):
        r.register_forward_hook(lambda m, a, o, i=i: ran.__setitem__(i, ran[i] + 1))
    with monkeypatch.context() as m:
        m.setattr(torch, "randn", ReplayRandn([e.numpy() for e in eps]))
        with torch.no_grad():
            out = net.forward_batched(x, S)
    assert len(calls) == 1 and calls[0].get("relu_out") is True and not calls[0].get("relu_in"), calls
    assert ran == [0, 0], "a ReLU next to a folding layer ran as a pass of its own"
    assert NEW + TYPE_NAME[dtype] in _hip.last_kernel()
    # the reference: float32 layer launches on the upcast activations, cast once per layer
    h = x
    with torch.no_grad():
        for i, (s, (n_in, n_out, _)) in enumerate(zip(subs, dims)):
            g = s._stacked("g_mu").unsqueeze(1) + F.softplus(s._stacked("g_rho")).unsqueeze(1) * eps[i].to(dev)
            hp = F.pad(h, (0, s.padding)) if s.padding > 0 else h
            shared = hp.dim() == 2
            rows = hp if shared else hp.reshape(S * B, s.D_in)
            y = _hip.fused_shs_stacked_layer(rows.float().contiguous(), s._stacked("s1"), g, s._stacked("s2"), S, B, bias=s.bias,
                                             n_cols=n_out, relu_out=i < 2, shared=shared)
            h = y.to(dtype).view(S, B, n_out)
    assert out.shape == (B, 8, S) and out.dtype == dtype and bool(torch.isfinite(h.float()).all())
    _assert_same(out, h.permute(1, 2, 0), "network")


# ---- 8. hipGraph and the allocator's peak
def test_graph_capture_and_replay(hip_lib):
    from whvi_amd import _hip
    dev = torch.device("cuda")
    dtype, log2d, J, S, B = torch.float16, 10, 4, 2, 64               # the (1024, 4096) layer
    x, a, b, c = _operands(dtype, log2d, J, S, B, False, dev)
    bias = _bias(J, 1 << log2d, dev)
    kw = dict(bias=bias, relu_in=True, relu_out=True)
    eager = _hip.fused_shs_stacked_layer16(x, a, b, c, S, B, **kw)
    _assert_same(eager, _want(x, a, b, c, S, B, False, bias, J << log2d, True, True), "eager")
    y = torch.zeros_like(eager)
    side = torch.cuda.Stream()
    side.wait_stream(torch.cuda.current_stream())
    with torch.cuda.stream(side):
        _hip.fused_shs_stacked_layer16(x, a, b, c, S, B, out=y, **kw)
    torch.cuda.current_stream().wait_stream(side)
    graph = torch.cuda.CUDAGraph()
    with torch.cuda.graph(graph):
        _hip.fused_shs_stacked_layer16(x, a, b, c, S, B, out=y, **kw)
    for _ in range(2):
        y.zero_()
        graph.replay()
        torch.cuda.synchronize()
        assert torch.equal(y.view(torch.int16), eager.view(torch.int16))


def test_peak_memory_of_the_forward(hip_lib):
    """D = 1024, J = 4, S = 8, B = 4096 with a bias and a ReLU: one result tensor with the flags on; with ``fused_epilogue16`` off
    the launch's output and the sum (then the sum and the ReLU's output) are alive together: two."""
    dev = torch.device("cuda")
    S, B = 8, 4096
    layer = make_layer(1024, 4096).to(dev)
    x = torch.randn(S, B, 1024, generator=torch.Generator().manual_seed(3)).to(dev, torch.float16)
    result = S * B * 4096 * 2
    peak = {}
    for flag in (False, True):
        _flags(layer.weight_submodule, fused_epilogue16=flag)
        torch.manual_seed(4)
        torch.cuda.synchronize()
        torch.cuda.empty_cache()
        torch.cuda.reset_peak_memory_stats()
        base = torch.cuda.memory_allocated()
        with torch.no_grad():
            y = layer.forward_mc(x, S, relu_out=True)
        torch.cuda.synchronize()
        peak[flag] = torch.cuda.max_memory_allocated() - base
        assert y.shape == (S, B, 4096) and y.dtype == torch.float16
        del y
    print(f"forward peak above the inputs, D = 1024, J = 4, S = 8, B = 4096, fp16, bias + ReLU: flags on {peak[True] / 2**20:.0f} MiB, "
          f"fused_epilogue16 off {peak[False] / 2**20:.0f} MiB; one result tensor is {result / 2**20:.0f} MiB")
    assert result <= peak[True] < 1.25 * result
    assert peak[False] >= 2 * result
