"""The one-launch backward of the fused pipeline on 16-bit activation streams (whvi_fused_shs_bwd_f16 / _bf16,
``FastfoodFunction(..., keep_half=True, fused_backward=True)``) on the GPU.

Operands: ``x`` and ``grad_y`` are seeded ``randn`` rounded to the dtype; ``a, b, c`` are float32 ``randn`` with ``a`` and ``b``
scaled by 1 / sqrt(D) as in tests/test_fused16_gpu.py, so that fp16 results stay finite.  Per case:

1. ``grad_x`` is ``_hip.fused_shs(grad_y16, c, b, a)`` -- the 16-bit forward launch with ``a`` and ``c`` exchanged -- under that
   file's ``_assert_same`` (values after ``+ 0.0``, NaN and inf positions, no tolerance).
2. ``grad_a, grad_b, grad_c`` against float64 autograd of the dense product built with ``build_H`` on the operands upcast to
   double: max|got - ref64| <= 1e-5 max|ref64| per tensor, the project's bound for this composition (contract 2).
   The ``keep_half`` chain (flag off: the existing route) goes through the same check and is asserted too; both ratios are
   printed per case before anything is asserted.
3. From D = 512 up the parameter gradients are bit-equal (after ``+ 0.0``) to the float32 launch on the upcast tensors,
   ``_hip.fused_shs_bwd(grad_y16.float(), x16.float(), ...)``: the same grid, rows per tile, fma operand order, wave order and
   block order.  Below 512 the lanes of a column hold other rows than in the float32 kernel, and only check 2 applies.
4. Two calls are bit-equal; ``need_x=False`` returns no ``grad_x`` and the same sums.

The shapes (S, B) are the float32 test's: (1, 1) leaves three of the block's four waves idle, (3, 5) and (2, 777) end in ragged
tiles and slabs, (4, 64) is whole tiles; D < 512 puts several rows side by side in a wave (lanes share columns), D >= 2048 reads
``x`` a second time."""
import pytest
import torch

pytestmark = pytest.mark.gpu

BOUND = 1e-5
DTYPES = (torch.float16, torch.bfloat16)
TYPE_NAME = {torch.float16: "__half", torch.bfloat16: "__hip_bfloat16"}
SHAPES = ((1, 1), (3, 5), (2, 777), (4, 64))
CASES = [(log2d, S, B) for log2d in range(6, 13) for (S, B) in SHAPES]
_H = {}


def _dev():
    if not torch.cuda.is_available():
        pytest.skip("needs a GPU")
    return torch.device("cuda", 0)


def _build_h(D, dev):
    if D not in _H:
        from whvi_amd.utils import build_H
        _H[D] = build_H(D, dev).double()
    return _H[D]


def _inputs(dtype, log2d, S, B, shared, dev):
    D = 1 << log2d
    g = torch.Generator().manual_seed(2000 * log2d + 20 * CASES.index((log2d, S, B)) + 2 * int(shared) + DTYPES.index(dtype))
    x = torch.randn(B if shared else S * B, D, generator=g).to(dtype)
    gy = torch.randn(S * B, D, generator=g).to(dtype)
    scale = 1.0 / D ** 0.5
    a = torch.randn(D, generator=g) * scale
    b = torch.randn(S, D, generator=g) * scale
    c = torch.randn(D, generator=g)
    return tuple(t.to(dev) for t in (x, gy, a, b, c))


def _ref64(x, gy, a, b, c, S, B, shared):
    """float64 autograd of the dense a (.) (H @ (b_s (.) (H @ (c (.) x)))) on the operands upcast to double."""
    D = x.size(1)
    H = _build_h(D, x.device)
    x64, a64, b64, c64 = (t.double().requires_grad_() for t in (x, a, b, c))
    xs = x64.unsqueeze(0).expand(S, B, D) if shared else x64.view(S, B, D)
    t1 = (c64 * xs) @ H
    y = a64 * ((b64.unsqueeze(1) * t1) @ H)
    (y * gy.double().view(S, B, D)).sum().backward()
    return x64.grad, a64.grad, b64.grad, c64.grad


def _ratio(got, ref):
    return float((got.double() - ref).abs().max()) / float(ref.abs().max())


def _assert_same(got, want, what):
    """tests/test_fused16_gpu.py's comparison: values after + 0.0, NaN and inf positions, no tolerance."""
    g, w = got.detach().cpu().float() + 0.0, want.detach().cpu().float() + 0.0
    gn, wn = torch.isnan(g), torch.isnan(w)
    assert torch.equal(gn, wn), (what, "NaN positions differ", int((gn != wn).sum()))
    bad = (g != w) & ~gn
    assert not bool(bad.any()), (what, int(bad.sum()), "first", g[bad][:4].tolist(), w[bad][:4].tolist())
    assert torch.equal(torch.isinf(g), torch.isinf(w)), what


def _bits_equal(u, v):
    return torch.equal((u + 0.0).view(torch.int32), (v + 0.0).view(torch.int32))


def _note_backward_kernel(leaf, seen):
    """Appends to ``seen`` what ``_hip.last_kernel()`` says once the backward has produced ``leaf``'s gradient.  Autograd runs
    the backward on a thread of its own and ``whvi_last_kernel`` is per thread, so the question is put there, by a hook."""
    from whvi_amd import _hip
    leaf.register_hook(lambda grad: seen.append(_hip.last_kernel()))


def _through_function(x, gy, a, b, c, S, stride, shared, keep_half, fused, need_x=True):
    """(grad_x | None, grad_a, grad_b, grad_c) through FastfoodFunction, and the library's last kernel on the backward thread
    when ``a``'s gradient arrived."""
    from whvi_amd.fastfood import FastfoodFunction
    xs = x.clone().requires_grad_(need_x)
    as_, bs, cs = (t.clone().requires_grad_() for t in (a, b, c))
    seen = []
    _note_backward_kernel(as_, seen)
    y = FastfoodFunction.apply(xs, as_, bs, cs, S, stride, shared, keep_half, fused)
    y.backward(gy.to(y.dtype))
    assert len(seen) == 1
    return (xs.grad, as_.grad, bs.grad, cs.grad), seen[0], y.dtype


@pytest.mark.parametrize("shared", (False, True), ids=("own_x", "shared_x"))
@pytest.mark.parametrize("log2d,S,B", CASES)
@pytest.mark.parametrize("dtype", DTYPES, ids=("f16", "bf16"))
def test_gradients(dtype, log2d, S, B, shared):
    from whvi_amd import _hip
    dev = _dev()
    D = 1 << log2d
    x, gy, a, b, c = _inputs(dtype, log2d, S, B, shared, dev)
    ref = _ref64(x, gy, a, b, c, S, B, shared)
    raw = _hip.fused_shs_bwd(gy, x, a, b, c, S, B, shared=shared)
    name = _hip.last_kernel()
    assert name.startswith(f"whvi::fused_shs_bwd_kernel<{TYPE_NAME[dtype]}, {log2d}, "), name
    assert raw[0].dtype == dtype and all(t.dtype == torch.float32 for t in raw[1:])
    assert raw[0].shape == (S * B, D) and raw[1].shape == (D,) and raw[2].shape == (S, D) and raw[3].shape == (D,)
    chain, chain_kernel, _ = _through_function(x, gy, a, b, c, S, B, shared, True, False)
    assert "fused_shs_bwd" not in chain_kernel, chain_kernel
    # 2. (measured first, printed before any assertion) the parameter gradients of both routes against float64
    worst = {n: (_ratio(g_on, r), _ratio(g_off, r)) for n, g_on, g_off, r in zip("abc", raw[1:], chain[1:], ref[1:])}
    print(f"fused_bwd16 {TYPE_NAME[dtype]} D={D} S={S} B={B} shared={shared} ratios (fused, chain): " +
          " ".join(f"{k}={v[0]:.2e}/{v[1]:.2e}" for k, v in worst.items()))
    # 1. grad_x: the 16-bit launch that computes it alone, a and c exchanged
    alone = _hip.fused_shs(gy, c, b, a, axis="col", n_samples=S, sample_stride=B)
    assert alone.dtype == dtype
    _assert_same(raw[0], alone, (dtype, log2d, S, B, shared, "grad_x"))
    for n in "abc":
        assert worst[n][1] <= BOUND, ("chain", n, worst[n])
        assert worst[n][0] <= BOUND, ("fused", n, worst[n])
    # 3. the float32 launch on the upcast tensors: the same bits from D = 512 up
    if D >= 512:
        wide = _hip.fused_shs_bwd(gy.float(), x.float(), a, b, c, S, B, shared=shared, need_x=False)
        assert "fused_shs_bwd_kernel<float" in _hip.last_kernel()
        for n, u, v in zip("abc", raw[1:], wide[1:]):
            assert _bits_equal(u, v), (dtype, log2d, S, B, shared, "grad_" + n, int((u != v).sum()))
    # 4. a second call, all four outputs; need_x=False: no grad_x, the same sums
    again = _hip.fused_shs_bwd(gy, x, a, b, c, S, B, shared=shared)
    assert torch.equal(raw[0].view(torch.int16), again[0].view(torch.int16))
    for u, v in zip(raw[1:], again[1:]):
        assert torch.equal(u.view(torch.int32), v.view(torch.int32))
    skipped = _hip.fused_shs_bwd(gy, x, a, b, c, S, B, shared=shared, need_x=False)
    assert skipped[0] is None
    for u, v in zip(raw[1:], skipped[1:]):
        assert torch.equal(u.view(torch.int32), v.view(torch.int32))


@pytest.mark.parametrize("dtype", DTYPES, ids=("f16", "bf16"))
def test_kernel_named_through_the_function(dtype):
    """Both flags: the 16-bit backward kernel, named on the backward thread; either flag off: not named.  grad_x comes back in
    x's dtype, the parameter gradients in float32, and they are the raw call's."""
    from whvi_amd import _hip
    dev = _dev()
    log2d, S, B = 11, 4, 64
    x, gy, a, b, c = _inputs(dtype, log2d, S, B, False, dev)
    raw = _hip.fused_shs_bwd(gy, x, a, b, c, S, B)
    for keep_half, fused in ((True, True), (True, False), (False, True), (False, False)):
        got, kernel, y_dtype = _through_function(x, gy, a, b, c, S, B, False, keep_half, fused)
        both = keep_half and fused
        assert (f"fused_shs_bwd_kernel<{TYPE_NAME[dtype]}" in kernel) == both, (keep_half, fused, kernel)
        assert "fused_shs_bwd" not in kernel or both, (keep_half, fused, kernel)
        assert y_dtype == (dtype if keep_half else torch.float32)
        assert got[0].dtype == dtype and all(t.dtype == torch.float32 for t in got[1:])
        if both:
            assert kernel == f"whvi::fused_shs_bwd_kernel<{TYPE_NAME[dtype]}, 11, 4, false>", kernel
            assert torch.equal(got[0].view(torch.int16), raw[0].view(torch.int16))
            for u, v in zip(got[1:], raw[1:]):
                assert torch.equal(u.view(torch.int32), v.view(torch.int32))


@pytest.mark.parametrize("dtype", DTYPES, ids=("f16", "bf16"))
def test_shared_x_keeps_the_chain_when_it_needs_a_gradient(dtype):
    from whvi_amd import _hip
    dev = _dev()
    log2d, S, B = 9, 3, 5
    x, gy, a, b, c = _inputs(dtype, log2d, S, B, True, dev)
    needing, kernel, _ = _through_function(x, gy, a, b, c, S, B, True, True, True, need_x=True)
    assert "fused_shs_bwd" not in kernel, kernel
    off, _, _ = _through_function(x, gy, a, b, c, S, B, True, True, False, need_x=True)
    assert needing[0].dtype == dtype and needing[0].shape == (B, 1 << log2d)
    assert torch.equal(needing[0].view(torch.int16), off[0].view(torch.int16))       # ONE rounding of the float32 sum over samples
    for u, v in zip(needing[1:], off[1:]):
        assert torch.equal(u.view(torch.int32), v.view(torch.int32))
    free, kernel, _ = _through_function(x, gy, a, b, c, S, B, True, True, True, need_x=False)
    assert f"fused_shs_bwd_kernel<{TYPE_NAME[dtype]}" in kernel, kernel
    raw = _hip.fused_shs_bwd(gy, x, a, b, c, S, B, shared=True, need_x=False)
    assert free[0] is None
    for u, v in zip(free[1:], raw[1:]):
        assert torch.equal(u.view(torch.int32), v.view(torch.int32))


@pytest.mark.parametrize("dtype", DTYPES, ids=("f16", "bf16"))
def test_module_gradients_are_the_raw_call(dtype):
    """WHVIFastfoodMatrix with both flags on a 3-D input: s1.grad and s2.grad are the raw call's grad_a and grad_c for the same
    seeded g."""
    from whvi_amd import _hip
    from whvi_amd.fastfood import WHVIFastfoodMatrix
    dev = _dev()
    D, S, B = 1024, 3, 37
    g = torch.Generator().manual_seed(5)
    x = torch.randn(S, B, D, generator=g).to(dtype).to(dev).requires_grad_()
    w = torch.randn(S, B, D, generator=g).to(dtype).to(dev)
    torch.manual_seed(11)
    layer = WHVIFastfoodMatrix(D).to(dev)
    with torch.no_grad():
        layer.s1.mul_(3.0)
        layer.s2.mul_(30.0)
        layer.g_mu.normal_()
    layer.keep_half = layer.fused_backward = True
    seen = []
    _note_backward_kernel(layer.s1, seen)
    torch.manual_seed(77)
    out = layer.forward_mc(x, S)
    assert out.dtype == dtype
    (out * w).sum().backward()
    assert len(seen) == 1 and f"fused_shs_bwd_kernel<{TYPE_NAME[dtype]}" in seen[0], seen
    torch.manual_seed(77)
    eps = torch.randn(S, D, device=dev)
    gk = (layer.g_mu + layer.g_sigma * eps).detach()
    raw = _hip.fused_shs_bwd(w.reshape(S * B, D), x.detach().reshape(S * B, D), layer.s1.detach(), gk, layer.s2.detach(), S, B)
    assert x.grad.dtype == dtype and layer.s1.grad.dtype == torch.float32
    assert torch.equal(x.grad.reshape(S * B, D).view(torch.int16), raw[0].view(torch.int16))
    assert torch.equal(layer.s1.grad, raw[1]) and torch.equal(layer.s2.grad, raw[3])
    assert bool(torch.isfinite(layer.g_mu.grad).all()) and bool(torch.isfinite(layer.g_rho.grad).all())


@pytest.mark.parametrize("what", ("d32", "d8192", "rows", "params16"))
def test_refusals_keep_the_chain(what):
    """D = 32, D = 8192, rows != S * stride and 16-bit parameters take the existing chain with both flags set: the kernel is not
    named and every gradient has the bits of ``keep_half`` alone."""
    from whvi_amd.fastfood import FastfoodFunction
    dev = _dev()
    dtype = torch.bfloat16
    D = {"d32": 32, "d8192": 8192}.get(what, 256)
    S, stride = 2, 3
    rows = S * stride * 2 if what == "rows" else S * stride           # two groups of (S, stride) rows: s(r) = (r // stride) % S
    g = torch.Generator().manual_seed(78)
    x, gy = (torch.randn(rows, D, generator=g).to(dtype).to(dev) for _ in range(2))
    a, b, c = torch.randn(D, generator=g) / D ** 0.5, torch.randn(S, D, generator=g) / D ** 0.5, torch.randn(D, generator=g)
    a, b, c = (t.to(dev, dtype if what == "params16" else torch.float32) for t in (a, b, c))
    got = {}
    for fused in (False, True):
        xs, as_, bs, cs = (t.clone().requires_grad_() for t in (x, a, b, c))
        seen = []
        _note_backward_kernel(as_, seen)
        y = FastfoodFunction.apply(xs, as_, bs, cs, S, stride, False, True, fused)
        assert y.dtype == dtype
        y.backward(gy)
        assert len(seen) == 1 and "fused_shs_bwd" not in seen[0], seen
        got[fused] = (xs.grad, as_.grad, bs.grad, cs.grad)
    for u, v in zip(got[False], got[True]):
        assert u.dtype == v.dtype and torch.equal(u, v) and bool(torch.isfinite(u.float()).all())


@pytest.mark.parametrize("dtype", DTYPES, ids=("f16", "bf16"))
def test_hip_graph_replay(dtype):
    """One capture on a single stream at D = 2048, replayed: the bits of the eager call."""
    from whvi_amd import _hip
    dev = _dev()
    log2d, S, B = 11, 3, 5
    x, gy, a, b, c = _inputs(dtype, log2d, S, B, False, dev)
    eager = _hip.fused_shs_bwd(gy, x, a, b, c, S, B)
    side = torch.cuda.Stream()
    side.wait_stream(torch.cuda.current_stream())
    with torch.cuda.stream(side):
        _hip.fused_shs_bwd(gy, x, a, b, c, S, B)
    torch.cuda.current_stream().wait_stream(side)
    graph = torch.cuda.CUDAGraph()
    with torch.cuda.graph(graph):
        captured = _hip.fused_shs_bwd(gy, x, a, b, c, S, B)
    for _ in range(2):
        for t in captured:
            t.zero_()
        graph.replay()
        torch.cuda.synchronize()
        assert torch.equal(captured[0].view(torch.int16), eager[0].view(torch.int16))
        for u, v in zip(captured[1:], eager[1:]):
            assert torch.equal(u.view(torch.int32), v.view(torch.int32))


def test_memory():
    """D = 1024, S = 8, B = 4096: a 16-bit activation is A = 64 MiB.  Peak above what is held before the backward: both flags,
    grad_x + the workspace + allocator rounding; flag off, at least the two float32 upcasts (4 A)."""
    from whvi_amd import _hip
    from whvi_amd.fastfood import FastfoodFunction
    dev = _dev()
    dtype = torch.bfloat16
    D, S, B = 1024, 8, 4096
    A = S * B * D * 2
    g = torch.Generator(device=dev).manual_seed(3)
    x = torch.randn(S * B, D, device=dev, generator=g).to(dtype)
    gy = torch.randn(S * B, D, device=dev, generator=g).to(dtype)
    a, c = torch.randn(D, device=dev, generator=g) / D ** 0.5, torch.randn(D, device=dev, generator=g)
    b = torch.randn(S, D, device=dev, generator=g) / D ** 0.5
    work = int(_hip.lib().whvi_fused_shs_bwd_workspace(S, B, 10))
    peaks = {}
    for fused in (True, False):
        xs, as_, bs, cs = (t.clone().requires_grad_() for t in (x, a, b, c))
        y = FastfoodFunction.apply(xs, as_, bs, cs, S, B, False, True, fused)
        torch.cuda.synchronize()
        torch.cuda.reset_peak_memory_stats(dev)
        held = torch.cuda.memory_allocated(dev)
        y.backward(gy)
        torch.cuda.synchronize()
        peaks[fused] = torch.cuda.max_memory_allocated(dev) - held
        assert xs.grad.dtype == dtype
        del xs, as_, bs, cs, y
    print(f"fused_bwd16 memory: A = {A >> 20} MiB, workspace {work} B, peak fused {peaks[True] / A:.3f} A, "
          f"chain {peaks[False] / A:.3f} A")
    assert peaks[True] <= A + work + (4 << 20), peaks
    assert peaks[False] >= 4 * A, peaks
