"""The one-launch backward of the rectangular fastfood layer (whvi_fused_shs_stacked_bwd_f32,
``FastfoodStackedFunction(..., fused_backward=True)``) on the GPU.

1. The raw call against the per-block launches (``_hip.fused_shs_bwd`` on the contiguous copy of each segment of ``grad_y``):
   the 3 J parameter gradients bit-equal, ``grad_x`` bit-equal to the per-block ``grad_x`` added in ascending ``j``, two calls
   bit-equal, ``need_x=False``, guards around ``grad_y`` and ``grad_x`` -- every shipped (D, J), own and shared ``x``.
2. All four gradients against float64 autograd of the dense product built with ``build_H``: max|got - ref64| <= 1e-5 max|ref64|
   per tensor, the project's bound for this composition (tests/test_fused_bwd_gpu.py).  The per-block route's ratios are computed
   first and printed beside the launch's; a tensor on which the per-block route itself misses the bound is reported and not
   charged to the launch (check 1 holds it to that route's bits).
3. Routing of ``FastfoodStackedFunction.backward``, asked by a hook (autograd runs the backward on a thread of its own).
4. The Module: every gradient with the launch ``torch.equal`` to the per-block launches.
5. One graph capture, and the peak memory of the backward.

Peak memory (printed by test 5): D = 1024, J = 4, S = 8, B = 4096, A = 128 MiB."""
import pytest
import torch

from test_fastfood_stacked_host import check_layer_against_dense, make_layer

pytestmark = pytest.mark.gpu

BOUND = 1e-5
SENTINEL = -777.25
GUARD = 1024                                     # floats on each side of a guarded buffer
SHAPES = ((1, 1), (3, 5), (2, 777), (4, 64))     # a lone row, a ragged TAIL tile, a slab boundary, several samples
SHIPPED = [(log2d, J) for log2d in range(6, 11) for J in (2, 3, 4)] + [(11, 2)]
KERNEL = "fused_shs_stacked_bwd_kernel"
_H = {}


def _build_h(D, dev):
    if D not in _H:
        from whvi_amd.utils import build_H
        _H[D] = build_H(D, dev).double()
    return _H[D]


def _operands(log2d, J, S, B, shared, dev):
    """Seeded finite normal data; a, b, c of order one."""
    D = 1 << log2d
    g = torch.Generator().manual_seed(100000 * log2d + 10000 * J + 1000 * S + 2 * B + int(shared))
    x = torch.randn(B if shared else S * B, D, generator=g)
    gy = torch.randn(S * B, J * D, generator=g)
    a, c = torch.randn(J, D, generator=g), torch.randn(J, D, generator=g)
    b = torch.randn(J, S, D, generator=g)
    return tuple(t.to(dev) for t in (x, gy, a, b, c))


def _guarded(shape, dev, fill=None):
    """``(big, view)``: ``view`` of ``shape`` inside a sentinel-filled buffer with GUARD floats on each side."""
    n = 1
    for d in shape:
        n *= d
    big = torch.full((GUARD + n + GUARD,), SENTINEL, device=dev)
    view = big[GUARD:GUARD + n].view(*shape)
    if fill is not None:
        view.copy_(fill)
    return big, view


def _guards_intact(big):
    return bool((big[:GUARD] == SENTINEL).all()) and bool((big[-GUARD:] == SENTINEL).all())


def _per_block(gy, x, a, b, c, S, B, shared):
    """The per-block launches on contiguous segments: ``(grad_x added in ascending j, per (sample, row); the list of each
    block's grad_x; grad_a (J, D); grad_b (J, S, D); grad_c (J, D))``."""
    from whvi_amd import _hip
    J, D = a.shape
    outs = [_hip.fused_shs_bwd(gy[:, j * D:(j + 1) * D].contiguous(), x, a[j], b[j], c[j], S, B, shared=shared) for j in range(J)]
    gx = outs[0][0]
    for o in outs[1:]:
        gx = gx + o[0]
    return gx, [o[0] for o in outs], torch.stack([o[1] for o in outs]), torch.stack([o[2] for o in outs]), torch.stack([o[3] for o in outs])


def _ref64(x, gy, a, b, c, S, B, shared):
    """float64 autograd of the J dense products a_j (.) (H @ (b_js (.) (H @ (c_j (.) x)))) side by side, from the same float32
    operands; ``grad_x`` folded over the samples for a shared ``x``."""
    J, D = a.shape
    H = _build_h(D, x.device)
    x64, a64, b64, c64 = (t.double().requires_grad_() for t in (x, a, b, c))
    xs = x64.unsqueeze(0).expand(S, B, D) if shared else x64.view(S, B, D)
    y = torch.cat([a64[j] * ((b64[j].unsqueeze(1) * ((c64[j] * xs) @ H)) @ H) for j in range(J)], dim=-1)
    (y * gy.double().view(S, B, J * D)).sum().backward()
    return x64.grad, a64.grad, b64.grad, c64.grad


def _ratio(got, ref):
    return float((got.double() - ref).abs().max()) / float(ref.abs().max())


def _eq(u, v):
    return torch.equal(u.view(torch.int32), v.view(torch.int32))


# ---- 1. the raw call against the per-block launches --------------------------------------------------------------------------
@pytest.mark.parametrize("shared", (False, True), ids=("own_x", "shared_x"))
@pytest.mark.parametrize("log2d,J", SHIPPED)
def test_bit_equal_to_the_per_block_launches(log2d, J, shared, hip_lib):
    from whvi_amd import _hip
    dev = torch.device("cuda")
    D = 1 << log2d
    assert _hip.fused_shs_stacked_bwd_supported(torch.float32, D, J)
    for S, B in SHAPES:
        x, gy0, a, b, c = _operands(log2d, J, S, B, shared, dev)
        big_y, gy = _guarded((S * B, J * D), dev, fill=gy0)
        big_x, gx = _guarded((S * B, D), dev)
        got = _hip.fused_shs_stacked_bwd(gy, x, a, b, c, S, B, shared=shared, grad_x=gx)
        assert _hip.last_kernel() == f"whvi::{KERNEL}<float, {log2d}, {8 if log2d == 11 else 4}, {J}, false>"
        assert got[0].data_ptr() == gx.data_ptr()
        assert _guards_intact(big_x) and _guards_intact(big_y), "a guard was written"
        assert _eq(gy, gy0)
        want_x, _, want_a, want_b, want_c = _per_block(gy0, x, a, b, c, S, B, shared)
        assert all(bool(torch.isfinite(t).all()) for t in (want_x, want_a, want_b, want_c))
        case = (log2d, J, S, B, shared)
        assert got[1].shape == (J, D) and got[2].shape == (J, S, D) and got[3].shape == (J, D)
        for j in range(J):
            assert _eq(got[1][j], want_a[j]), ("grad_a", j, case)
            assert _eq(got[2][j], want_b[j]), ("grad_b", j, case)
            assert _eq(got[3][j], want_c[j]), ("grad_c", j, case)
        assert _eq(got[0], want_x), ("grad_x", case)
        again = _hip.fused_shs_stacked_bwd(gy, x, a, b, c, S, B, shared=shared)
        for u, v in zip(got, again):
            assert _eq(u, v), ("second call", case)
        skipped = _hip.fused_shs_stacked_bwd(gy, x, a, b, c, S, B, shared=shared, need_x=False)
        assert skipped[0] is None
        for u, v in zip(got[1:], skipped[1:]):
            assert _eq(u, v), ("need_x=False", case)


# ---- 2. float64 ----------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("shared", (False, True), ids=("own_x", "shared_x"))
@pytest.mark.parametrize("log2d,J", SHIPPED)
def test_gradients_against_float64(log2d, J, shared, hip_lib):
    from whvi_amd import _hip
    dev = torch.device("cuda")
    D = 1 << log2d
    for S, B in ((3, 5), (2, 777)):
        x, gy, a, b, c = _operands(log2d, J, S, B, shared, dev)
        ref = _ref64(x, gy, a, b, c, S, B, shared)
        # the per-block route first, as FastfoodStackedFunction's loop forms it: each block's grad_x folded, then added
        _, each_x, pb_a, pb_b, pb_c = _per_block(gy, x, a, b, c, S, B, shared)
        pb_x = None
        for g in each_x:
            g = g.view(S, B, D).sum(dim=0) if shared else g
            pb_x = g if pb_x is None else pb_x + g
        got = _hip.fused_shs_stacked_bwd(gy, x, a, b, c, S, B, shared=shared)
        got_x = got[0].view(S, B, D).sum(dim=0) if shared else got[0]
        ratios = {name: (_ratio(new, r), _ratio(old, r))
                  for name, new, old, r in zip("xabc", (got_x,) + tuple(got[1:]), (pb_x, pb_a, pb_b, pb_c), ref)}
        print(f"stacked_bwd D={D} J={J} S={S} B={B} shared={shared} ratios (launch, per-block): " +
              " ".join(f"{k}={v[0]:.2e}/{v[1]:.2e}" for k, v in ratios.items()))
        for name, (new, old) in ratios.items():
            if old > BOUND:
                print(f"stacked_bwd D={D} J={J} S={S} B={B} shared={shared}: the per-block route misses the bound on grad_{name} "
                      f"({old:.2e}); the launch gives {new:.2e}")
                continue
            assert new <= BOUND, (name, new, old)


# ---- 3. routing ----------------------------------------------------------------------------------------------------------------
def _backward_kernel(layer, x, S, hook_on=None):
    """The library's last kernel on the autograd thread once the backward of ``layer.forward_mc(x, S)`` has produced the gradient
    of ``hook_on`` (default: the input)."""
    from whvi_amd import _hip
    seen = []
    x = x.detach().clone().requires_grad_(hook_on is None)
    handle = (x if hook_on is None else hook_on).register_hook(lambda grad: seen.append(_hip.last_kernel()))
    layer.zero_grad()
    torch.manual_seed(5)
    _hip.fwht_rows(torch.zeros(1, 4, device=x.device))                      # (another kernel's name in this thread's note)
    layer.forward_mc(x, S).float().square().sum().backward()
    handle.remove()
    assert len(seen) == 1, seen
    return seen[0]


def test_routing(monkeypatch, hip_lib):
    dev = torch.device("cuda")
    S, B = 3, 7
    gen = torch.Generator().manual_seed(9)
    layer = make_layer(128, 512).to(dev)
    sub = layer.weight_submodule
    x3, x2 = torch.randn(S, B, 128, generator=gen).to(dev), torch.randn(B, 128, generator=gen).to(dev)
    sub.fused_backward = True
    assert f"{KERNEL}<float, 7, 4, 4," in _backward_kernel(layer, x3, S)
    # a shared input that wants no gradient (a network's first layer) takes the launch; one that wants a gradient keeps the loop
    assert f"{KERNEL}<float, 7, 4, 4," in _backward_kernel(layer, x2, S, hook_on=sub.weight_matrices[0].s1)
    assert KERNEL not in _backward_kernel(layer, x2, S)
    sub.fused_backward = False
    assert KERNEL not in _backward_kernel(layer, x3, S)
    # refused with the flag on: five blocks, one block, float64 -- and still within the float64 bound
    for n_in, n_out, double in ((512, 2560, False), (128, 128, False), (128, 512, True)):
        layer = make_layer(n_in, n_out).to(dev)
        if double:
            layer = layer.double()
        sub = layer.weight_submodule
        sub.fused_backward = True
        assert sub.stack == -(-n_out // n_in)
        x = torch.randn(S, B, n_in, generator=gen, dtype=torch.float64 if double else torch.float32).to(dev)
        assert KERNEL not in _backward_kernel(layer, x, S), (n_in, n_out, double)
        check_layer_against_dense(layer, x, S, monkeypatch, grad_tol=1e-12 if double else BOUND)


def test_keep_half_keeps_the_per_block_route(hip_lib):
    """16-bit activations with ``keep_half``: the per-block 16-bit launches, not the new kernel.  The parameter gradients are
    float32 sums of exactly upcast operands and meet the 1e-5 bound; ``grad_x`` is stored as float16 once per block and the J
    blocks are added in float16 -- J + (J - 1) roundings of at most 2^-11 relative each -- so its bound is
    1e-5 + (2 J - 1) 2^-11."""
    from whvi_amd import _hip
    from whvi_amd.fastfood import FastfoodStackedFunction
    dev = torch.device("cuda")
    log2d, J, S, B = 7, 4, 3, 5
    D = 1 << log2d
    x, gy, a, b, c = _operands(log2d, J, S, B, False, dev)
    x, gy = x.half(), gy.half()
    leaves = [t.clone().requires_grad_() for t in (x, a, b, c)]
    seen = []
    leaves[0].register_hook(lambda grad: seen.append(_hip.last_kernel()))
    y = FastfoodStackedFunction.apply(*leaves, S, B, False, True, True)
    assert y.dtype == torch.float16
    y.backward(gy)
    assert len(seen) == 1 and KERNEL not in seen[0] and "fused_shs_bwd_kernel<__half" in seen[0], seen
    ref = _ref64(x.float(), gy.float(), a, b, c, S, B, False)
    for name, leaf, r in zip("xabc", leaves, ref):
        bound = BOUND + (2 * J - 1) * 2.0 ** -11 if name == "x" else BOUND
        assert _ratio(leaf.grad, r) <= bound, (name, _ratio(leaf.grad, r))


# ---- 4. the Module -------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("n_in,n_out", [(128, 512), (100, 256), (1024, 4096), (128, 200)])
def test_module_bit_equal_to_the_per_block_launches(n_in, n_out, monkeypatch, hip_lib):
    """(100, 256): a padded input; (128, 200): a narrowed output, whose grad_y tail is zeros."""
    from whvi_amd import _hip
    dev = torch.device("cuda")
    S, B = 3, 65
    gen = torch.Generator().manual_seed(n_in + n_out)
    layer = make_layer(n_in, n_out, bias=True).to(dev)
    sub = layer.weight_submodule
    sub.fused_backward = True
    assert _hip.fused_shs_stacked_bwd_supported(torch.float32, sub.D_in, sub.stack)
    for shape in ((B, n_in), (S, B, n_in)):
        x0 = torch.randn(*shape, generator=gen).to(dev)
        w = torch.randn(S, B, n_out, generator=gen).to(dev)
        results, kernels = {}, {}
        for launch in (True, False):
            if not launch:
                monkeypatch.setattr(_hip, "fused_shs_stacked_bwd_supported", lambda *args: False)
            x = x0.clone().requires_grad_()
            seen = []
            x.register_hook(lambda grad: seen.append(_hip.last_kernel()))
            layer.zero_grad()
            torch.manual_seed(21)
            y = layer.forward_mc(x, S)
            (y * w).sum().backward()
            monkeypatch.undo()
            kernels[launch] = seen[0]
            results[launch] = [y.detach(), x.grad] + [p.grad for p in layer.parameters()]
        assert KERNEL not in kernels[False]
        assert (KERNEL in kernels[True]) == (len(shape) == 3)       # (a shared input that wants a gradient keeps the loop)
        names = ["y", "x"] + [n for n, _ in layer.named_parameters()]
        for name, u, v in zip(names, results[True], results[False]):
            assert u is not None and _eq(u, v), (name, shape)
        if len(shape) == 2:
            # the same input as data (no gradient wanted): the launch, and the parameter gradients' bits again
            layer.zero_grad()
            seen = []
            first = sub.weight_matrices[0].s1
            handle = first.register_hook(lambda grad: seen.append(_hip.last_kernel()))
            torch.manual_seed(21)
            (layer.forward_mc(x0, S) * w).sum().backward()
            handle.remove()
            assert len(seen) == 1 and KERNEL in seen[0], seen
            for name, p, v in zip(names[2:], layer.parameters(), results[False][2:]):
                assert _eq(p.grad, v), (name, "no input gradient")


# ---- 5. graph capture and peak memory ------------------------------------------------------------------------------------------
def test_graph_capture_and_replay(hip_lib):
    from whvi_amd import _hip
    dev = torch.device("cuda")
    log2d, J, S, B = 10, 4, 2, 64                                     # the (1024, 4096) layer
    x, gy, a, b, c = _operands(log2d, J, S, B, False, dev)
    eager = _hip.fused_shs_stacked_bwd(gy, x, a, b, c, S, B)
    side = torch.cuda.Stream()
    side.wait_stream(torch.cuda.current_stream())
    with torch.cuda.stream(side):
        _hip.fused_shs_stacked_bwd(gy, x, a, b, c, S, B)
    torch.cuda.current_stream().wait_stream(side)
    graph = torch.cuda.CUDAGraph()
    with torch.cuda.graph(graph):
        captured = _hip.fused_shs_stacked_bwd(gy, x, a, b, c, S, B)
    for _ in range(2):
        for t in captured:
            t.zero_()
        graph.replay()
        torch.cuda.synchronize()
        for u, v in zip(captured, eager):
            assert _eq(u, v)


def test_memory(monkeypatch, hip_lib):
    """D = 1024, J = 4, S = 8, B = 4096: one (rows, D) activation is A = 128 MiB.  Peak above what is held before the backward: the
    launch allocates grad_x, the workspace and the parameter gradients; the per-block loop holds a segment's copy, a block's
    grad_x and the running sum."""
    from whvi_amd import _hip
    from whvi_amd.fastfood import FastfoodStackedFunction
    dev = torch.device("cuda")
    D, J, S, B = 1024, 4, 8, 4096
    A = S * B * D * 4
    g = torch.Generator(device=dev).manual_seed(3)
    x = torch.randn(S * B, D, device=dev, generator=g)
    gy = torch.randn(S * B, J * D, device=dev, generator=g)
    a, c = torch.randn(J, D, device=dev, generator=g), torch.randn(J, D, device=dev, generator=g)
    b = torch.randn(J, S, D, device=dev, generator=g)
    work = int(_hip.lib().whvi_fused_shs_stacked_bwd_workspace(S, B, 10, J))
    peaks = {}
    for launch in (True, False):
        if not launch:
            monkeypatch.setattr(_hip, "fused_shs_stacked_bwd_supported", lambda *args: False)
        leaves = [t.clone().requires_grad_() for t in (x, a, b, c)]
        y = FastfoodStackedFunction.apply(*leaves, S, B, False, False, True)
        torch.cuda.synchronize()
        torch.cuda.reset_peak_memory_stats(dev)
        held = torch.cuda.memory_allocated(dev)
        y.backward(gy)
        torch.cuda.synchronize()
        peaks[launch] = torch.cuda.max_memory_allocated(dev) - held
        del leaves, y
    monkeypatch.undo()
    print(f"stacked_bwd memory: A = {A >> 20} MiB, workspace {work} B, peak launch {peaks[True] / A:.3f} A, per-block "
          f"{peaks[False] / A:.3f} A")
    assert peaks[True] <= A + work + (4 << 20), peaks
    assert peaks[False] >= 2 * A, peaks
