"""The one-launch backward of the rectangular fastfood layer with its epilogue, on the GPU
(whvi_fused_shs_stacked_layer_bwd_f32, ``FastfoodStackedLayerFunction(..., fused_backward=True, fused_epilogue_backward=True)``).
The reference is the composed backward: ``threshold_backward`` on ``grad_y``, ``F.pad`` to ``J * D`` columns,
``_hip.fused_shs_stacked_bwd`` on ``relu(x)``, ``threshold_backward`` on ``grad_x`` -- ``grad_x`` and the gradients of ``a, b, c``
bit for bit, the bias gradient within ``1e-5 * max|ref64|`` of the float64 column sum of the masked gradient (the bound
tests/test_fastfood_stacked_layer_gpu.py holds this tensor to).  Then non-finite inputs, the Module's routing, its gradients,
a network, one graph capture and the allocator's peak."""
import pytest
import torch
import torch.nn as nn
import torch.nn.functional as F

from whvi_amd.layers import WHVILinear
from whvi_amd.networks import WHVIRegression

from test_fastfood_stacked_gpu import GUARD, SENTINEL, _assert_same, _operands
from test_fastfood_stacked_host import MODE, dense_reference, make_layer
from test_host import ReplayRandn

pytestmark = pytest.mark.gpu

KERNEL = "fused_shs_stacked_layer_bwd_kernel"
BOUND = 1e-5
NAN = float("nan")


def _rule(log2d, J):
    return (6 <= log2d <= 10 and 2 <= J <= 4) or (log2d == 11 and J == 2)


def _pitched(rows, n_cols, ld, dev):
    """``(rows, n_cols)`` view at pitch ``ld`` inside a NaN-filled buffer: the gap columns and the surroundings hold NaN."""
    big = torch.full((GUARD + rows * ld + GUARD,), NAN, device=dev)
    return big[GUARD:GUARD + rows * ld].view(rows, ld)[:, :n_cols]


def _inputs(log2d, J, S, B, shared, n_cols, ld, dev, relu_in=True, relu_out=True, seed=0):
    """``x, a, b, c, bias, grad_y, y``: ``grad_y`` and ``y`` slices of NaN-filled buffers, ``y`` written by the forward launch."""
    from whvi_amd import _hip
    D = 1 << log2d
    x, a, b, c = _operands(log2d, J, S, B, shared, dev, seed=seed)
    bias = torch.randn(J * D, generator=torch.Generator().manual_seed(7 + log2d + J + seed)).to(dev)
    gy = _pitched(S * B, n_cols, ld, dev)
    gy.copy_(torch.randn(S * B, n_cols, generator=torch.Generator().manual_seed(11 * log2d + J + S + B + seed)).to(dev))
    y = _hip.fused_shs_stacked_layer(x, a, b, c, S, B, bias=bias, n_cols=n_cols, relu_in=relu_in, relu_out=relu_out, shared=shared,
                                     out=_pitched(S * B, n_cols, ld, dev))
    return x, a, b, c, bias, gy, y


def _reference(gy, y, x, a, b, c, S, B, shared, relu_in, relu_out, need_x):
    """The composed backward: ``(grad_x | None, grad_a, grad_b, grad_c, masked zero-padded g)``."""
    from whvi_amd import _hip
    J, D = a.shape
    g = (torch.ops.aten.threshold_backward(gy, y, 0) if relu_out else gy).contiguous()
    if g.size(1) < J * D:
        g = F.pad(g, (0, J * D - g.size(1)))
    xin = torch.relu(x) if relu_in else x
    gx, ga, gb, gc = _hip.fused_shs_stacked_bwd(g, xin, a, b, c, S, B, shared=shared, need_x=need_x)
    if relu_in and gx is not None:
        gx = torch.ops.aten.threshold_backward(gx, xin, 0)
    return gx, ga, gb, gc, g


def _launch(gy, y, x, a, b, c, S, B, shared, relu_in, relu_out, need_x, need_bias):
    """The new call, ``grad_x`` written into a guarded slice of a sentinel-filled buffer; the guards must be intact."""
    from whvi_amd import _hip
    rows, D = S * B, a.size(1)
    big = torch.full((GUARD + rows * D + GUARD,), SENTINEL, device=x.device)
    dst = big[GUARD:GUARD + rows * D].view(rows, D)
    _hip.fwht_rows(torch.zeros(1, 4, device=x.device))                      # (another kernel's name in the note)
    out = _hip.fused_shs_stacked_layer_bwd(gy, y if relu_out else None, x, a, b, c, S, B, n_cols=gy.size(1), relu_in=relu_in,
                                           relu_out=relu_out, shared=shared, need_x=need_x, need_bias=need_bias,
                                           grad_x=dst if need_x else None)
    assert bool((big[:GUARD] == SENTINEL).all()) and bool((big[GUARD + rows * D:] == SENTINEL).all()), "a guard was written"
    if need_x:
        assert out[0].data_ptr() == dst.data_ptr()
    else:
        assert out[0] is None and bool((dst == SENTINEL).all())
    assert (out[4] is not None) == need_bias
    return out


def _check_bias(got, g, n_cols, what):
    ref = g.double().sum(dim=0)
    ratio = float((got.double() - ref).abs().max()) / float(ref.abs().max())
    assert got.shape == ref.shape
    assert torch.equal(got[n_cols:].view(torch.int32), torch.zeros_like(got[n_cols:]).view(torch.int32)), what     # +0.0 exactly
    assert ratio <= BOUND, (what, ratio)
    return ratio


# ---- 1. the raw call -----------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("log2d", [6, 7, 8, 9, 10, 11])
def test_raw_call_bit_equal_to_the_composed_backward(log2d, hip_lib):
    from whvi_amd import _hip
    dev = torch.device("cuda")
    D = 1 << log2d
    worst = 0.0
    for J in (2, 3, 4):
        if not _rule(log2d, J):
            continue
        assert _hip.fused_shs_stacked_layer_bwd_supported(torch.float32, D, J, True)
        n_cols = (J - 1) * D + D // 2 + 4
        for S, B in ((1, 1), (3, 5), (2, 777), (4, 64)):
            for shared in (False, True):
                need_x = not shared
                x, a, b, c, bias, gy, y = _inputs(log2d, J, S, B, shared, n_cols, n_cols + 8, dev)
                assert gy.stride(0) == y.stride(0) == n_cols + 8
                got = _launch(gy, y, x, a, b, c, S, B, shared, True, True, need_x, True)
                assert _hip.last_kernel() == f"whvi::{KERNEL}<float, {log2d}, {8 if log2d == 11 else 4}, {J}, true, false>"
                want = _reference(gy, y, x, a, b, c, S, B, shared, True, True, need_x)
                assert bool(torch.isfinite(want[4]).all()) and bool((want[4] == 0).any()) and bool((want[4] != 0).any())
                for name, u, v in zip(("grad_x", "grad_a", "grad_b", "grad_c"), got, want):
                    assert (u is None and v is None) or torch.equal(u, v), (name, J, S, B, shared)
                worst = max(worst, _check_bias(got[4], want[4], n_cols, (J, S, B, shared)))
                again = _launch(gy, y, x, a, b, c, S, B, shared, True, True, need_x, True)
                for u, v in zip(got, again):
                    assert (u is None and v is None) or torch.equal(u.view(torch.int32), v.view(torch.int32))
                if (S, B) != (3, 5):
                    continue
                for cols in (J * D, J * D - 4, (J - 1) * D + 4):
                    for relu_in in (False, True):
                        for relu_out in (False, True):
                            x, a, b, c, bias, gy, y = _inputs(log2d, J, S, B, shared, cols, cols, dev, relu_in, relu_out)
                            for with_x in ((False, True) if not shared else (False,)):
                                want = _reference(gy, y, x, a, b, c, S, B, shared, relu_in, relu_out, with_x)
                                for need_bias in (False, True):
                                    got = _launch(gy, y, x, a, b, c, S, B, shared, relu_in, relu_out, with_x, need_bias)
                                    what = (J, cols, relu_in, relu_out, with_x, need_bias, shared)
                                    assert f"{J}, {'true' if need_bias else 'false'}, false>" in _hip.last_kernel(), what
                                    for u, v in zip(got[:4], want):
                                        assert (u is None and v is None) or torch.equal(u, v), what
                                    if need_bias:
                                        worst = max(worst, _check_bias(got[4], want[4], cols, what))
                # no option, no bias, n_cols == ld == J D: the launch without an epilogue
                x, a, b, c, bias, gy, y = _inputs(log2d, J, S, B, shared, J * D, J * D, dev, False, False)
                got = _hip.fused_shs_stacked_layer_bwd(gy, None, x, a, b, c, S, B, shared=shared, need_x=need_x)
                want = _hip.fused_shs_stacked_bwd(gy, x, a, b, c, S, B, shared=shared, need_x=need_x)
                assert got[4] is None
                for u, v in zip(got[:4], want):
                    assert (u is None and v is None) or torch.equal(u.view(torch.int32), v.view(torch.int32))
    print(f"log2(D) = {log2d}: worst bias gradient error / max|ref64| = {worst:.3e}")


# ---- 2. non-finite inputs ------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("log2d", [6, 9, 10, 11])
def test_non_finite_inputs(log2d, hip_lib):
    dev = torch.device("cuda")
    D = 1 << log2d
    J, S, B = (2 if log2d == 11 else 3), 3, 5
    n_cols = (J - 1) * D + D // 2 + 4
    inf = float("inf")
    x, a, b, c, bias, gy, y = _inputs(log2d, J, S, B, False, n_cols, n_cols + 8, dev, seed=7)
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
        _assert_same(u, v)
    ref = g.double().sum(dim=0)
    assert torch.equal(torch.isnan(got[4]), torch.isnan(ref)) and torch.equal(torch.isinf(got[4]), torch.isinf(ref))
    fin = torch.isfinite(ref)
    assert float((got[4].double() - ref)[fin].abs().max()) <= BOUND * float(ref[fin].abs().max())
    again = _launch(gy, y, x, a, b, c, S, B, False, True, True, True, True)
    for u, v in zip(got, again):
        _assert_same(u, v)


# ---- 3. routing ----------------------------------------------------------------------------------------------------------------
def _backward(layer, x, S, flags, want_x=True, hook_on=None):
    """``(kernel named when the gradient of x -- or of hook_on -- is produced, y, x.grad, parameter gradients)`` of
    ``relu(layer(relu(x)))`` under seed 5 with ``fused_epilogue, fused_backward, fused_epilogue_backward = flags``."""
    from whvi_amd import _hip
    sub = layer.weight_submodule
    sub.fused_epilogue, sub.fused_backward, sub.fused_epilogue_backward = flags
    seen = []
    x = x.detach().clone().requires_grad_(want_x)
    handle = (x if hook_on is None else hook_on).register_hook(lambda grad: seen.append(_hip.last_kernel()))
    layer.zero_grad()
    torch.manual_seed(5)
    _hip.fwht_rows(torch.zeros(1, 4, device=x.device))                      # (another kernel's name in this thread's note)
    y = layer.forward_mc(x, S, relu_in=True, relu_out=True)
    w = torch.randn(y.shape, generator=torch.Generator().manual_seed(6)).to(y)
    (y * w).sum().backward()
    handle.remove()
    assert len(seen) == 1, seen
    return seen[0], y.detach(), x.grad, [p.grad.clone() for p in layer.parameters()]


def _same(u, v):
    assert torch.equal(u[1], v[1])
    assert (u[2] is None and v[2] is None) or torch.equal(u[2], v[2])
    assert len(u[3]) == len(v[3])
    for p, q in zip(u[3], v[3]):
        assert torch.equal(p, q)


def test_routing(hip_lib):
    from whvi_amd import _hip
    dev = torch.device("cuda")
    S, B = 3, 7
    gen = torch.Generator().manual_seed(9)
    ON, COMPOSED = (True, True, True), (True, True, False)
    for n_in, n_out, tag in ((128, 512, "7, 4, 4, true, false>"), (128, 200, "7, 4, 2, true, false>")):
        layer = make_layer(n_in, n_out).to(dev)
        s1 = layer.weight_submodule.weight_matrices[0].s1
        x3, x2 = torch.randn(S, B, n_in, generator=gen).to(dev), torch.randn(B, n_in, generator=gen).to(dev)
        assert f"{KERNEL}<float, {tag}" in _backward(layer, x3, S, ON)[0]
        # a 2-D input that is data takes the launch; one that wants a gradient keeps the composed backward
        assert f"{KERNEL}<float, {tag}" in _backward(layer, x2, S, ON, want_x=False, hook_on=s1)[0]
        off = _backward(layer, x2, S, ON)
        assert KERNEL not in off[0]
        _same(off, _backward(layer, x2, S, COMPOSED))
        # either flag off
        for flags in ((True, False, True), (True, True, False), (False, True, True)):
            got = _backward(layer, x3, S, flags)
            assert KERNEL not in got[0], flags
            ref = _backward(layer, x3, S, (flags[0], flags[1], False))
            _same(got, ref)
    # a bias and nothing else to fold (no ReLU, n_out == D_out): the composed backward, whose row sum measured as fast
    layer = make_layer(128, 512).to(dev)
    sub = layer.weight_submodule
    out = {}
    for flags in (ON, COMPOSED):
        sub.fused_epilogue, sub.fused_backward, sub.fused_epilogue_backward = flags
        seen = []
        xr = x3.clone().requires_grad_()
        xr.register_hook(lambda grad: seen.append(_hip.last_kernel()))
        layer.zero_grad()
        torch.manual_seed(5)
        layer.forward_mc(xr, S).square().sum().backward()
        assert len(seen) == 1 and KERNEL not in seen[0]
        out[flags] = [xr.grad] + [p.grad.clone() for p in layer.parameters()]
    for p, q in zip(out[ON], out[COMPOSED]):
        assert torch.equal(p, q)
    # refused with every flag on: five blocks of 512, one block, float64
    for n_in, n_out, double in ((512, 2560, False), (128, 128, False), (128, 512, True)):
        layer = make_layer(n_in, n_out).to(dev)
        if double:
            layer = layer.double()
        assert layer.weight_submodule.stack == -(-n_out // n_in)
        x = torch.randn(S, B, n_in, generator=gen, dtype=torch.float64 if double else torch.float32).to(dev)
        got = _backward(layer, x, S, ON)
        assert KERNEL not in got[0], (n_in, n_out, double)
        _same(got, _backward(layer, x, S, COMPOSED))


@pytest.mark.parametrize("relu_out", [False, True])
def test_gradient_that_is_a_view_of_a_wider_one(relu_out, hip_lib):
    """``torch.cat`` behind the layer: autograd hands the backward a ``(S * B, 512)`` view with row stride 1024.  Without
    ``relu_out`` the launch reads it in place; with it the saved output has pitch 512 and the gradient is copied first.  Either
    way the launch runs and every gradient but the bias has the composed backward's bits (the bias: both routes are within
    ``BOUND`` of float64 at this shape, test_module_gradients, so within twice that of each other)."""
    from whvi_amd import _hip
    dev = torch.device("cuda")
    S, B = 3, 7
    gen = torch.Generator().manual_seed(13)
    layer = make_layer(128, 512).to(dev)
    sub = layer.weight_submodule
    x = torch.randn(S, B, 128, generator=gen).to(dev)
    other = torch.randn(S, B, 512, generator=gen).to(dev)
    w = torch.randn(S, B, 1024, generator=gen).to(dev)
    out = {}
    for flag in (True, False):
        sub.fused_epilogue, sub.fused_backward, sub.fused_epilogue_backward = True, True, flag
        xr = x.clone().requires_grad_()
        seen, strides = [], []
        xr.register_hook(lambda grad: seen.append(_hip.last_kernel()))
        layer.zero_grad()
        torch.manual_seed(5)
        _hip.fwht_rows(torch.zeros(1, 4, device=dev))
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


# ---- 4. the Module -------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("n_in,n_out", [(128, 512), (128, 200), (100, 256), (1024, 4096)])
def test_module_gradients(n_in, n_out, monkeypatch, hip_lib):
    """``x, s1, s2, g_mu, g_rho``: the bits of the composed backward.  The bias: max|got - ref64| <= 1e-5 * max|ref64| against
    float64 autograd of the dense product."""
    from whvi_amd import _hip
    dev = torch.device("cuda")
    S, B = 3, 65
    layer = make_layer(n_in, n_out).to(dev)
    sub = layer.weight_submodule
    sub.fused_epilogue = sub.fused_backward = True
    eps = torch.randn(sub.stack, S, sub.D_in, generator=torch.Generator().manual_seed(5))
    names = [n for n, _ in sub.named_parameters()]
    x = torch.randn(S, B, n_in, generator=torch.Generator().manual_seed(8)).to(dev)
    w = torch.randn(S, B, n_out, generator=torch.Generator().manual_seed(6)).to(dev)
    grads = {}
    for flag in (False, True):
        sub.fused_epilogue_backward = flag
        xr = x.clone().requires_grad_()
        seen = []
        xr.register_hook(lambda grad: seen.append(_hip.last_kernel()))
        monkeypatch.setattr(torch, "randn", ReplayRandn([eps.numpy()]))
        y = layer.forward_mc(xr, S, relu_in=True, relu_out=True)
        monkeypatch.undo()
        grads[flag] = (y.detach(),) + torch.autograd.grad((y * w).sum(), [xr] + list(sub.parameters()))
        assert (KERNEL in seen[0]) == flag, seen
    assert torch.equal(grads[False][0], grads[True][0])
    for name, p, q in zip(["x"] + names, grads[False][1:], grads[True][1:]):
        assert p.shape == q.shape, name
        if name != "bias":
            assert torch.equal(p, q), name
    want, leaves = dense_reference(sub, torch.relu(x), eps.to(dev))
    ref = torch.autograd.grad((torch.relu(want) * w.double()).sum(), leaves[1 + names.index("bias")])[0]
    got, off = grads[True][2 + names.index("bias")], grads[False][2 + names.index("bias")]
    ratio = float((got.double() - ref).abs().max()) / float(ref.abs().max())
    ratio_off = float((off.double() - ref).abs().max()) / float(ref.abs().max())
    print(f"({n_in}, {n_out}): bias gradient error / max|ref64| = {ratio:.3e} (the composed backward: {ratio_off:.3e})")
    assert got.shape == ref.shape == (1, sub.D_out)
    assert bool((got[0, n_out:] == 0).all())
    assert ratio <= BOUND


def test_network_one_training_step(hip_lib):
    """A three-layer network whose middle, rectangular layer takes the launch: every gradient but that layer's bias -- and after
    one SGD step every such parameter -- has the bits of the network with ``fused_epilogue_backward`` off."""
    from whvi_amd import _hip
    dev = torch.device("cuda")
    S, B = 4, 33
    x = torch.randn(B, 6, generator=torch.Generator().manual_seed(1)).to(dev)
    t = torch.randn(B, 1, generator=torch.Generator().manual_seed(2)).to(dev)
    out = {}
    for flag in (False, True):
        torch.manual_seed(0)
        net = WHVIRegression([WHVILinear(6, 128), nn.ReLU(), WHVILinear(128, 200, mode=MODE, bias=True), nn.ReLU(),
                              WHVILinear(200, 1, mode=MODE)], train_samples=S, eval_samples=S).to(dev)
        stacked = [m.weight_submodule for m in net.sequential if isinstance(m, WHVILinear)
                   and type(m.weight_submodule).__name__ == "WHVIFastfoodStackedMatrix"]
        assert len(stacked) == 2
        for s in stacked:
            s.fused_epilogue = s.fused_backward = True
            s.fused_epilogue_backward = flag
        seen = []
        handle = stacked[0].weight_matrices[0].s1.register_hook(lambda grad: seen.append(_hip.last_kernel()))
        net.mc_mode = "batched"
        net.train()
        opt = torch.optim.SGD(net.parameters(), lr=1e-3)
        opt.zero_grad()
        torch.manual_seed(3)
        loss = net.loss(x, t, n=100)
        loss.backward()
        handle.remove()
        assert len(seen) == 1 and (KERNEL in seen[0]) == flag, seen
        grads = {n: p.grad.clone() for n, p in net.named_parameters()}
        opt.step()
        mid_bias = [n for n, p in net.named_parameters() if p is stacked[0].bias]
        assert len(mid_bias) == 1
        out[flag] = (loss.detach(), grads, {n: p.detach().clone() for n, p in net.named_parameters()}, mid_bias[0])
    assert torch.isfinite(out[False][0]) and torch.equal(out[False][0], out[True][0])
    assert out[False][1].keys() == out[True][1].keys() and len(out[True][1]) > 0
    skipped = 0
    for n in out[True][1]:
        if n == out[True][3]:                                          # (the launch's own summation order: test_module_gradients)
            skipped += 1
            continue
        assert torch.equal(out[False][1][n], out[True][1][n]), n
        assert torch.equal(out[False][2][n], out[True][2][n]), n
    assert skipped == 1


# ---- 5. graph capture, 6. peak memory ------------------------------------------------------------------------------------------
def test_graph_capture_and_replay(hip_lib):
    from whvi_amd import _hip
    dev = torch.device("cuda")
    log2d, J, S, B = 10, 4, 2, 64                                     # the (1024, 4096) layer
    x, a, b, c, bias, gy, y = _inputs(log2d, J, S, B, False, J << log2d, J << log2d, dev)
    kw = dict(relu_in=True, relu_out=True, need_bias=True)
    eager = _hip.fused_shs_stacked_layer_bwd(gy, y, x, a, b, c, S, B, **kw)
    want = _reference(gy, y, x, a, b, c, S, B, False, True, True, True)
    for u, v in zip(eager[:4], want):
        assert torch.equal(u, v)
    side = torch.cuda.Stream()
    side.wait_stream(torch.cuda.current_stream())
    with torch.cuda.stream(side):
        _hip.fused_shs_stacked_layer_bwd(gy, y, x, a, b, c, S, B, **kw)
    torch.cuda.current_stream().wait_stream(side)
    graph = torch.cuda.CUDAGraph()
    with torch.cuda.graph(graph):
        captured = _hip.fused_shs_stacked_layer_bwd(gy, y, x, a, b, c, S, B, **kw)
    for _ in range(2):
        for t in captured:
            t.zero_()
        graph.replay()
        torch.cuda.synchronize()
        for u, v in zip(captured, eager):
            assert torch.equal(u.view(torch.int32), v.view(torch.int32))


def test_peak_memory_of_the_backward(hip_lib):
    """D = 1024, J = 4, S = 8, B = 4096 with a bias and both ReLUs: one (rows, D) activation is A = 128 MiB.  Above what is held
    before the backward the launch allocates grad_x, the workspace and the parameter gradients; the composed backward also holds
    the masked gradient (4 A), relu(x) and the unmasked grad_x."""
    from whvi_amd import _hip
    from whvi_amd.fastfood import FastfoodStackedLayerFunction
    dev = torch.device("cuda")
    D, J, S, B = 1024, 4, 8, 4096
    A = S * B * D * 4
    g = torch.Generator(device=dev).manual_seed(3)
    x = torch.randn(S * B, D, device=dev, generator=g)
    gy = torch.randn(S * B, J * D, device=dev, generator=g)
    a, c = torch.randn(J, D, device=dev, generator=g), torch.randn(J, D, device=dev, generator=g)
    b = torch.randn(J, S, D, device=dev, generator=g)
    bias = torch.randn(1, J * D, device=dev, generator=g)
    work = int(_hip.lib().whvi_fused_shs_stacked_layer_bwd_workspace(S, B, 10, J, 1))
    params = (3 * J * D + J * S * D) * 4
    peaks = {}
    for flag in (True, False):
        leaves = [t.clone().requires_grad_() for t in (x, a, b, c, bias)]
        y = FastfoodStackedLayerFunction.apply(*leaves, J * D, True, True, S, B, False, True, flag)
        torch.cuda.synchronize()
        torch.cuda.reset_peak_memory_stats(dev)
        held = torch.cuda.memory_allocated(dev)
        y.backward(gy)
        torch.cuda.synchronize()
        peaks[flag] = torch.cuda.max_memory_allocated(dev) - held
        del leaves, y
    print(f"stacked_layer_bwd memory: A = {A >> 20} MiB, workspace {work >> 20} MiB, peak launch {peaks[True] / A:.3f} A "
          f"({peaks[True] >> 20} MiB), composed {peaks[False] / A:.3f} A ({peaks[False] >> 20} MiB)")
    assert peaks[True] <= A + work + params + (2 << 20), peaks
