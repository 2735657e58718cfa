"""The rectangular fastfood layer with its epilogue in the one launch, on the GPU: whvi_fused_shs_stacked_layer_f32 bit for bit
against ``relu?(fused_shs_stacked(relu?(x)) + bias?)[:, :n_cols]`` (every supported D, own and shared input, a pitch wider than
n_cols inside a guarded buffer, every combination of the three options, non-finite inputs, repeatability), the Module's
routing under ``fused_epilogue``, its gradients against the flag-off route (bit for bit) and float64 (the bias), a network
whose ReLU is folded, one graph capture and the allocator's peak."""
import pytest
import torch
import torch.nn as nn

from whvi_amd.layers import WHVILinear
from whvi_amd.networks import WHVIRegression

from test_fastfood_stacked_gpu import GUARD, SENTINEL, _assert_same, _operands
from test_fastfood_stacked_host import MODE, dense_reference, make_layer
from test_host import ReplayRandn

pytestmark = pytest.mark.gpu

NEW, OLD = "fused_shs_stacked_layer_kernel<float, ", "fused_shs_stacked_kernel<float, "


def _bias(J, D, dev, seed=0):
    return torch.randn(J * D, generator=torch.Generator().manual_seed(77 + 10 * J + D + seed)).to(dev)


def _want(x, a, b, c, S, B, shared, bias, n_cols, relu_in, relu_out):
    from whvi_amd import _hip
    y = _hip.fused_shs_stacked(torch.relu(x) if relu_in else x, a, b, c, S, B, shared=shared)
    if bias is not None:
        y = y + bias
    return (torch.relu(y) if relu_out else y)[:, :n_cols]


def _layer_into_guarded(x, a, b, c, S, B, shared, bias, n_cols, ld, relu_in, relu_out):
    """The launch into rows of pitch ``ld`` inside a sentinel-filled buffer: the guards and the ``ld - n_cols`` gap columns of
    every row must still hold the sentinel."""
    from whvi_amd import _hip
    rows = S * B
    big = torch.full((GUARD + rows * ld + GUARD,), SENTINEL, device=x.device)
    pitched = big[GUARD:GUARD + rows * ld].view(rows, ld)
    dst = pitched[:, :n_cols]
    out = _hip.fused_shs_stacked_layer(x, a, b, c, S, B, bias=bias, n_cols=n_cols, relu_in=relu_in, relu_out=relu_out, shared=shared,
                                       out=dst)
    assert out.data_ptr() == dst.data_ptr() and out.shape == (rows, n_cols)
    assert bool((big[:GUARD] == SENTINEL).all()) and bool((big[GUARD + rows * ld:] == SENTINEL).all()), "a guard was written"
    assert bool((pitched[:, n_cols:] == SENTINEL).all()), "a gap column was written"
    return dst


@pytest.mark.parametrize("log2d", [6, 7, 8, 9, 10, 11])
def test_raw_call_bit_equal_to_the_separate_passes(log2d, hip_lib):
    from whvi_amd import _hip
    dev = torch.device("cuda")
    D = 1 << log2d
    most = 65536 // (16 * D)                     # the bias rule
    for J in sorted({j for j in (1, 2, 3, min(most, 5)) if j <= most}):
        assert _hip.fused_shs_stacked_layer_supported(torch.float32, D, J, True)
        bias = _bias(J, D, dev)
        n_cols = (J - 1) * D + D // 2 + 4
        for S, B in ((1, 1), (3, 5), (2, 777), (4, 64)):
            for shared in (False, True):
                x, a, b, c = _operands(log2d, J, S, B, shared, dev)
                got = _layer_into_guarded(x, a, b, c, S, B, shared, bias, n_cols, n_cols + 8, True, True)
                assert NEW + "%d, " % log2d in _hip.last_kernel()
                want = _want(x, a, b, c, S, B, shared, bias, n_cols, True, True)
                assert bool(torch.isfinite(want).all()) and bool((want > 0).any()) and bool((want == 0).any())
                _assert_same(got, want)
                again = _layer_into_guarded(x, a, b, c, S, B, shared, bias, n_cols, n_cols + 8, True, True)
                assert torch.equal(got.contiguous().view(torch.int32), again.contiguous().view(torch.int32))
                if (S, B) != (3, 5):
                    continue
                for cols in (J * D, J * D - 4, (J - 1) * D + 4):
                    for with_bias in (False, True):
                        for relu_in in (False, True):
                            for relu_out in (False, True):
                                h = bias if with_bias else None
                                got = _layer_into_guarded(x, a, b, c, S, B, shared, h, cols, cols, relu_in, relu_out)
                                _assert_same(got, _want(x, a, b, c, S, B, shared, h, cols, relu_in, relu_out))
                # no option at all: the bits of the launch without an epilogue
                plain = _hip.fused_shs_stacked_layer(x, a, b, c, S, B, shared=shared)
                assert plain.shape == (S * B, J * D) and plain.is_contiguous()
                assert torch.equal(plain.view(torch.int32), _hip.fused_shs_stacked(x, a, b, c, S, B, shared=shared).view(torch.int32))


@pytest.mark.parametrize("log2d", [6, 9, 10, 11])
def test_non_finite_inputs(log2d, hip_lib):
    dev = torch.device("cuda")
    D = 1 << log2d
    J, S, B = min(65536 // (16 * D), 3), 3, 5
    n_cols = (J - 1) * D + D // 2 + 4
    for shared in (False, True):
        x, a, b, c = _operands(log2d, J, S, B, shared, dev, seed=7)
        bias = _bias(J, D, dev, seed=1)
        x[1, 3], x[1, D - 2], x[x.size(0) - 1, 0], x[x.size(0) - 1, D // 2] = float("inf"), float("-inf"), float("nan"), float("inf")
        bias[5] = float("nan")
        got = _layer_into_guarded(x, a, b, c, S, B, shared, bias, n_cols, n_cols + 8, True, True)
        want = _want(x, a, b, c, S, B, shared, bias, n_cols, True, True)
        assert bool(torch.isnan(want[:, 5]).all()) and bool(torch.isnan(want[1]).any()) and bool(torch.isfinite(want).any())
        _assert_same(got, want)                                            # (NaN survives both ReLUs where the reference has it)
        again = _layer_into_guarded(x, a, b, c, S, B, shared, bias, n_cols, n_cols + 8, True, True)
        _assert_same(again, got)


def _forward(layer, x, S, flag, seed=31, **relus):
    """``(output, kernel named)`` of one batched pass under ``seed``, another kernel launched first."""
    from whvi_amd import _hip
    layer.weight_submodule.fused_epilogue = flag
    _hip.fwht_rows(torch.zeros(1, 4, device=x.device))                      # (another kernel's name in the note)
    torch.manual_seed(seed)
    with torch.no_grad():
        y = layer.forward_mc(x, S, **relus)
    return y, _hip.last_kernel()


def test_routing(hip_lib):
    dev = torch.device("cuda")
    S, B = 2, 9
    gen = torch.Generator().manual_seed(4)
    xs = lambda n_in, dtype=torch.float32: [torch.randn(B, n_in, generator=gen).to(dev, dtype),          # noqa: E731
                                            torch.randn(S, B, n_in, generator=gen).to(dev, dtype)]
    # folded: a bias at (128, 512); n_out = 200 written at pitch 200; n_out = 250 at pitch D_out behind the narrowing view
    for n_in, n_out in ((128, 512), (128, 200), (100, 250)):
        layer = make_layer(n_in, n_out).to(dev)
        sub = layer.weight_submodule
        for x in xs(n_in):
            for relus in ({}, {"relu_out": True}, {"relu_in": True, "relu_out": True}):
                y, name = _forward(layer, x, S, True, **relus)
                assert NEW + "7, 4, false>" in name, (n_in, n_out, name)
                assert layer.fuses_relu(x)
                ref, ref_name = _forward(layer, x, S, False, **relus)
                assert NEW not in ref_name and not layer.fuses_relu(x)
                assert y.shape == ref.shape == (S, B, n_out) and torch.equal(y, ref)
                if n_out % 4 == 0:
                    assert y.is_contiguous() and y.size(-1) == n_out and y.stride(1) == n_out
                else:
                    assert y.stride(1) == sub.D_out == 256 and not y.is_contiguous()
    # a narrowing alone is folded too (no bias, no ReLU, 200 % 4 == 0) ...
    layer = make_layer(128, 200, bias=False).to(dev)
    for x in xs(128):
        y, name = _forward(layer, x, S, True)
        assert NEW in name and y.is_contiguous() and torch.equal(y, _forward(layer, x, S, False)[0])
    # ... and with nothing to fold the layer takes the launch it took: no bias, no ReLU, n_out == D_out
    layer = make_layer(128, 512, bias=False).to(dev)
    for x in xs(128):
        y, name = _forward(layer, x, S, True)
        assert NEW not in name and OLD in name
        assert torch.equal(y, _forward(layer, x, S, False)[0])
    # not folded, same values: float64; keep_half with fp16 input; five blocks of 1024 with a bias (beyond the LDS rule)
    cases = [(make_layer(128, 512).to(dev).double(), xs(128, torch.float64), False),
             (make_layer(128, 512).to(dev), xs(128, torch.float16), True),
             (make_layer(1024, 5120).to(dev), xs(1024), False)]
    for layer, inputs, keep_half in cases:
        layer.weight_submodule.keep_half = keep_half
        for x in inputs:
            for relus in ({}, {"relu_in": True, "relu_out": True}):
                y, name = _forward(layer, x, S, True, **relus)
                assert NEW not in name, name
                assert not layer.fuses_relu(x)
                ref, _ = _forward(layer, x, S, False, **relus)
                assert y.dtype == ref.dtype and torch.equal(y, ref)
        assert not keep_half or y.dtype == torch.float16


@pytest.mark.parametrize("fused_backward", [False, True])
@pytest.mark.parametrize("n_out", [512, 200])
def test_gradients(n_out, fused_backward, monkeypatch, hip_lib):
    """``x, s1, s2, g_mu, g_rho``: the bits of the flag-off route with ``torch.relu`` around the layer (both routes hand the same
    ``g`` to the same backward launches).  The bias: max|got - ref64| <= 1e-5 * max|ref64| against float64 autograd of the dense
    product, the bound tests/test_fastfood_stacked_gpu.py holds the backward routes to."""
    from whvi_amd import _hip
    dev = torch.device("cuda")
    S, B, n_in = 3, 65, 128
    layer = make_layer(n_in, n_out).to(dev)
    sub = layer.weight_submodule
    sub.fused_backward = fused_backward
    eps = torch.randn(sub.stack, S, sub.D_in, generator=torch.Generator().manual_seed(5))
    names = [n for n, _ in sub.named_parameters()]
    for shape in ((B, n_in), (S, B, n_in)):
        x = torch.randn(shape, generator=torch.Generator().manual_seed(8)).to(dev)
        w = torch.randn(S, B, n_out, generator=torch.Generator().manual_seed(6)).to(dev)
        grads = {}
        for flag in (False, True):
            sub.fused_epilogue = flag
            xr = x.clone().requires_grad_()
            monkeypatch.setattr(torch, "randn", ReplayRandn([eps.numpy()]))
            _hip.fwht_rows(torch.zeros(1, 4, device=dev))
            y = layer.forward_mc(xr, S, relu_in=True, relu_out=True)
            named = _hip.last_kernel()
            monkeypatch.undo()
            assert (NEW in named) == flag
            grads[flag] = (y.detach(),) + torch.autograd.grad((y * w).sum(), [xr] + list(sub.parameters()))
        assert torch.equal(grads[False][0], grads[True][0])
        for name, p, q in zip(["x"] + names, grads[False][1:], grads[True][1:]):
            assert p.shape == q.shape, name
            if name != "bias":
                assert torch.equal(p, q), name
        # the bias against float64: relu(dense(relu(x)) + bias), its leaves [x, parameters...]
        want, leaves = dense_reference(sub, torch.relu(x), eps.to(dev))
        ref = torch.autograd.grad((torch.relu(want) * w.double()).sum(), leaves[1 + names.index("bias")])[0]
        got, off = grads[True][1 + 1 + names.index("bias")], grads[False][1 + 1 + names.index("bias")]
        ratio = float((got.double() - ref).abs().max()) / float(ref.abs().max())
        print(f"n_out={n_out} fused_backward={fused_backward} x{tuple(shape)}: bias gradient error / max|ref64| = {ratio:.3e}; "
              f"bit-equal to the flag-off route: {torch.equal(got, off)}")
        assert got.shape == ref.shape == (1, sub.D_out)
        assert bool((got[0, n_out:] == 0).all())
        assert ratio <= 1e-5


def test_network_folds_the_relu(monkeypatch, hip_lib):
    dev = torch.device("cuda")
    S, B = 4, 33
    torch.manual_seed(0)
    relus = [nn.ReLU(), nn.ReLU()]
    net = WHVIRegression([WHVILinear(6, 128), relus[0], WHVILinear(128, 200, mode=MODE, bias=True), relus[1],
                          WHVILinear(200, 1, mode=MODE)], train_samples=S, eval_samples=S).to(dev)
    mid = net.sequential[2]
    stacked = [m.weight_submodule for m in net.sequential if isinstance(m, WHVILinear)
               and type(m.weight_submodule).__name__ == "WHVIFastfoodStackedMatrix"]
    assert len(stacked) == 2 and mid.weight_submodule is stacked[0]
    x = torch.randn(B, 6, generator=torch.Generator().manual_seed(1)).to(dev)
    calls, ran = [], [0, 0]
    real = mid.forward_mc
    monkeypatch.setattr(mid, "forward_mc", lambda h, n, **kw: (calls.append(kw), real(h, n, **kw))[1])
    for i, r in enumerate(relus):
        r.register_forward_hook(lambda m, a, o, i=i: ran.__setitem__(i, ran[i] + 1))
    out = {}
    for flag in (False, True):
        for s in stacked:
            s.fused_epilogue = flag
        del calls[:]
        ran[:] = [0, 0]
        torch.manual_seed(2)
        with torch.no_grad():
            out[flag] = net.forward_batched(x, S)
        if flag:
            assert len(calls) == 1 and calls[0].get("relu_out") is True, calls
            assert ran[1] == 0, "the ReLU behind the folding layer ran as a pass of its own"
        else:
            assert len(calls) == 1 and not calls[0].get("relu_out"), calls
            assert ran[1] == 1
    assert out[True].shape == (B, 1, S) and torch.equal(out[True], out[False])


def test_graph_capture_and_replay(hip_lib):
    from whvi_amd import _hip
    dev = torch.device("cuda")
    log2d, J, S, B = 10, 4, 2, 64                                     # the (1024, 4096) layer
    x, a, b, c = _operands(log2d, J, S, B, False, dev)
    bias = _bias(J, 1 << log2d, dev)
    kw = dict(bias=bias, relu_in=True, relu_out=True)
    eager = _hip.fused_shs_stacked_layer(x, a, b, c, S, B, **kw)
    _assert_same(eager, _want(x, a, b, c, S, B, False, bias, J << log2d, True, True))
    y = torch.zeros_like(eager)
    side = torch.cuda.Stream()
    side.wait_stream(torch.cuda.current_stream())
    with torch.cuda.stream(side):
        _hip.fused_shs_stacked_layer(x, a, b, c, S, B, out=y, **kw)
    torch.cuda.current_stream().wait_stream(side)
    graph = torch.cuda.CUDAGraph()
    with torch.cuda.graph(graph):
        _hip.fused_shs_stacked_layer(x, a, b, c, S, B, out=y, **kw)
    for _ in range(2):
        y.zero_()
        graph.replay()
        torch.cuda.synchronize()
        assert torch.equal(y.view(torch.int32), eager.view(torch.int32))


def test_peak_memory_of_the_forward(hip_lib):
    dev = torch.device("cuda")
    S, B = 8, 4096
    layer = make_layer(1024, 4096).to(dev)
    x = torch.randn(S, B, 1024, generator=torch.Generator().manual_seed(3)).to(dev)
    peak = {}
    for flag in (False, True):
        layer.weight_submodule.fused_epilogue = flag
        torch.manual_seed(4)
        torch.cuda.synchronize()
        torch.cuda.empty_cache()
        torch.cuda.reset_peak_memory_stats()
        base = torch.cuda.memory_allocated()
        with torch.no_grad():
            y = layer.forward_mc(x, S, relu_out=True)
        torch.cuda.synchronize()
        peak[flag] = torch.cuda.max_memory_allocated() - base
        assert y.shape == (S, B, 4096)
        del y
    print(f"forward peak above the inputs, D = 1024, J = 4, S = 8, B = 4096, bias + ReLU: flag on {peak[True] / 2**20:.0f} MiB, "
          f"flag off {peak[False] / 2**20:.0f} MiB")
    assert peak[True] < peak[False]
