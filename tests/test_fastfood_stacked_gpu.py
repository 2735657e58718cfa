"""The rectangular fastfood layer on the GPU: whvi_fused_shs_stacked_f32 bit for bit against the per-block launches of
whvi_fused_shs_f32 (every supported D, own and shared input, guards around dst, non-finite inputs, repeatability), the
Module's routing, the Module and its gradients against the dense float64 product (tests/test_fastfood_stacked_host.py builds
it), and one graph capture."""
import pytest
import torch

from test_fastfood_stacked_host import check_layer_against_dense, make_layer

pytestmark = pytest.mark.gpu

SENTINEL = -777.25
GUARD = 1024                                     # floats on each side of dst


def _operands(log2d, J, S, B, shared, dev, seed=0):
    D = 1 << log2d
    g = torch.Generator().manual_seed(1000 * log2d + 100 * J + 10 * S + B + seed)
    x = torch.randn(B if shared else S * B, D, generator=g).to(dev)
    a, c = (torch.randn(J, D, generator=g).to(dev) for _ in range(2))
    b = torch.randn(J, S, D, generator=g).to(dev)
    return x, a, b, c


def _per_block(x, a, b, c, S, B, shared):
    """``torch.cat`` of the per-block launches (a shared source below the shared form's 1 KiB rows is expanded: the same bits,
    include/whvi_hip.h)."""
    from whvi_amd import _hip
    native = shared and _hip.fused_src_shared_supported(x.dtype, x.size(1))
    src = x.repeat(S, 1) if shared and not native else x
    return torch.cat([_hip.fused_shs(src, a[j], b[j], c[j], axis="col", n_samples=S, sample_stride=B, src_shared=native)
                      for j in range(a.size(0))], dim=1)


def _stacked_into_guarded(x, a, b, c, S, B, shared):
    from whvi_amd import _hip
    n = S * B * a.size(0) * a.size(1)
    big = torch.full((GUARD + n + GUARD,), SENTINEL, device=x.device)
    dst = big[GUARD:GUARD + n].view(S * B, -1)
    out = _hip.fused_shs_stacked(x, a, b, c, S, B, shared=shared, out=dst)
    assert out.data_ptr() == dst.data_ptr()
    assert bool((big[:GUARD] == SENTINEL).all()) and bool((big[GUARD + n:] == SENTINEL).all()), "a guard was written"
    return dst


def _assert_same(got, want):
    nan = torch.isnan(want)
    assert torch.equal(torch.isnan(got), nan)
    assert torch.equal(torch.isinf(got), torch.isinf(want))
    assert torch.equal((got + 0.0)[~nan], (want + 0.0)[~nan])


@pytest.mark.parametrize("log2d", [6, 7, 8, 9, 10, 11])
def test_bit_equal_to_the_per_block_launches(log2d, hip_lib):
    from whvi_amd import _hip
    dev = torch.device("cuda")
    D = 1 << log2d
    most = 65536 // (12 * D)
    for J in sorted({j for j in (1, 2, 3, min(most, 5)) if j <= most}):
        assert _hip.fused_shs_stacked_supported(torch.float32, D, J)
        for S, B in ((1, 1), (3, 5), (2, 777), (4, 64)):
            for shared in (False, True):
                x, a, b, c = _operands(log2d, J, S, B, shared, dev)
                got = _stacked_into_guarded(x, a, b, c, S, B, shared)
                assert "fused_shs_stacked_kernel<float, %d, " % log2d in _hip.last_kernel()
                want = _per_block(x, a, b, c, S, B, shared)
                assert bool(torch.isfinite(want).all())
                _assert_same(got, want)
                again = _stacked_into_guarded(x, a, b, c, S, B, shared)
                assert torch.equal(got.view(torch.int32), again.view(torch.int32))
    # once more with +-inf and NaN planted in two rows of x
    J, S, B = min(most, 3), 3, 5
    for shared in (False, True):
        x, a, b, c = _operands(log2d, J, S, B, shared, dev, seed=7)
        x[1, 3], x[1, D - 2], x[x.size(0) - 1, 0], x[x.size(0) - 1, D // 2] = float("inf"), float("-inf"), float("nan"), float("inf")
        got = _stacked_into_guarded(x, a, b, c, S, B, shared)
        want = _per_block(x, a, b, c, S, B, shared)
        assert bool(torch.isnan(want).any()) and bool(torch.isfinite(want).any())
        _assert_same(got, want)
        again = _stacked_into_guarded(x, a, b, c, S, B, shared)
        _assert_same(again, got)


def test_routing(monkeypatch, hip_lib):
    from whvi_amd import _hip
    dev = torch.device("cuda")
    S, B = 2, 9
    gen = torch.Generator().manual_seed(4)
    layer = make_layer(128, 512).to(dev)
    _hip.fwht_rows(torch.zeros(1, 4, device=dev))                       # (another kernel's name in the note)
    with torch.no_grad():
        for x in (torch.randn(B, 128, generator=gen), torch.randn(S, B, 128, generator=gen)):
            layer.forward_mc(x.to(dev), S)
            assert "whvi::fused_shs_stacked_kernel<float, 7, 4, false>" == _hip.last_kernel()
    # outside the launch's range: the composed route, still within the float64 bound
    for n_in, n_out, double in ((8, 32, False), (1024, 6144, False), (128, 512, True)):
        layer = make_layer(n_in, n_out).to(dev)
        if double:
            layer = layer.double()
        sub = layer.weight_submodule
        assert double or not _hip.fused_shs_stacked_supported(torch.float32, sub.D_in, sub.stack)
        x = torch.randn(B, n_in, generator=gen, dtype=torch.float64 if double else torch.float32).to(dev)
        _hip.fwht_rows(torch.zeros(1, 4, device=dev))
        check_layer_against_dense(layer, x, S, monkeypatch)
        assert "fused_shs_stacked_kernel" not in _hip.last_kernel()


@pytest.mark.parametrize("n_in,n_out", [(128, 512), (128, 200), (100, 256), (256, 2)])
def test_module_against_the_dense_float64_product(n_in, n_out, monkeypatch, hip_lib):
    dev = torch.device("cuda")
    S, B = 3, 7
    gen = torch.Generator().manual_seed(n_in + n_out)
    for bias in (True, False):
        layer = make_layer(n_in, n_out, bias=bias).to(dev)
        for x in (torch.randn(B, n_in, generator=gen), torch.randn(S, B, n_in, generator=gen)):
            check_layer_against_dense(layer, x.to(dev), S, monkeypatch)


@pytest.mark.parametrize("fused_backward", [False, True])
@pytest.mark.parametrize("shared", [True, False])
def test_gradients_against_float64(shared, fused_backward, monkeypatch, hip_lib):
    """max|got - ref64| <= 1e-5 * max|ref64| per tensor: the bound tests/test_fused_bwd_gpu.py holds both backward routes to."""
    dev = torch.device("cuda")
    S, B = 3, 65
    layer = make_layer(128, 512).to(dev)
    layer.weight_submodule.fused_backward = fused_backward
    x = torch.randn((B, 128) if shared else (S, B, 128), generator=torch.Generator().manual_seed(8)).to(dev)
    check_layer_against_dense(layer, x, S, monkeypatch, grad_tol=1e-5)


def test_graph_capture_and_replay(hip_lib):
    from whvi_amd import _hip
    dev = torch.device("cuda")
    log2d, J, S, B = 10, 4, 2, 64                                     # the (1024, 4096) layer
    x, a, b, c = _operands(log2d, J, S, B, False, dev)
    eager = _hip.fused_shs_stacked(x, a, b, c, S, B)
    y = torch.zeros_like(eager)
    side = torch.cuda.Stream()
    side.wait_stream(torch.cuda.current_stream())
    with torch.cuda.stream(side):
        _hip.fused_shs_stacked(x, a, b, c, S, B, out=y)
    torch.cuda.current_stream().wait_stream(side)
    graph = torch.cuda.CUDAGraph()
    with torch.cuda.graph(graph):
        _hip.fused_shs_stacked(x, a, b, c, S, B, out=y)
    for _ in range(2):
        y.zero_()
        graph.replay()
        torch.cuda.synchronize()
        assert torch.equal(y.view(torch.int32), eager.view(torch.int32))
