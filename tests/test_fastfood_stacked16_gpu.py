"""The rectangular fastfood layer on 16-bit activations on the GPU: whvi_fused_shs_stacked_f16 / _bf16 bit for bit against the
per-block launches of whvi_fused_shs_ex_f16 / _bf16 (both storage types, every supported D, own and shared input, guards
around dst, non-finite inputs, repeatability), the Module's routing under ``keep_half``, padded and narrowed shapes and the
gradients against the per-block route, and one graph capture.

Operands as in tests/test_fused_bwd16_gpu.py: ``x`` is seeded ``randn`` rounded to the dtype; ``a, b, c`` are float32 ``randn``
with ``a`` and ``b`` scaled by 1 / sqrt(D), so that fp16 results stay finite.  The comparison is that file's ``_assert_same``:
values after ``+ 0.0``, NaN and inf positions, no tolerance.  A shared source is compared with the per-block launch on the
expanded source (that launch has no shared-source form)."""
import pytest
import torch

from test_fastfood_stacked_host import make_layer
from test_fused_bwd16_gpu import TYPE_NAME, _assert_same

pytestmark = pytest.mark.gpu

DTYPES = (torch.float16, torch.bfloat16)
SENTINEL = -776.0                                # exact in both storage types
GUARD = 2048                                     # elements on each side of dst
SHAPES = ((1, 1), (3, 5), (2, 777), (4, 64))


def _operands(dtype, log2d, J, S, B, shared, dev, seed=0):
    D = 1 << log2d
    g = torch.Generator().manual_seed(1000 * log2d + 100 * J + 10 * S + B + seed + 5000 * DTYPES.index(dtype))
    x = torch.randn(B if shared else S * B, D, generator=g).to(dtype)
    scale = 1.0 / D ** 0.5
    a = torch.randn(J, D, generator=g) * scale
    b = torch.randn(J, S, D, generator=g) * scale
    c = torch.randn(J, D, generator=g)
    return tuple(t.to(dev) for t in (x, a, b, c))


def _per_block(x, a, b, c, S, B, shared):
    """The per-block 16-bit launches, block by block (a shared source expanded first)."""
    from whvi_amd import _hip
    src = x.repeat(S, 1) if shared else x
    return [_hip.fused_shs(src, a[j], b[j], c[j], axis="col", n_samples=S, sample_stride=B) for j in range(a.size(0))]


def _stacked_into_guarded(x, a, b, c, S, B, shared):
    from whvi_amd import _hip
    n = S * B * a.size(0) * a.size(1)
    big = torch.full((GUARD + n + GUARD,), SENTINEL, dtype=x.dtype, device=x.device)
    dst = big[GUARD:GUARD + n].view(S * B, -1)
    out = _hip.fused_shs_stacked16(x, a, b, c, S, B, shared=shared, out=dst)
    assert out.data_ptr() == dst.data_ptr()
    assert bool((big[:GUARD] == SENTINEL).all()) and bool((big[GUARD + n:] == SENTINEL).all()), "a guard was written"
    return dst


def _assert_blocks(got, want, what):
    D = want[0].size(1)
    assert got.shape == (want[0].size(0), len(want) * D) and got.dtype == want[0].dtype
    for j, w in enumerate(want):
        _assert_same(got[:, j * D:(j + 1) * D], w, what + (j,))


@pytest.mark.parametrize("log2d", [6, 7, 8, 9, 10, 11])
@pytest.mark.parametrize("dtype", DTYPES, ids=("f16", "bf16"))
def test_bit_equal_to_the_per_block_launches(dtype, log2d, hip_lib):
    from whvi_amd import _hip
    dev = torch.device("cuda")
    D = 1 << log2d
    most = 65536 // (12 * D)
    name = "whvi::fused_stacked16_kernel<%s, %d, %d, false>" % (TYPE_NAME[dtype], log2d, 4 if log2d == 11 else 2)
    for J in sorted({j for j in (1, 2, 3, min(most, 5)) if j <= most}):
        assert _hip.fused_shs_stacked16_supported(dtype, D, J)
        for S, B in SHAPES:
            for shared in (False, True):
                x, a, b, c = _operands(dtype, log2d, J, S, B, shared, dev)
                got = _stacked_into_guarded(x, a, b, c, S, B, shared)
                assert _hip.last_kernel() == name
                want = _per_block(x, a, b, c, S, B, shared)
                assert all(bool(torch.isfinite(w).all()) for w in want)
                _assert_blocks(got, want, (J, S, B, shared))
                again = _stacked_into_guarded(x, a, b, c, S, B, shared)
                assert torch.equal(got.view(torch.int16), again.view(torch.int16))
    # once more with +-inf and NaN planted in two rows of x
    J, S, B = min(most, 3), 3, 5
    for shared in (False, True):
        x, a, b, c = _operands(dtype, log2d, J, S, B, shared, dev, seed=7)
        x[1, 3], x[1, D - 2], x[x.size(0) - 1, 0], x[x.size(0) - 1, D // 2] = float("inf"), float("-inf"), float("nan"), float("inf")
        got = _stacked_into_guarded(x, a, b, c, S, B, shared)
        want = _per_block(x, a, b, c, S, B, shared)
        assert any(bool(torch.isnan(w).any()) for w in want) and all(bool(torch.isfinite(w).any()) for w in want)
        _assert_blocks(got, want, (J, S, B, shared, "non-finite"))
        again = _stacked_into_guarded(x, a, b, c, S, B, shared)
        _assert_same(again, got, "non-finite, second call")


def _forward(layer, x, S, seed=21):
    from whvi_amd import _hip
    _hip.fwht_rows(torch.zeros(1, 4, device=x.device))                  # (another kernel's name in the note)
    torch.manual_seed(seed)
    with torch.no_grad():
        y = layer.forward_mc(x, S)
    return y, _hip.last_kernel()


@pytest.mark.parametrize("dtype", DTYPES, ids=("f16", "bf16"))
def test_routing(dtype, monkeypatch, hip_lib):
    """Fails without the launch: with ``keep_half`` the (128, 512) layer names fused_stacked16_kernel."""
    from whvi_amd import _hip
    dev = torch.device("cuda")
    S, B = 2, 9
    gen = torch.Generator().manual_seed(4)
    layer = make_layer(128, 512).to(dev)
    layer.weight_submodule.keep_half = True
    name = "whvi::fused_stacked16_kernel<%s, 7, 2, false>" % TYPE_NAME[dtype]
    for x in (torch.randn(B, 128, generator=gen), torch.randn(S, B, 128, generator=gen)):
        x = x.to(dtype).to(dev)
        y, seen = _forward(layer, x, S)
        assert seen == name and y.dtype == dtype and y.shape == (S, B, 512)
        with monkeypatch.context() as m:
            m.setattr(_hip, "fused_shs_stacked16_supported", lambda *a: False)
            ref, seen = _forward(layer, x, S)
        assert "fused_stacked16_kernel" not in seen and "fused_shs16_kernel<" + TYPE_NAME[dtype] in seen
        assert ref.dtype == dtype and torch.equal(y, ref)
        # without keep_half: promoted to float32 as before
        layer.weight_submodule.keep_half = False
        wide, seen = _forward(layer, x, S)
        layer.weight_submodule.keep_half = True
        assert "fused_stacked16_kernel" not in seen and wide.dtype == torch.float32
    # outside the launch's range: D_in = 8, and six blocks of 1024
    for n_in, n_out in ((8, 32), (1024, 6144)):
        layer = make_layer(n_in, n_out).to(dev)
        sub = layer.weight_submodule
        sub.keep_half = True
        assert not _hip.fused_shs_stacked16_supported(dtype, sub.D_in, sub.stack)
        y, seen = _forward(layer, torch.randn(B, n_in, generator=gen).to(dtype).to(dev), S)
        assert "fused_stacked16_kernel" not in seen and y.dtype == dtype and y.shape == (S, B, n_out)


@pytest.mark.parametrize("n_in,n_out", [(100, 256), (128, 200)])
def test_padded_and_narrowed_shapes_equal_the_per_block_route(n_in, n_out, monkeypatch, hip_lib):
    from whvi_amd import _hip
    dev = torch.device("cuda")
    S, B = 3, 7
    gen = torch.Generator().manual_seed(n_in + n_out)
    layer = make_layer(n_in, n_out, bias=True).to(dev)
    layer.weight_submodule.keep_half = True
    for dtype in DTYPES:
        for shape in ((B, n_in), (S, B, n_in)):
            x = torch.randn(*shape, generator=gen).to(dtype).to(dev)
            y, seen = _forward(layer, x, S)
            assert "fused_stacked16_kernel<" + TYPE_NAME[dtype] in seen
            with monkeypatch.context() as m:
                m.setattr(_hip, "fused_shs_stacked16_supported", lambda *a: False)
                ref, seen = _forward(layer, x, S)
            assert "fused_stacked16_kernel" not in seen
            assert y.shape == ref.shape == (S, B, n_out) and y.dtype == ref.dtype == dtype
            assert bool(torch.isfinite(ref.float()).all()) and torch.equal(y, ref)


def test_gradients_equal_the_per_block_forwards(monkeypatch, hip_lib):
    """The backward code and the saved tensors are the same on both routes, and so is the output: every gradient is equal."""
    from whvi_amd import _hip
    dev = torch.device("cuda")
    S, B, n_in, n_out = 3, 65, 128, 512
    gen = torch.Generator().manual_seed(33)
    layer = make_layer(n_in, n_out).to(dev)
    sub = layer.weight_submodule
    sub.keep_half = True
    for fused_backward in (False, True):
        sub.fused_backward = fused_backward
        for shape in ((B, n_in), (S, B, n_in)):
            x0 = torch.randn(*shape, generator=gen).half().to(dev)
            w = torch.randn(S, B, n_out, generator=gen).half().to(dev)
            results = {}
            for launch in (True, False):
                with monkeypatch.context() as m:
                    if not launch:
                        m.setattr(_hip, "fused_shs_stacked16_supported", lambda *a: False)
                    x = x0.clone().requires_grad_()
                    layer.zero_grad()
                    _hip.fwht_rows(torch.zeros(1, 4, device=dev))
                    torch.manual_seed(12)
                    y = layer.forward_mc(x, S)
                    assert ("fused_stacked16_kernel<__half, 7, 2, false>" in _hip.last_kernel()) == launch
                    y.backward(w)
                results[launch] = [y.detach(), x.grad] + [p.grad.clone() for p in sub.parameters()]
            assert results[True][0].dtype == torch.float16
            for got, want in zip(results[True], results[False]):
                assert got.dtype == want.dtype and bool(torch.isfinite(want.float()).all())
                assert torch.equal(got, want)


def test_graph_capture_and_replay(hip_lib):
    from whvi_amd import _hip
    dev = torch.device("cuda")
    log2d, J, S, B = 10, 4, 2, 64                                     # the (1024, 4096) layer
    x, a, b, c = _operands(torch.float16, log2d, J, S, B, False, dev)
    eager = _hip.fused_shs_stacked16(x, a, b, c, S, B)
    y = torch.zeros_like(eager)
    side = torch.cuda.Stream()
    side.wait_stream(torch.cuda.current_stream())
    with torch.cuda.stream(side):
        _hip.fused_shs_stacked16(x, a, b, c, S, B, out=y)
    torch.cuda.current_stream().wait_stream(side)
    graph = torch.cuda.CUDAGraph()
    with torch.cuda.graph(graph):
        _hip.fused_shs_stacked16(x, a, b, c, S, B, out=y)
    for _ in range(2):
        y.zero_()
        graph.replay()
        torch.cuda.synchronize()
        assert torch.equal(y.view(torch.int16), eager.view(torch.int16))
