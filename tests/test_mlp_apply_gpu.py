"""The one-launch predictive pass (WHVINetwork.set_fused_inference, whvi_mlp_apply_f32) on the GPU: bit for bit the batched
route's values for the same generator state -- the reference's shapes, every bias and ReLU combination, packed parameters,
in-kernel RNG, non-finite inputs and signed zeros -- in one launch without the (S, B, D) activations; the batched route
wherever the pass is not covered; hipGraph capture; and not one byte written outside y."""
import numpy as np
import pytest
import torch
import torch.nn as nn

from whvi_amd import _hip
from whvi_amd.layers import WHVILinear
from whvi_amd.networks import WHVIRegression

pytestmark = pytest.mark.gpu
DEV = "cuda"


def _net(n_in, D, n_mid=1, bias=True, relus=True, seed=0, **kw):
    """WHVILinear(n_in, D), n_mid x WHVILinear(D, D), WHVILinear(D, 1); ``bias`` / ``relus``: one bool or one per layer /
    boundary.  Parameters moved off their initial values so that every product matters."""
    torch.manual_seed(seed)
    bias = [bias] * (n_mid + 2) if isinstance(bias, bool) else list(bias)
    relus = [relus] * (n_mid + 1) if isinstance(relus, bool) else list(relus)
    mods = [WHVILinear(n_in, D, bias=bias[0])]
    for j in range(n_mid):
        mods += [nn.ReLU()] if relus[j] else []
        mods.append(WHVILinear(D, D, bias=bias[1 + j]))
    mods += [nn.ReLU()] if relus[n_mid] else []
    mods.append(WHVILinear(D, 1, bias=bias[-1]))
    net = WHVIRegression(mods, **kw)
    with torch.no_grad():
        for name, p in net.named_parameters():
            if name.endswith(("g_mu", "s1", "s2", "bias")):
                p.normal_(0.0, 1.0 if name.endswith(("s1", "s2")) else 0.3)
    return net.to(DEV).eval()


def _pass(net, x, S, fused, seed=1):
    net.set_fused_inference(fused)
    if any(getattr(m, "inkernel_rng", False) for m in net.modules()):
        net.set_inkernel_rng(True)              # a fresh generator, seeded from torch's below
    torch.manual_seed(seed)
    with torch.no_grad():
        out = net.forward_batched(x, S)
    if fused:
        assert _hip.last_kernel().startswith("whvi::mlp_apply_kernel<"), _hip.last_kernel()
    return out


def _same(got, want):
    """Bit-identical, NaN payloads aside."""
    assert got.shape == want.shape and got.stride() == want.stride() and got.dtype == want.dtype
    ng, nw = torch.isnan(got), torch.isnan(want)
    assert torch.equal(ng, nw), f"{int((ng != nw).sum())} NaN positions differ"
    a, b = got[~ng].view(torch.int32), want[~nw].view(torch.int32)
    assert torch.equal(a, b), f"{int((a != b).sum())} of {a.numel()} values differ"


def _check(net, x, S, expect_nan=False):
    want = _pass(net, x, S, False)
    got = _pass(net, x, S, True)
    assert got.shape == (x.shape[0], 1, S)
    _same(got, want)
    if expect_nan:
        assert bool(torch.isnan(want).any())
    return got


@pytest.mark.parametrize("S", [16, 64])
def test_config4_full_size(S, hip_lib):
    net = _net(3, 1024)
    x = torch.randn(45730, 3, device=DEV)
    got = _check(net, x, S)
    assert torch.isfinite(got).all()


@pytest.mark.parametrize("B", [31, 64, 1000])
def test_uci_shape(B, hip_lib):
    _check(_net(6, 128), torch.randn(B, 6, device=DEV), 64)


def test_toy_network(hip_lib):
    _check(_net(1, 128), torch.linspace(-2, 2, 500, device=DEV).unsqueeze(1), 64)


@pytest.mark.parametrize("n_in,D,n_mid", [(8, 64, 1), (4, 64, 3), (1, 64, 2), (7, 256, 1), (3, 512, 1), (5, 512, 4),
                                          (1, 1024, 4), (8, 1024, 3), (3, 2048, 1), (1, 2048, 2), (8, 256, 2)])
def test_widths_kinds_and_depths(n_in, D, n_mid, hip_lib):
    _check(_net(n_in, D, n_mid), torch.randn(333, n_in, device=DEV), 5)


@pytest.mark.parametrize("bias", [(a, b, c) for a in (0, 1) for b in (0, 1) for c in (0, 1)])
@pytest.mark.parametrize("n_in", [3, 1])
def test_every_bias_combination(bias, n_in, hip_lib):
    _check(_net(n_in, 256, bias=[bool(v) for v in bias]), torch.randn(257, n_in, device=DEV), 6)


@pytest.mark.parametrize("relus", [(False, True), (True, False), (False, False)])
@pytest.mark.parametrize("n_in", [6, 1])
def test_relus_removed(relus, n_in, hip_lib):
    _check(_net(n_in, 128, relus=list(relus)), torch.randn(300, n_in, device=DEV), 8)
    _check(_net(n_in, 256, n_mid=2, relus=list(relus) + [relus[0]]), torch.randn(300, n_in, device=DEV), 3)


def test_packed_parameters(hip_lib):
    net = _net(3, 1024).pack_parameters()
    _check(net, torch.randn(2000, 3, device=DEV), 16)


def test_inkernel_rng(hip_lib):
    net = _net(3, 1024).set_inkernel_rng(True)
    _check(net, torch.randn(2000, 3, device=DEV), 16)
    net = _net(1, 128).set_inkernel_rng(True)
    _check(net, torch.randn(100, 1, device=DEV), 64)


# ---- non-finite values and signed zeros: the dense products' rules, through every lane layout (D = 64 / 128 / 1024)
SHAPES = [(3, 1024), (6, 128), (1, 64)]


@pytest.mark.parametrize("n_in,D", SHAPES)
def test_inf_and_nan_input_rows(n_in, D, hip_lib):
    x = torch.randn(300, n_in, device=DEV)
    x[3, 0] = float("inf")
    x[17, n_in - 1] = float("nan")
    x[40, 0] = -float("inf")
    _check(_net(n_in, D), x, 7, expect_nan=True)


@pytest.mark.parametrize("n_in,D", SHAPES)
def test_square_layer_s1_inf_and_overflowing_mean(n_in, D, hip_lib):
    net = _net(n_in, D, n_mid=2)
    mids = [m.weight_submodule for m in net.sequential if isinstance(m, WHVILinear)][1:-1]
    with torch.no_grad():
        mids[0].s1[5] = float("inf")
        mids[1].g_mu[7] = 3e38                  # D/2 * u * s2 overflows: that diagonal entry is NaN
        mids[1].s2[7] = 1.0
    _check(net, torch.randn(200, n_in, device=DEV), 5, expect_nan=True)


def test_nan_in_the_stacked_weight(hip_lib):
    net = _net(3, 1024)
    first = net.sequential[0].weight_submodule
    with torch.no_grad():
        first.weight_matrices[2].s1[1] = float("nan")
    _check(net, torch.randn(500, 3, device=DEV), 6, expect_nan=True)


@pytest.mark.parametrize("n_in,D", SHAPES)
@pytest.mark.parametrize("bias", [True, False])
def test_zero_rows_and_signed_zeros(n_in, D, bias, hip_lib):
    x = torch.randn(211, n_in, device=DEV)
    x[::5] = 0.0
    x[1::5] = -0.0
    _check(_net(n_in, D, bias=bias), x, 9)
    _check(_net(n_in, D, bias=bias, relus=False), x, 9)


# ---- one launch, no activations
def test_config4_is_one_launch_without_activations(monkeypatch, hip_lib):
    from whvi_amd import weights

    def boom(*a, **k):
        raise AssertionError("the fused pass took a three-launch route")
    for name in ("small_k_apply", "diag_apply", "row_dot"):
        monkeypatch.setattr(_hip, name, boom)
    for cls in (weights.SmallKApplyFunction, weights.DiagApplyFunction, weights.RowDotFunction):
        monkeypatch.setattr(cls, "apply", boom)
    net = _net(3, 1024).set_fused_inference(True)
    x = torch.randn(45730, 3, device=DEV)
    with torch.no_grad():
        net.forward_batched(x, 16)                 # warm (allocator, library)
        torch.cuda.synchronize()
        torch.cuda.reset_peak_memory_stats()
        base = torch.cuda.memory_allocated()
        out = net.forward_batched(x, 16)
        torch.cuda.synchronize()
    assert _hip.last_kernel().startswith("whvi::mlp_apply_kernel<float, 10, 4>")
    assert out.shape == (45730, 1, 16) and torch.isfinite(out).all()
    assert torch.cuda.max_memory_allocated() - base < 64 << 20


def test_kl_bookkeeping_matches_the_batched_route(hip_lib):
    net = _net(3, 256)
    x = torch.randn(100, 3, device=DEV)
    for fused in (False, True):
        _pass(net, x, 4, fused)
        assert net._pass_kl is None
        assert all(getattr(m, "_mc_kl", None) is None for m in net.modules())


# ---- where the fused pass does not apply: the batched route, same values
def test_grad_wanted_takes_the_batched_route(hip_lib):
    net = _net(6, 128)
    x = torch.randn(50, 6, device=DEV)
    outs = []
    for fused in (False, True):
        net.set_fused_inference(fused)
        torch.manual_seed(3)
        outs.append(net.forward_batched(x, 8))
    assert outs[1].grad_fn is not None and not _hip.last_kernel().startswith("whvi::mlp_apply_kernel")
    _same(outs[1].detach(), outs[0].detach())
    assert torch.is_tensor(net._pass_kl)


def test_unsupported_shapes_take_the_batched_route(hip_lib):
    net = _net(3, 8192)
    x = torch.randn(3, 3, device=DEV)
    with torch.no_grad():
        outs = []
        for fused in (False, True):
            net.set_fused_inference(fused)
            torch.manual_seed(4)
            outs.append(net.forward_batched(x, 2))
    _same(outs[1], outs[0])
    from whvi_amd import fused_mlp
    net = _net(6, 128).double()
    with torch.no_grad():
        for dtype in (torch.float64, torch.float32):
            assert "float32" in fused_mlp.plan(net, torch.randn(20, 6, device=DEV, dtype=dtype), 4)


def test_eval_model_under_the_flag(hip_lib):
    net = _net(6, 128, eval_samples=16)
    x, y = torch.randn(64, 6, device=DEV), torch.randn(64, 1, device=DEV)
    torch.manual_seed(6)
    want = net.eval_model(x, y)
    net.set_fused_inference(True)
    torch.manual_seed(6)
    got = net.eval_model(x, y)
    assert _hip.last_kernel().startswith("whvi::") and got == want


@pytest.mark.parametrize("n_in,D,B,S", [(1, 128, 100, 64), (3, 1024, 2000, 16)])
def test_graphed_predictor_captures_the_fused_pass(n_in, D, B, S, hip_lib):
    from whvi_amd.graphs import GraphedPredictor
    net = _net(n_in, D)
    x = torch.randn(B, n_in, device=DEV)
    outs = []
    for fused in (False, True):
        net.set_fused_inference(fused)
        torch.manual_seed(7)
        gp = GraphedPredictor(net, x, S)
        if fused:
            assert _hip.last_kernel().startswith("whvi::mlp_apply_kernel<")
        outs.append((gp(x).clone(), gp(x).clone()))
        del gp
    for a, b in zip(outs[0], outs[1]):
        _same(b, a)
    assert not torch.equal(outs[1][0], outs[1][1])          # every replay draws afresh


# ---- sentinels: every buffer inside a sentinel-filled allocation at a random offset; nothing outside y may change
PAD = 1024
SENT = -7.25e33


def _placed(t, rng):
    off = 4 * int(rng.integers(0, 64))
    buf = torch.full((PAD + off + t.numel() + PAD,), SENT, device=DEV, dtype=torch.float32)
    view = buf[PAD + off:PAD + off + t.numel()].view(t.shape)
    view.copy_(t)
    return buf, view


def _three_launches(x, w_in, b_in, s1, s2, u, b_mid, mid_bias, w_out, b_out, relu, S):
    n_mid = s1.shape[0]
    if w_in.dim() == 2:
        h = x.view(1, -1, 1) * w_in.unsqueeze(1)
        if b_in is not None:
            h = h + b_in
    else:
        h = _hip.small_k_apply(x, w_in, b_in, relu_out=bool(relu & 1))
    for m in range(n_mid):
        h = _hip.diag_apply(h, s1[m], s2[m], u[m], b_mid[m] if (mid_bias >> m) & 1 else None, n_samples=S,
                            relu_in=(m == 0 and w_in.dim() == 2 and bool(relu & 1)), relu_out=bool((relu >> (m + 1)) & 1))
    y = _hip.row_dot(h, w_out)
    return (y + b_out if b_out is not None else y).view(S, -1)


def _sentinel_cases(n, seed):
    rng = np.random.default_rng(seed)
    out = []
    while len(out) < n:
        log2d, kin, n_mid = int(rng.integers(6, 12)), int(rng.choice([1, 4, 8])), int(rng.integers(1, 4))
        if _hip.mlp_apply_supported(kin, n_mid, 1 << log2d):
            out.append((len(out), log2d, kin, n_mid, int(rng.integers(1, 7)), int(rng.integers(1, 700))))
    return out


@pytest.mark.parametrize("case,log2d,kin,n_mid,S,B", _sentinel_cases(16, 5))
def test_stays_inside_its_buffers(case, log2d, kin, n_mid, S, B, hip_lib):
    rng = np.random.default_rng(1000 + case)
    g = torch.Generator(device=DEV).manual_seed(case)
    D = 1 << log2d
    rnd = lambda *shape: torch.randn(*shape, device=DEV, generator=g)  # noqa: E731
    ops = {"x": rnd(B, kin), "w_in": rnd(S, D) if kin == 1 else rnd(S, D, kin) * (torch.rand(S, D, kin, device=DEV, generator=g) < 0.5),
           "b_in": rnd(D) if rng.integers(0, 2) else None, "s1": rnd(n_mid, D), "s2": rnd(n_mid, D), "u": rnd(n_mid, S + 1, D) * 0.3,
           "b_mid": rnd(n_mid, D), "w_out": rnd(S, D), "b_out": rnd(1) if rng.integers(0, 2) else None}
    mid_bias, relu = int(rng.integers(0, 1 << n_mid)), int(rng.integers(0, 1 << (n_mid + 1)))
    placed = {k: (None, None) if v is None else _placed(v, rng) for k, v in ops.items()}
    before = {k: b.clone() for k, (b, _) in placed.items() if b is not None}
    ybuf, y = _placed(torch.full((S, B), SENT, device=DEV), rng)
    ptr = lambda k: None if placed[k][1] is None else placed[k][1].data_ptr()  # noqa: E731
    rc = _hip.lib().whvi_mlp_apply_f32(y.data_ptr(), ptr("x"), kin, ptr("w_in"), ptr("b_in"), n_mid, ptr("s1"), ptr("s2"), ptr("u"),
                                       ptr("b_mid"), mid_bias, ptr("w_out"), ptr("b_out"), S, B, log2d, relu, None)
    torch.cuda.synchronize()
    assert rc == 0, _hip.last_error()
    off = (y.data_ptr() - ybuf.data_ptr()) // 4
    assert bool((ybuf[:off] == SENT).all()) and bool((ybuf[off + S * B:] == SENT).all()) and bool((y != SENT).all())
    for k, b in before.items():
        assert torch.equal(placed[k][0], b), k
    want = _three_launches(ops["x"], ops["w_in"], ops["b_in"], ops["s1"], ops["s2"], ops["u"], ops["b_mid"], mid_bias, ops["w_out"],
                           ops["b_out"], relu, S)
    _same(y, want.contiguous())
