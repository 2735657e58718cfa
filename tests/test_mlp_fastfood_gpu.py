"""The one-launch predictive pass of fastfood networks (WHVINetwork.set_fused_inference, whvi_amd/fused_fastfood.py,
whvi_mlp_fastfood_apply_f32) on the GPU: bit for bit the batched route's values for the same generator state -- the toy,
UCI and config-4 shapes, every supported (K, D, n_mid), every bias and activation pattern, packed parameters, in-kernel RNG,
non-finite inputs and signed zeros -- in one launch without the (S, B, D) activations; close to float64; the batched route
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
ACTS = {"relu": nn.ReLU, "sigmoid": nn.Sigmoid, "tanh": nn.Tanh}


def _net(n_in, D, n_mid=1, bias=True, acts=True, act="relu", seed=0, modes=None, **kw):
    """WHVILinear(n_in, D), n_mid x WHVILinear(D, D, mode="fastfood"), WHVILinear(D, 1); ``bias`` / ``acts``: one bool or one
    per layer / boundary; ``modes``: the square layers' modes (all fastfood by default).  Parameters moved off their initial
    values so that every product matters."""
    torch.manual_seed(seed)
    bias = [bias] * (n_mid + 2) if isinstance(bias, bool) else list(bias)
    acts = [acts] * (n_mid + 1) if isinstance(acts, bool) else list(acts)
    modes = modes or ["fastfood"] * n_mid
    mods = [WHVILinear(n_in, D, bias=bias[0])]
    for j in range(n_mid):
        mods += [ACTS[act]()] if acts[j] else []
        mods.append(WHVILinear(D, D, bias=bias[1 + j], mode=modes[j]))
    mods += [ACTS[act]()] if acts[n_mid] else []
    mods.append(WHVILinear(D, 1, bias=bias[-1]))
    net = WHVIRegression(mods, **kw)
    with torch.no_grad():
        for name, p in net.named_parameters():
            if name.endswith(("g_mu", "s1", "s2", "bias")):
                p.normal_(0.0, 1.0 if name.endswith(("s1", "s2")) else 0.3)
    # keep the fastfood layers' outputs O(1): each unnormalised transform grows a row by sqrt(D)
    for m in net.sequential:
        w = getattr(m, "weight_submodule", None)
        if w is not None and type(w).__name__ == "WHVIFastfoodMatrix":
            with torch.no_grad():
                w.s1.mul_(1.0 / w.D)
    return net.to(DEV).eval()


def _pass(net, x, S, fused, seed=1):
    net.set_fused_inference(fused)
    if any(getattr(m, "inkernel_rng", False) for m in net.modules()):
        net.set_inkernel_rng(True)              # a fresh generator, seeded from torch's below
    torch.manual_seed(seed)
    with torch.no_grad():
        out = net.forward_batched(x, S)
    if fused:
        assert _hip.last_kernel().startswith("whvi::mlp_fastfood_apply_kernel<"), _hip.last_kernel()
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


# ---- the reference's shapes
def test_config4_share(hip_lib):
    got = _check(_net(3, 1024), torch.randn(45730, 3, device=DEV), 16)
    assert torch.isfinite(got).all()


@pytest.mark.parametrize("B", [31, 1000])
def test_uci_shape(B, hip_lib):
    _check(_net(6, 128), torch.randn(B, 6, device=DEV), 64)


def test_toy_network_sigmoid(hip_lib):
    _check(_net(1, 128, act="sigmoid"), torch.linspace(-2, 2, 500, device=DEV).unsqueeze(1), 64)


def _supported_shapes():
    return [(kin, 1 << log2d, n_mid) for kin in (1, 4, 8) for log2d in range(6, 12) for n_mid in (1, 2, 3, 4)
            if _hip.mlp_fastfood_apply_supported(kin, n_mid, 1 << log2d)]


@pytest.mark.parametrize("kin,D,n_mid", _supported_shapes())
def test_every_supported_shape(kin, D, n_mid, hip_lib):
    n_in = {1: 1, 4: 3, 8: 6}[kin]
    _check(_net(n_in, D, n_mid), torch.randn(333, n_in, device=DEV), 5)


@pytest.mark.parametrize("bias", [(a, b, c) for a in (0, 1) for b in (0, 1) for c in (0, 1)])
@pytest.mark.parametrize("n_in", [3, 1])
def test_every_bias_combination(bias, n_in, hip_lib):
    _check(_net(n_in, 256, bias=[bool(v) for v in bias]), torch.randn(257, n_in, device=DEV), 6)
    _check(_net(n_in, 64, n_mid=2, bias=[bool(bias[0]), bool(bias[1]), not bias[1], bool(bias[2])]),
           torch.randn(100, n_in, device=DEV), 3)


@pytest.mark.parametrize("act", ["relu", "sigmoid", "tanh"])
@pytest.mark.parametrize("n_in", [6, 1])
def test_every_activation_pattern(act, n_in, hip_lib):
    for bits in range(4):                           # bits == 0: no activation module at all
        _check(_net(n_in, 128, acts=[bool(bits & 1), bool(bits & 2)], act=act), torch.randn(300, n_in, device=DEV), 8)
    for bits in (0b101, 0b010, 0b111):
        _check(_net(n_in, 256, n_mid=2, acts=[bool(bits >> i & 1) for i in range(3)], act=act),
               torch.randn(200, n_in, device=DEV), 3)


def test_packed_parameters_and_inkernel_rng(hip_lib):
    _check(_net(3, 1024).pack_parameters(), torch.randn(2000, 3, device=DEV), 16)
    _check(_net(3, 1024).set_inkernel_rng(True), torch.randn(2000, 3, device=DEV), 16)
    _check(_net(1, 128, act="sigmoid").set_inkernel_rng(True), torch.randn(100, 1, device=DEV), 64)


# ---- non-finite values and signed zeros, through every lane layout (D = 64 / 128 / 1024)
SHAPES = [(3, 1024), (6, 128), (1, 64)]


@pytest.mark.parametrize("n_in,D", SHAPES)
@pytest.mark.parametrize("act", ["relu", "sigmoid"])
def test_inf_and_nan_input_rows(n_in, D, act, hip_lib):
    x = torch.randn(300, n_in, device=DEV)
    x[3, 0] = float("inf")
    x[17, n_in - 1] = float("nan")
    x[40, 0] = -float("inf")
    _check(_net(n_in, D, act=act), x, 7, expect_nan=True)


@pytest.mark.parametrize("n_in,D", SHAPES)
def test_inf_in_a_fastfood_layer(n_in, D, hip_lib):
    net = _net(n_in, D, n_mid=2)
    mids = [m.weight_submodule for m in net.sequential if isinstance(m, WHVILinear)][1:-1]
    with torch.no_grad():
        mids[0].s1[5] = float("inf")
        mids[1].g_mu[7] = float("-inf")
    _check(net, torch.randn(200, n_in, device=DEV), 5, expect_nan=True)


@pytest.mark.parametrize("n_in,D", SHAPES)
@pytest.mark.parametrize("bias", [True, False])
def test_zero_rows_and_signed_zeros(n_in, D, bias, hip_lib):
    x = torch.randn(211, n_in, device=DEV)
    x[::5] = 0.0
    x[1::5] = -0.0
    for act in ("relu", "tanh"):
        _check(_net(n_in, D, bias=bias, act=act), x, 9)
        _check(_net(n_in, D, bias=bias, acts=False), x, 9)
        _check(_net(n_in, D, n_mid=2, bias=bias, act=act), x, 3)


# ---- float64: the operator itself, from the dense weight of every fastfood layer
@pytest.mark.parametrize("act", ["relu", None])
@pytest.mark.parametrize("kin,D,n_mid", [(1, 64, 1), (4, 128, 2), (8, 64, 3)])
def test_float64_bound(kin, D, n_mid, act, hip_lib):
    from whvi_amd.fastfood import WHVIFastfoodMatrix
    g = torch.Generator(device=DEV).manual_seed(D + n_mid)
    rnd = lambda *shape: torch.randn(*shape, device=DEV, generator=g)  # noqa: E731
    S, B = 3, 97
    x, w_in = rnd(B, kin), (rnd(S, D) if kin == 1 else rnd(S, D, kin))
    b_in, b_mid, w_out, b_out = rnd(D), rnd(n_mid, D) * 0.3, rnd(S, D), rnd(1)
    s1, s2, gg = rnd(n_mid, D) / D, rnd(n_mid, D), rnd(n_mid, S, D)
    bits = (1 << (n_mid + 1)) - 1 if act else 0
    y = _hip.mlp_fastfood_apply(x, w_in, b_in, s1, s2, gg, b_mid, w_out, b_out, mid_bias=(1 << n_mid) - 1, act_bits=bits,
                                act=act or "relu")
    layers = [WHVIFastfoodMatrix(D).to(DEV).double() for _ in range(n_mid)]

    def ref(absolute):
        """y in float64 from every layer's dense_weight; ``absolute``: the same pass on absolute values, each fastfood layer
        as |s1| |H| |g_k| |H| |s2| -- the magnitude its roundings scale with (A64)."""
        f = (lambda t: t.double().abs()) if absolute else (lambda t: t.double())   # noqa: E731
        rel = (lambda t: t) if (absolute or not act) else torch.relu              # noqa: E731
        out = []
        for s in range(S):
            h = f(x) * f(w_in[s]).view(1, D) if kin == 1 else f(x) @ f(w_in[s]).T
            h = rel(h + f(b_in))
            for m, lay in enumerate(layers):
                if absolute:          # |H| diag(|g|) |H| = sum |g| times the all-ones matrix
                    W = torch.outer(f(s1[m]), f(s2[m])) * f(gg[m, s]).sum()
                else:
                    with torch.no_grad():
                        lay.s1.copy_(s1[m])
                        lay.s2.copy_(s2[m])
                        W = lay.dense_weight(gg[m, s].double())
                h = rel(h @ W.T + f(b_mid[m]))
            out.append(h @ f(w_out[s]) + f(b_out))
        return torch.stack(out)

    y64, a64 = ref(False), ref(True)
    assert bool(((y.double() - y64).abs() <= 1e-5 * a64).all()), float(((y.double() - y64).abs() / a64).max())


# ---- one launch, no activations
def test_config4_is_one_launch_without_activations(monkeypatch, hip_lib):
    from whvi_amd import fastfood, weights

    def boom(*a, **k):
        raise AssertionError("the fused pass took the batched route")
    for name in ("small_k_apply", "fused_shs", "row_dot"):
        monkeypatch.setattr(_hip, name, boom)
    for cls in (weights.SmallKApplyFunction, weights.RowDotFunction, fastfood.FastfoodFunction):
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
    assert _hip.last_kernel() == "whvi::mlp_fastfood_apply_kernel<float, 10, 4, 1>"
    assert out.shape == (45730, 1, 16) and torch.isfinite(out).all()
    assert torch.cuda.max_memory_allocated() - base < 64 << 20
    assert net._pass_kl is None and all(getattr(m, "_mc_kl", None) is None for m in net.modules())


# ---- where the fused pass does not apply: the batched route, same values
def _both(net, x, S, seed, grad=False):
    outs = []
    for fused in (False, True):
        net.set_fused_inference(fused)
        torch.manual_seed(seed)
        with torch.set_grad_enabled(grad):
            outs.append(net.forward_batched(x, S))
        assert not _hip.last_kernel().startswith("whvi::mlp_fastfood_apply_kernel"), _hip.last_kernel()
    return outs


def test_grad_wanted_takes_the_batched_route(hip_lib):
    net = _net(6, 128)
    a, b = _both(net, torch.randn(50, 6, device=DEV), 8, 3, grad=True)
    assert b.grad_fn is not None
    _same(b.detach(), a.detach())


def test_unsupported_shapes_and_mixed_modes_take_the_batched_route(hip_lib):
    for net, n_in in ((_net(3, 4096), 3), (_net(8, 2048), 8), (_net(1, 64, n_mid=5), 1),
                      (_net(3, 256, n_mid=2, modes=["fastfood", "reference"]), 3),
                      (_net(3, 256, n_mid=2, modes=["reference", "fastfood"]), 3)):
        a, b = _both(net, torch.randn(37, n_in, device=DEV), 3, 4)
        _same(b, a)
    from whvi_amd import fused_fastfood
    assert "float32" in fused_fastfood.plan(_net(6, 128).double(), torch.randn(20, 6, device=DEV, dtype=torch.float64), 4)


def test_eval_model_under_the_flag(hip_lib):
    net = _net(6, 128, eval_samples=16)
    x, y = torch.randn(64, 6, device=DEV), torch.randn(64, 1, device=DEV)
    torch.manual_seed(6)
    want = net.eval_model(x, y)
    net.set_fused_inference(True)
    torch.manual_seed(6)
    got = net.eval_model(x, y)
    assert _hip.last_kernel().startswith("whvi::mlp_fastfood_apply_kernel<") and got == want


@pytest.mark.parametrize("n_in,D,B,S,act", [(1, 128, 100, 64, "sigmoid"), (3, 1024, 2000, 16, "relu")])
def test_graphed_predictor_captures_the_fused_pass(n_in, D, B, S, act, hip_lib):
    from whvi_amd.graphs import GraphedPredictor
    net = _net(n_in, D, act=act)
    x = torch.randn(B, n_in, device=DEV)
    outs = []
    for fused in (False, True):
        net.set_fused_inference(fused)
        torch.manual_seed(7)
        gp = GraphedPredictor(net, x, S)
        if fused:
            assert _hip.last_kernel().startswith("whvi::mlp_fastfood_apply_kernel<")
        outs.append((gp(x).clone(), gp(x).clone()))
        del gp
    for a, b in zip(outs[0], outs[1]):
        _same(b, a)
    assert not torch.equal(outs[1][0], outs[1][1])          # every replay draws afresh


# ---- sentinels: every buffer inside a sentinel-filled allocation at a random offset; nothing outside y may change
PAD = 1024
SENT = float("nan")


def _placed(t, rng):
    off = 4 * int(rng.integers(0, 64))
    buf = torch.full((PAD + off + t.numel() + PAD,), SENT, device=DEV, dtype=torch.float32)
    view = buf[PAD + off:PAD + off + t.numel()].view(t.shape)
    view.copy_(t)
    return buf, view


def _batched_launches(x, w_in, b_in, s1, s2, g, b_mid, mid_bias, w_out, b_out, bits, S):
    """The batched route's launches for the same operands: first layer, fused_shs + bias add + ReLU per layer, row_dot."""
    n_mid, D = s1.shape
    if w_in.dim() == 2:
        h = x.view(1, -1, 1) * w_in.unsqueeze(1)
        if b_in is not None:
            h = h + b_in
        if bits & 1:
            h = torch.relu(h)
    else:
        h = _hip.small_k_apply(x, w_in, b_in, relu_out=bool(bits & 1))
    B = x.shape[0]
    for m in range(n_mid):
        h = _hip.fused_shs(h.reshape(S * B, D), s1[m], g[m], s2[m], axis="col", n_samples=S, sample_stride=B).view(S, B, D)
        if (mid_bias >> m) & 1:
            h = h + b_mid[m]
        if (bits >> (m + 1)) & 1:
            h = torch.relu(h)
    y = _hip.row_dot(h.contiguous(), w_out)
    return (y + b_out if b_out is not None else y).view(S, -1)


def _sentinel_cases(n, seed):
    rng = np.random.default_rng(seed)
    out = []
    while len(out) < n:
        log2d, kin, n_mid = int(rng.integers(6, 12)), int(rng.choice([1, 4, 8])), int(rng.integers(1, 4))
        if _hip.mlp_fastfood_apply_supported(kin, n_mid, 1 << log2d):
            out.append((len(out), log2d, kin, n_mid, int(rng.integers(1, 7)), int(rng.integers(1, 700))))
    return out


@pytest.mark.parametrize("case,log2d,kin,n_mid,S,B", _sentinel_cases(16, 8))
def test_stays_inside_its_buffers(case, log2d, kin, n_mid, S, B, hip_lib):
    rng = np.random.default_rng(2000 + case)
    gen = torch.Generator(device=DEV).manual_seed(case)
    D = 1 << log2d
    rnd = lambda *shape: torch.randn(*shape, device=DEV, generator=gen)  # noqa: E731
    ops = {"x": rnd(B, kin), "w_in": rnd(S, D) if kin == 1 else rnd(S, D, kin),
           "b_in": rnd(D) if rng.integers(0, 2) else None, "s1": rnd(n_mid, D) / D, "s2": rnd(n_mid, D),
           "g": rnd(n_mid, S, D), "b_mid": rnd(n_mid, D), "w_out": rnd(S, D), "b_out": rnd(1) if rng.integers(0, 2) else None}
    mid_bias, bits = int(rng.integers(0, 1 << n_mid)), int(rng.integers(0, 1 << (n_mid + 1)))
    placed = {k: (None, None) if v is None else _placed(v, rng) for k, v in ops.items()}
    before = {k: b.clone() for k, (b, _) in placed.items() if b is not None}
    ybuf, y = _placed(torch.full((S, B), SENT, device=DEV), rng)
    ptr = lambda k: None if placed[k][1] is None else placed[k][1].data_ptr()  # noqa: E731
    rc = _hip.lib().whvi_mlp_fastfood_apply_f32(y.data_ptr(), ptr("x"), kin, ptr("w_in"), ptr("b_in"), n_mid, ptr("s1"),
                                                ptr("s2"), ptr("g"), ptr("b_mid"), mid_bias, ptr("w_out"), ptr("b_out"), S, B,
                                                log2d, 1, bits, None)
    torch.cuda.synchronize()
    assert rc == 0, _hip.last_error()
    assert _hip.last_kernel() == f"whvi::mlp_fastfood_apply_kernel<float, {log2d}, {kin}, 1>"
    off = (y.data_ptr() - ybuf.data_ptr()) // 4
    assert bool(ybuf[:off].isnan().all()) and bool(ybuf[off + S * B:].isnan().all()) and not bool(y.isnan().any())
    for k, b in before.items():
        assert torch.equal(placed[k][0].isnan(), b.isnan()) and torch.equal(placed[k][0].nan_to_num(), b.nan_to_num()), k
    want = _batched_launches(ops["x"], ops["w_in"], ops["b_in"], ops["s1"], ops["s2"], ops["g"], ops["b_mid"], mid_bias,
                             ops["w_out"], ops["b_out"], bits, S)
    _same(y, want.contiguous())
