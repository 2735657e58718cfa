"""Sigmoid and tanh in the one-launch passes on the GPU (whvi_mlp_apply_act_f32, whvi_mlp_apply_act_bwd_f32): every reachable
forward instantiation inside a float64 bound and against the batched route for the same draws, gradients of both routes
inside the float64 bound, one forward and one backward launch for the notebook's network, the batched route's non-finite
pattern, deterministic gradients, the fallbacks, hipGraph capture, and not one byte written outside the outputs."""
import os
import sys

import numpy as np
import pytest
import torch
import torch.nn as nn
from torch.utils.data import DataLoader, TensorDataset

from whvi_amd import _hip, fused_mlp, weights
from whvi_amd.layers import WHVILinear
from whvi_amd.networks import WHVIRegression

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
from test_mlp_apply_gpu import SENT, _placed, _same  # noqa: E402
from test_mlp_train_gpu import _Replay, _within_bound  # noqa: E402

pytestmark = pytest.mark.gpu
DEV = "cuda"
ACT = {"sigmoid": (nn.Sigmoid, torch.sigmoid, 0.25), "tanh": (nn.Tanh, torch.tanh, 1.0)}


def _snet(n_in, D, act, n_mid=1, bias=True, bits=None, seed=0, **kw):
    """WHVILinear(n_in, D), n_mid x WHVILinear(D, D), WHVILinear(D, 1) with nn.Sigmoid / nn.Tanh at the boundaries of ``bits``
    (all by default); parameters moved off their initial values so that every product matters."""
    torch.manual_seed(seed)
    cls = ACT[act][0]
    bits = (1 << (n_mid + 1)) - 1 if bits is None else bits
    mods = [WHVILinear(n_in, D, bias=bias)]
    for j in range(n_mid):
        mods += [cls()] if (bits >> j) & 1 else []
        mods.append(WHVILinear(D, D, bias=bias))
    mods += [cls()] if (bits >> n_mid) & 1 else []
    mods.append(WHVILinear(D, 1, bias=bias))
    net = WHVIRegression(mods, **kw)
    with torch.no_grad():
        for name, p in net.named_parameters():
            if name.endswith(("g_mu", "s1", "s2", "bias")):
                p.normal_(0.0, 1.0 if name.endswith(("s1", "s2")) else 0.3)
    return net.to(DEV).eval()


def _pass(net, x, S, fused, seed=1):
    net.set_fused_inference(fused)
    torch.manual_seed(seed)
    with torch.no_grad():
        out = net.forward_batched(x, S)
    if fused:
        assert _hip.last_kernel().startswith("whvi::mlp_smooth_apply_kernel<"), _hip.last_kernel()
    return out


def _ndiff(got, want):
    """Elements whose bits differ (NaN payloads aside); the NaN positions must agree."""
    ng, nw = torch.isnan(got), torch.isnan(want)
    assert torch.equal(ng, nw), f"{int((ng != nw).sum())} NaN positions differ"
    return int((got[~ng].view(torch.int32) != want[~nw].view(torch.int32)).sum())


# ---- forward: every reachable instantiation against float64, and against the batched route
def _operands(kin, D, n_mid, S, B, seed, biases=True):
    g = torch.Generator(device=DEV).manual_seed(seed)
    rnd = lambda *shape: torch.randn(*shape, device=DEV, generator=g)  # noqa: E731
    ops = {"x": rnd(B, kin), "w_in": (rnd(S, D) if kin == 1 else rnd(S, D, kin)) * 0.7, "b_in": rnd(D) * 0.3 if biases else None,
           "s1": rnd(n_mid, D), "s2": rnd(n_mid, D), "u": rnd(n_mid, S + 1, D) * 2.0 / D,
           "b_mid": rnd(n_mid, D) * 0.3 if biases else None, "w_out": rnd(S, D), "b_out": rnd(1) if biases else None}
    return ops, ((1 << n_mid) - 1 if biases else 0), rnd(S, B)


def _diag64(s1, s2, u, s, absolute=False):
    a, c, u0, uk = s1.double(), s2.double(), u[0].double(), u[1 + s].double()
    D = float(s1.shape[0])
    if absolute:
        return (a * D * (u0 * c)).abs() + (a * D * (uk * c)).abs()
    return a * D * (u0 * c) + a * D * (uk * c)


def _forward64(ops, mid_bias, act, bits):
    """y64 (S, B) in float64 from the float32 operands, and A64: the same pass on absolute values, where each activation
    passes on its largest slope times the absolute pre-activation plus the size of its output."""
    fn = {"sigmoid": torch.sigmoid, "tanh": torch.tanh}[act]
    slope = ACT[act][2]
    x, w_in, b_in, s1, s2, u, b_mid, w_out, b_out = (ops[k] for k in ("x", "w_in", "b_in", "s1", "s2", "u", "b_mid", "w_out",
                                                                        "b_out"))
    S, n_mid = w_out.shape[0], s1.shape[0]
    ys, As = [], []
    for s in range(S):
        if w_in.dim() == 2:
            z, A = x.double() * w_in[s].double(), (x.double() * w_in[s].double()).abs()
        else:
            z, A = x.double() @ w_in[s].double().t(), x.double().abs() @ w_in[s].double().abs().t()
        if b_in is not None:
            z, A = z + b_in.double(), A + b_in.double().abs()
        for m in range(n_mid + 1):
            if (bits >> m) & 1:
                h = fn(z)
                A = slope * A + h.abs()
                z = h
            if m == n_mid:
                break
            z, A = z * _diag64(s1[m], s2[m], u[m], s), A * _diag64(s1[m], s2[m], u[m], s, True)
            if (mid_bias >> m) & 1:
                z, A = z + b_mid[m].double(), A + b_mid[m].double().abs()
        y, Ay = z @ w_out[s].double(), A @ w_out[s].double().abs()
        if b_out is not None:
            y, Ay = y + b_out.double(), Ay + b_out.double().abs()
        ys.append(y)
        As.append(Ay)
    return torch.stack(ys), torch.stack(As)


def _batched(ops, mid_bias, act, bits, S):
    """The batched route's launches on the same operands: small_k_apply / x * w, torch's activation, diag_apply, row_dot."""
    fn = ACT[act][1]
    x, w_in = ops["x"], ops["w_in"]
    if w_in.dim() == 2:
        h = x.view(1, -1, 1) * w_in.unsqueeze(1)
        if ops["b_in"] is not None:
            h = h + ops["b_in"]
    else:
        h = _hip.small_k_apply(x, w_in, ops["b_in"])
    n_mid = ops["s1"].shape[0]
    for m in range(n_mid):
        if (bits >> m) & 1:
            h = fn(h)
        h = _hip.diag_apply(h, ops["s1"][m], ops["s2"][m], ops["u"][m], ops["b_mid"][m] if (mid_bias >> m) & 1 else None,
                            n_samples=S)
    if (bits >> n_mid) & 1:
        h = fn(h)
    y = _hip.row_dot(h, ops["w_out"])
    return (y + ops["b_out"] if ops["b_out"] is not None else y).view(S, -1)


FORWARD_CASES = [(log2d, kin, act) for log2d in range(6, 12) for kin in (1, 4, 8) for act in ("sigmoid", "tanh")
                 if _hip.mlp_apply_supported(kin, 1, 1 << log2d)]


@pytest.mark.parametrize("log2d,kin,act", FORWARD_CASES)
def test_every_forward_instantiation_inside_the_float64_bound(log2d, kin, act, hip_lib):
    D = 1 << log2d
    n_mid = 2 if _hip.mlp_apply_supported(kin, 2, D) else 1
    S, B = 3, 333
    for bits in ((1 << (n_mid + 1)) - 1, 0b01 if n_mid == 1 else 0b101):
        ops, mid_bias, _ = _operands(kin, D, n_mid, S, B, seed=log2d * 7 + kin + bits)
        y = _hip.mlp_apply(ops["x"], ops["w_in"], ops["b_in"], ops["s1"], ops["s2"], ops["u"], ops["b_mid"], ops["w_out"],
                           ops["b_out"], mid_bias=mid_bias, relu=bits, act=act)
        code = _hip.MLP_ACTS[act]
        assert _hip.last_kernel() == f"whvi::mlp_smooth_apply_kernel<float, {log2d}, {kin}, {code}>", _hip.last_kernel()
        y64, A64 = _forward64(ops, mid_bias, act, bits)
        _within_bound(y, y64, A64, (log2d, kin, act, bits))
        want = _batched(ops, mid_bias, act, bits, S)
        n = _ndiff(y, want.contiguous())         # none at any shape tested: ATen's float formulas, same ocml
        assert n == 0, f"{n} of {y.numel()} elements differ from the batched route"
        _same(y, want.contiguous())


@pytest.mark.parametrize("act", ["sigmoid", "tanh"])
@pytest.mark.parametrize("n_in,D,S,B", [(1, 128, 8, 100), (3, 1024, 16, 4000), (6, 128, 64, 500)])
def test_network_pass_is_the_batched_routes(act, n_in, D, S, B, hip_lib):
    net = _snet(n_in, D, act)
    x = torch.randn(B, n_in, device=DEV)
    _same(_pass(net, x, S, True), _pass(net, x, S, False))


# ---- gradients against float64
def _leaves(ops, need_x):
    return {k: (None if v is None else v.detach().clone().requires_grad_(k != "x" or need_x)) for k, v in ops.items()}


def _three_launch_grads(ops, g, mid_bias, act, bits, S, need_x):
    """The batched route's autograd Functions and torch's activation, composed as forward_batched composes them."""
    fn = ACT[act][1]
    leaves = _leaves(ops, need_x)
    x, w_in, b_in = leaves["x"], leaves["w_in"], leaves["b_in"]
    n_mid = ops["s1"].shape[0]
    if w_in.dim() == 2:
        h = x * w_in.unsqueeze(1)
        if b_in is not None:
            h = h + b_in
    else:
        h = weights.SmallKApplyFunction.apply(x, w_in, b_in, False)
    for m in range(n_mid):
        if (bits >> m) & 1:
            h = fn(h)
        bias = leaves["b_mid"][m] if (mid_bias >> m) & 1 else None
        h = weights.DiagApplyFunction.apply(h, leaves["s1"][m], leaves["s2"][m], leaves["u"][m], bias, S, True, False, False)
    if (bits >> n_mid) & 1:
        h = fn(h)
    yv = weights.RowDotFunction.apply(h, leaves["w_out"], False)
    if leaves["b_out"] is not None:
        yv = yv + leaves["b_out"]
    yv = yv.view(S, -1)
    yv.backward(g)
    return yv.detach(), {k: (None if v is None else v.grad) for k, v in leaves.items()}


def _fused_grads(ops, g, mid_bias, act, bits, need_x):
    leaves = _leaves(ops, need_x)
    yv = fused_mlp.MLPApplyFunction.apply(leaves["x"], leaves["w_in"], leaves["b_in"], leaves["s1"], leaves["s2"], leaves["u"],
                                          leaves["b_mid"], leaves["w_out"], leaves["b_out"], mid_bias, bits, act)
    yv.backward(g)
    return yv.detach(), {k: (None if v is None else v.grad) for k, v in leaves.items()}


def _ref64(ops, g, mid_bias, act, bits, S, absolute):
    """The batched route's backward in float64 from the same float32 operands and float32 activations (the route's own
    forward launches); the activation's derivative from its float32 output in float64.  ``absolute``: every factor by its
    absolute value."""
    fn = ACT[act][1]
    dact = (lambda y: y * (1.0 - y)) if act == "sigmoid" else (lambda y: 1.0 - y * y)  # noqa: E731
    f = (lambda t: t.double().abs()) if absolute else (lambda t: t.double())  # noqa: E731
    x, w_in, b_in, s1, s2, u, b_mid, w_out = (ops[k] for k in ("x", "w_in", "b_in", "s1", "s2", "u", "b_mid", "w_out"))
    n_mid, D = s1.shape
    B = x.shape[0]
    col = w_in.dim() == 2
    Dd = float(D)
    out = {"x": torch.zeros(B, x.shape[1], dtype=torch.float64, device=DEV),
           "w_in": torch.zeros(w_in.shape, dtype=torch.float64, device=DEV),
           "b_in": torch.zeros(D, dtype=torch.float64, device=DEV),
           "w_mid": torch.zeros(n_mid, S, D, dtype=torch.float64, device=DEV),
           "b_mid": torch.zeros(n_mid, D, dtype=torch.float64, device=DEV),
           "w_out": torch.zeros(S, D, dtype=torch.float64, device=DEV),
           "b_out": torch.zeros(1, dtype=torch.float64, device=DEV)}
    with torch.no_grad():
        for s in range(S):
            if col:
                a0 = x * w_in[s]
                if b_in is not None:
                    a0 = a0 + b_in
            else:
                a0 = _hip.small_k_apply(x, w_in[s:s + 1], b_in)[0]
            hs = [fn(a0) if bits & 1 else a0]              # hs[m]: the input of square layer m (activated), hs[-1]: the last
            for m in range(n_mid):
                bias = b_mid[m] if (mid_bias >> m) & 1 else None
                z = _hip.diag_apply(hs[-1].unsqueeze(0), s1[m], s2[m], u[m][[0, 1 + s]], bias, n_samples=1)[0]
                hs.append(fn(z) if (bits >> (m + 1)) & 1 else z)
            gs = f(g[s]).unsqueeze(1)
            d = gs * f(w_out[s])
            out["w_out"][s] = (f(hs[-1]) * gs).sum(0)
            out["b_out"] += gs.sum()
            for m in reversed(range(n_mid)):
                if (bits >> (m + 1)) & 1:
                    d = d * dact(hs[m + 1].double()).abs()  # y (1 - y) and 1 - y^2 are >= 0
                out["w_mid"][m, s] = (d * f(hs[m])).sum(0)
                out["b_mid"][m] += d.sum(0)
                w = _diag64(s1[m], s2[m], u[m][[0, 1 + s]], 0, absolute)
                d = d * w
            if bits & 1:
                d = d * dact(hs[0].double()).abs()
            out["b_in"] += d.sum(0)
            if col:
                out["w_in"][s] = (d * f(x)).sum(0)
                out["x"] += (d * f(w_in[s])).sum(1, keepdim=True)
            else:
                out["w_in"][s] = d.t() @ f(x)
                out["x"] += d @ f(w_in[s])
    gw = out.pop("w_mid")
    a, c = f(s1).unsqueeze(1), f(s2).unsqueeze(1)
    u0, uk = f(u[:, :1]), f(u[:, 1:])
    k_u = gw * (a * Dd * c)
    out["u"] = torch.cat((k_u.sum(1, keepdim=True), k_u), dim=1)
    out["s1"] = (gw * (Dd * (u0 * c) + Dd * (uk * c))).sum(1) if absolute else (gw * (Dd * (u0 * c + uk * c))).sum(1)
    out["s2"] = (gw * (a * Dd * (u0 + uk))).sum(1)
    return out


BOUND_CASES = [  # kin, log2d, n_mid, S, B, biases, act, bits, grad_x
    (1, 7, 1, 1, 100, True, "sigmoid", 3, True),           # the notebook's model
    (1, 7, 1, 1, 100, True, "tanh", 3, True),
    (8, 7, 1, 1, 64, True, "sigmoid", 3, True),
    (4, 10, 1, 1, 256, True, "sigmoid", 3, False),         # config 4's recipe, sigmoid
    (4, 10, 1, 4, 999, True, "tanh", 1, True),
    (4, 6, 2, 3, 1000, False, "sigmoid", 5, True),
    (1, 6, 2, 2, 257, True, "tanh", 7, True),
    (8, 8, 1, 4, 300, False, "tanh", 2, True),
    (1, 8, 2, 1, 3, True, "sigmoid", 6, True),
    (4, 9, 1, 6, 1500, True, "tanh", 3, True),
    (8, 9, 2, 2, 129, True, "sigmoid", 7, True),
    (1, 10, 2, 3, 513, True, "tanh", 7, False),
    (8, 10, 1, 2, 1, True, "sigmoid", 3, True),
]


@pytest.mark.parametrize("kin,log2d,n_mid,S,B,biases,act,bits,need_x", BOUND_CASES)
def test_gradients_inside_the_float64_bound(kin, log2d, n_mid, S, B, biases, act, bits, need_x, hip_lib):
    ops, mid_bias, g = _operands(kin, 1 << log2d, n_mid, S, B, seed=11 + log2d * 13 + kin, biases=biases)
    yf, gf = _fused_grads(ops, g, mid_bias, act, bits, need_x)
    yb, gb = _three_launch_grads(ops, g, mid_bias, act, bits, S, need_x)
    _same(yf, yb.contiguous())
    ref, A = _ref64(ops, g, mid_bias, act, bits, S, False), _ref64(ops, g, mid_bias, act, bits, S, True)
    for k, v in ops.items():
        if v is None or (k == "x" and not need_x):
            continue
        for route, grads in (("fused", gf), ("batched", gb)):
            _within_bound(grads[k].reshape(ref[k].shape), ref[k], A[k], (route, k))


# ---- the notebook's network through the flags
def _toy_data(B=100, seed=2):
    g = torch.Generator(device=DEV).manual_seed(seed)
    return torch.rand(B, 1, device=DEV, generator=g) * 3 - 1, torch.randn(B, 1, device=DEV, generator=g)


def _notebook_net(act="sigmoid"):
    torch.manual_seed(1)
    cls = ACT[act][0]
    return WHVIRegression([WHVILinear(1, 128, lambda_=1.0), cls(), WHVILinear(128, 128, lambda_=2.5), cls(),
                           WHVILinear(128, 1, lambda_=5.0)], sigma=0.1).to(DEV)


def _loss_grads(net, x, y, fused, seed=3, x_grad=False):
    net.train()
    net.set_fused_training(fused)
    net.zero_grad(set_to_none=True)
    xx = x.detach().clone().requires_grad_(x_grad)
    torch.manual_seed(seed)
    loss = net.loss(xx, y, n=x.shape[0])
    loss.backward()
    grads = {n: p.grad.clone() for n, p in net.named_parameters() if p.grad is not None}
    return loss.detach(), grads, (xx.grad.clone() if x_grad else None)


def test_one_forward_and_one_backward_launch_for_a_sigmoid_network(monkeypatch, hip_lib):
    def boom(*a, **k):
        raise AssertionError("the fused pass took the batched route")
    for name in ("small_k_apply", "diag_apply", "diag_apply_bwd", "row_dot"):
        monkeypatch.setattr(_hip, name, boom)
    for cls in (weights.SmallKApplyFunction, weights.DiagApplyFunction, weights.RowDotFunction):
        monkeypatch.setattr(cls, "apply", boom)
    monkeypatch.setattr(nn.Sigmoid, "forward", boom)
    seen = []
    fwd, bwd = _hip.mlp_apply, _hip.mlp_apply_bwd

    def fwd_seen(*a, **k):
        out = fwd(*a, **k)
        seen.append(_hip.last_kernel())
        return out

    def bwd_seen(*a, **k):
        out = bwd(*a, **k)
        seen.append(_hip.last_kernel())
        return out
    monkeypatch.setattr(_hip, "mlp_apply", fwd_seen)
    monkeypatch.setattr(_hip, "mlp_apply_bwd", bwd_seen)
    net = _notebook_net().set_fused_training(True).set_fused_inference(True)
    x, y = _toy_data()
    net.train()
    loss = net.loss(x, y, n=100)
    loss.backward()
    assert seen == ["whvi::mlp_smooth_apply_kernel<float, 7, 1, 2>", "whvi::mlp_smooth_apply_bwd_kernel<float, 7, 1, 1, 2>"], seen
    assert torch.isfinite(loss) and all(p.grad is not None for p in net.parameters())
    net.eval()
    with torch.no_grad():
        pred = net(x)
    assert seen[2:] == ["whvi::mlp_smooth_apply_kernel<float, 7, 1, 2>"] and pred.shape == (100, 1, 64)


@pytest.mark.parametrize("act", ["sigmoid", "tanh"])
@pytest.mark.parametrize("n_in,D", [(1, 128), (3, 1024)])
def test_non_finite_inputs_give_the_batched_pattern(act, n_in, D, hip_lib):
    net = _snet(n_in, D, act)
    x, y = torch.randn(300, n_in, device=DEV), torch.randn(300, 1, device=DEV)
    x[7, 0] = float("inf")
    x[40, 0] = -float("inf")
    x[100, n_in - 1] = float("nan")
    _same(_pass(net, x, 5, True), _pass(net, x, 5, False))
    net.train_samples = 3
    l0, g0, x0 = _loss_grads(net, x, y, False, x_grad=True)
    l1, g1, x1 = _loss_grads(net, x, y, True, x_grad=True)
    assert bool(torch.isfinite(l0)) == bool(torch.isfinite(l1))
    for k in g0:
        assert torch.equal(torch.isfinite(g1[k]), torch.isfinite(g0[k])), k
    assert torch.equal(torch.isfinite(x1), torch.isfinite(x0))


@pytest.mark.parametrize("act", ["sigmoid", "tanh"])
def test_gradients_are_deterministic(act, hip_lib):
    net = _snet(3, 1024, act)
    net.train_samples = 8
    x, y = torch.randn(20000, 3, device=DEV), torch.randn(20000, 1, device=DEV)
    runs = [_loss_grads(net, x, y, True, x_grad=True) for _ in range(2)]
    for k in runs[0][1]:
        assert torch.equal(runs[0][1][k], runs[1][1][k]), k
    assert torch.equal(runs[0][2], runs[1][2])


def test_double_backward_raises(hip_lib):
    net = _notebook_net().train().set_fused_training(True)
    x, y = _toy_data()
    loss = net.loss(x, y, n=100)
    with pytest.raises(RuntimeError, match="create_graph"):
        torch.autograd.grad(loss, list(net.parameters()), create_graph=True)


def test_mixed_activations_take_the_batched_route(monkeypatch, hip_lib):
    torch.manual_seed(0)
    net = WHVIRegression([WHVILinear(1, 128), nn.Sigmoid(), WHVILinear(128, 128), nn.Tanh(), WHVILinear(128, 1)]).to(DEV)
    x, y = _toy_data()
    net.eval()
    want = _pass(net, x, 4, False)
    l0, g0, _ = _loss_grads(net, x, y, False)

    def boom(*a, **k):
        raise AssertionError("a mixed network took the fused pass")
    monkeypatch.setattr(_hip, "mlp_apply", boom)
    monkeypatch.setattr(_hip, "mlp_apply_bwd", boom)
    net.eval().set_fused_inference(True)
    torch.manual_seed(1)
    with torch.no_grad():
        got = net.forward_batched(x, 4)
    _same(got, want)
    l1, g1, _ = _loss_grads(net, x, y, True)
    _same(l1, l0)
    for k in g0:
        _same(g1[k], g0[k])
    assert "Tanh" in fused_mlp.match(net) and "Sigmoid" in fused_mlp.match(net)


# ---- hipGraph
@pytest.mark.parametrize("act", ["sigmoid", "tanh"])
@pytest.mark.parametrize("n_in,D,B,S", [(1, 128, 100, 64), (3, 1024, 2000, 16)])
def test_graphed_predictor_matches_the_eager_fused_pass(act, n_in, D, B, S, hip_lib):
    from whvi_amd.graphs import GraphedPredictor
    net = _snet(n_in, D, act)
    x = torch.randn(B, n_in, device=DEV)
    outs = []
    for fused in (True, False):                  # the graphed fused pass against the graphed batched one (same draws) ...
        net.set_fused_inference(fused)
        torch.manual_seed(7)
        gp = GraphedPredictor(net, x, S)
        if fused:
            assert _hip.last_kernel().startswith("whvi::mlp_smooth_apply_kernel<")
        outs.append(gp(x).clone())
        del gp
    _same(outs[0], outs[1])
    _same(_pass(net, x, S, True), _pass(net, x, S, False))     # ... which the eager fused pass matches bit for bit


@pytest.fixture
def warn_always():
    before = torch.is_warn_always_enabled()
    torch.set_warn_always(True)
    yield
    torch.set_warn_always(before)


def _train(act, graphed, tables, monkeypatch):
    from whvi_amd.evaluation import make_optimizer
    cls = ACT[act][0]
    torch.manual_seed(4)
    net = WHVIRegression([WHVILinear(3, 128, lambda_=3.0), cls(), WHVILinear(128, 128, lambda_=3.0), cls(),
                          WHVILinear(128, 1, lambda_=3.0)]).to(DEV).train()
    net.train_samples = 2
    net.set_fused_training(True)
    g = torch.Generator(device=DEV).manual_seed(5)
    X, Y = torch.randn(24, 3, device=DEV, generator=g), torch.randn(24, 1, device=DEV, generator=g)
    loader = DataLoader(TensorDataset(X, Y), batch_size=8)
    optimizer, scheduler = make_optimizer(net, lambda0=0.05, capturable=True)
    steps = len(tables[0])
    losses = []
    if graphed:
        seen = {"i": 0}

        def before_replay(step):
            i = seen["i"]
            if i > 0:
                losses.append(step.static_loss.clone())
            for buf, table in zip(step.eps_buffers, tables):
                buf.copy_(table[i])
            seen["i"] = i + 1
        step = net.train_model(loader, optimizer, scheduler, epochs1=2, epochs2=3, graphed=True,
                               graph_options={"static_eps": True, "before_replay": before_replay})
        losses.append(step.static_loss.clone())
        assert seen["i"] == steps
    else:
        inner = net.loss

        def traced(*a, **k):
            value = inner(*a, **k)
            losses.append(value.detach().clone())
            return value
        net.loss = traced
        monkeypatch.setattr(torch, "randn", _Replay([t[i] for i in range(steps) for t in tables]))
        net.train_model(loader, optimizer, scheduler, epochs1=2, epochs2=3)
        monkeypatch.undo()
    return torch.stack(losses), net.state_dict()


@pytest.mark.parametrize("act", ["sigmoid", "tanh"])
@pytest.mark.filterwarnings("error:The AccumulateGrad node's stream does not match:UserWarning")
def test_graphed_training_matches_the_eager_fused_run(act, monkeypatch, hip_lib, warn_always):
    g = torch.Generator(device=DEV).manual_seed(9)
    steps = 15
    tables = [torch.randn(steps, *shape, device=DEV, generator=g) for shape in ((32, 2, 4), (1, 2, 128), (1, 2, 128))]
    calls = []
    bwd = _hip.mlp_apply_bwd

    def counted(*a, **k):
        calls.append(k.get("act"))
        return bwd(*a, **k)
    monkeypatch.setattr(_hip, "mlp_apply_bwd", counted)
    loss_g, state_g = _train(act, True, tables, monkeypatch)
    monkeypatch.setattr(_hip, "mlp_apply_bwd", counted)
    loss_e, state_e = _train(act, False, tables, monkeypatch)
    assert calls and set(calls) == {act}
    assert loss_g.shape == (steps,)
    _same(loss_g, loss_e)
    for k in state_g:
        _same(state_g[k], state_e[k])


# ---- buffers
def _sentinel_cases(n, seed):
    rng = np.random.default_rng(seed)
    out = []
    while len(out) < n:
        log2d, kin, n_mid = int(rng.integers(6, 11)), int(rng.choice([1, 4, 8])), int(rng.integers(1, 3))
        if _hip.mlp_apply_bwd_supported(kin, n_mid, 1 << log2d):
            out.append((len(out), log2d, kin, n_mid, int(rng.integers(1, 6)), int(rng.integers(1, 1200)),
                        ("sigmoid", "tanh")[len(out) % 2]))
    return out


@pytest.mark.parametrize("case,log2d,kin,n_mid,S,B,act", _sentinel_cases(10, 17))
def test_stays_inside_its_buffers(case, log2d, kin, n_mid, S, B, act, hip_lib):
    rng = np.random.default_rng(3000 + case)
    D = 1 << log2d
    code = _hip.MLP_ACTS[act]
    ops, mid_bias, g = _operands(kin, D, n_mid, S, B, seed=case, biases=bool(rng.integers(0, 2)))
    bits = int(rng.integers(0, 1 << (n_mid + 1)))
    placed = {k: (None, None) if v is None else _placed(v, rng) for k, v in list(ops.items()) + [("g", g)]}
    before = {k: b.clone() for k, (b, _) in placed.items() if b is not None}
    ptr = lambda k: None if placed[k][1] is None else placed[k][1].data_ptr()  # noqa: E731
    ybuf, yv = _placed(torch.full((S, B), SENT, device=DEV), rng)
    rc = _hip.lib().whvi_mlp_apply_act_f32(yv.data_ptr(), ptr("x"), kin, ptr("w_in"), ptr("b_in"), n_mid, ptr("s1"), ptr("s2"),
                                           ptr("u"), ptr("b_mid"), mid_bias, ptr("w_out"), ptr("b_out"), S, B, log2d, code, bits,
                                           None)
    torch.cuda.synchronize()
    assert rc == 0, _hip.last_error()
    off = (yv.data_ptr() - ybuf.data_ptr()) // 4
    assert bool((ybuf[:off] == SENT).all()) and bool((ybuf[off + S * B:] == SENT).all()) and bool((yv != SENT).all())
    need = int(_hip.lib().whvi_mlp_apply_bwd_workspace(S, B, kin, n_mid, log2d))
    outs = {"gwi": (S, D) if kin == 1 else (S, D, kin), "gwm": (n_mid, S, D), "gwo": (S, D), "gb": ((1 + n_mid) * D + 1,),
            "gx": (S, B, kin), "work": (need,)}
    bufs = {k: _placed(torch.full(shape, SENT, device=DEV), rng) for k, shape in outs.items()}
    optr = lambda k: bufs[k][1].data_ptr()  # noqa: E731
    rc = _hip.lib().whvi_mlp_apply_act_bwd_f32(optr("gwi"), optr("gwm"), optr("gwo"), optr("gb"), optr("gx"), optr("work"), need,
                                               ptr("g"), ptr("x"), kin, ptr("w_in"), ptr("b_in"), n_mid, ptr("s1"), ptr("s2"),
                                               ptr("u"), ptr("b_mid"), mid_bias, ptr("w_out"), S, B, log2d, code, bits, None)
    torch.cuda.synchronize()
    assert rc == 0, _hip.last_error()
    for k, (buf, view) in bufs.items():
        off = (view.data_ptr() - buf.data_ptr()) // 4
        assert bool((buf[:off] == SENT).all()) and bool((buf[off + view.numel():] == SENT).all()), k
        if k != "work":
            assert bool((view != SENT).all()), k
    for k, b in before.items():
        assert torch.equal(placed[k][0], b), k
    want_y = _hip.mlp_apply(ops["x"], ops["w_in"], ops["b_in"], ops["s1"], ops["s2"], ops["u"], ops["b_mid"], ops["w_out"],
                            ops["b_out"], mid_bias=mid_bias, relu=bits, act=act)
    _same(yv, want_y)
    want = _hip.mlp_apply_bwd(g, ops["x"], ops["w_in"], ops["b_in"], ops["s1"], ops["s2"], ops["u"], ops["b_mid"], ops["w_out"],
                              mid_bias=mid_bias, relu=bits, need_grad_x=True, act=act)
    for k, w in zip(("gwi", "gwm", "gwo", "gb", "gx"), want):
        _same(bufs[k][1], w)


# ---- the reference's own notebook model (tests/golden/toy_sigmoid_golden.npz, tests/golden/make_golden_toy_sigmoid.py)
def run_toy_sigmoid_fixture(device, monkeypatch, fused, rtol=1e-5):
    """The notebook's second WHVI model from the fixture's initial parameters and recorded draws: the first step's loss, MNLL,
    KL and every gradient, the losses and parameters of the recorded Adam steps, and the eval-mode predictions -- each at
    ``rtol`` relative to the reference (the parameters after the steps: within 5 % of Adam's step budget), the predictions from the
    reference's trained parameters.  ``fused``: both flags on (the one-launch passes must then run)."""
    from test_config_parity import _check_grads, _load_flat, _npz, _rel
    g = _npz("toy_sigmoid_golden.npz")
    net = WHVIRegression([WHVILinear(1, 128, lambda_=1.0), nn.Sigmoid(), WHVILinear(128, 128, lambda_=2.5), nn.Sigmoid(),
                          WHVILinear(128, 1, lambda_=5.0)], sigma=0.1)
    _load_flat(net, g["param_names"], g["init_params"])
    net = net.to(device).train()
    net.mc_mode = "batched"
    net.set_fused_training(fused).set_fused_inference(fused)
    eps = torch.from_numpy(g["eps"]).to(device)
    steps, samples = len(g["losses"]), g["pred"].shape[2]
    # the batched route draws (J = 1, S, 128) per layer; the reference drew sample by sample, layer by layer
    draws = [eps[3 * i + k].view(1, 1, -1) for i in range(steps) for k in range(3)]
    base = 3 * steps
    draws += [eps[base + k:base + 3 * samples:3].unsqueeze(0) for k in range(3)]
    replay = _Replay(draws)
    calls = []
    fwd, bwd = _hip.mlp_apply, _hip.mlp_apply_bwd

    def fwd_counted(*a, **k):
        calls.append(("fwd", k.get("act")))
        return fwd(*a, **k)

    def bwd_counted(*a, **k):
        calls.append(("bwd", k.get("act")))
        return bwd(*a, **k)
    monkeypatch.setattr(_hip, "mlp_apply", fwd_counted)
    monkeypatch.setattr(_hip, "mlp_apply_bwd", bwd_counted)
    monkeypatch.setattr(torch, "randn", replay)
    x, y = torch.from_numpy(g["x"]).to(device), torch.from_numpy(g["y"]).to(device)
    optimizer = torch.optim.Adam(net.parameters(), lr=1e-3)
    scheduler = torch.optim.lr_scheduler.LambdaLR(optimizer, lambda t: (1 + 0.0005 * t) ** (-0.3))
    losses = []
    for step in range(steps):
        loss = net.loss(x, y, n=len(x))
        loss.backward()
        if step == 0:
            for what, got in (("loss", loss), ("mnll", net.current_mnll), ("kl", net.current_kl)):
                want, got = float(g[what]), float(got.detach())
                assert abs(got - want) <= rtol * abs(want), (what, got, want)
            _check_grads(net, g["grads"], rtol, "toy sigmoid, first step")
        losses.append(float(loss.detach()))
        optimizer.step()
        scheduler.step()
        net.zero_grad(set_to_none=True)
    assert _rel(np.array(losses), g["losses"]) <= rtol, "losses of the recorded steps"
    # parameters after the steps, against how far Adam can move them (about lr per step, whatever a gradient's size): within
    # 5 % of max(movement, sum of the learning rates).  The losses above hold the trajectory at 1e-5; the parameters are looser
    # because Adam turns rounding differences of gradients near zero into lr-sized steps -- one entry of the square layer's
    # s1 lands 4 % of that budget away on the GPU, identically on the batched and the fused route, against 2e-7 on the host.
    # Entries the reference never moves (first-step gradient exactly zero: 127 of the square layer's 128 s1, its as-written
    # weight being exactly diagonal) may pick up rounding-level gradients there and stay within the sum of the learning rates.
    lr_sum = sum(1e-3 * (1 + 0.0005 * t) ** -0.3 for t in range(steps))
    off = 0
    for name, p in net.named_parameters():
        ours = p.detach().cpu().double().numpy().reshape(-1)
        ref, start, grad0 = (g[k][off:off + ours.size].astype(np.float64) for k in ("final_params", "init_params", "grads"))
        off += ours.size
        live = grad0 != 0.0
        if live.any():
            moved = max(np.abs(ref - start)[live].max(), lr_sum)
            err = np.abs(ours - ref)[live].max()
            assert err <= 5e-2 * moved + 4e-7 * np.abs(ref).max(), (name, err, moved)
        if (~live).any():
            assert np.abs(ours - ref)[~live].max() <= 1.5 * lr_sum, (name, "entries at rest in the reference")
    # the predictive pass from the reference's own trained parameters
    _load_flat(net, g["param_names"], g["final_params"])
    net.eval_samples = samples
    net.eval()
    with torch.no_grad():
        pred = net(torch.from_numpy(g["x_test"]).to(device))
    monkeypatch.undo()
    assert replay.i == len(draws)
    assert pred.shape == tuple(g["pred"].shape)
    assert _rel(pred.cpu().numpy(), g["pred"]) <= rtol, "eval-mode predictions"
    return calls


def test_toy_sigmoid_reference_fixture_through_the_fused_passes(monkeypatch, hip_lib):
    calls = run_toy_sigmoid_fixture("cuda", monkeypatch, True)
    steps = len(np.load(os.path.join(os.path.dirname(__file__), "golden", "toy_sigmoid_golden.npz"))["losses"])
    assert calls == [("fwd", "sigmoid"), ("bwd", "sigmoid")] * steps + [("fwd", "sigmoid")], calls


def test_toy_sigmoid_reference_fixture_through_the_batched_route(monkeypatch, hip_lib):
    assert run_toy_sigmoid_fixture("cuda", monkeypatch, False) == []
