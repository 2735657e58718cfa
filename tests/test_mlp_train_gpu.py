"""The trainable one-launch pass (WHVINetwork.set_fused_training: whvi_mlp_apply_f32 forward, whvi_mlp_apply_bwd_f32 backward)
on the GPU: the loss and the forward output bit for bit the batched route's, one forward and one backward launch and none of
the three-launch route, the reference's recorded config-4 gradients, every gradient element inside the float64 error bound the
batched route itself meets, bit-equal gradients on every run, the batched route's non-finite pattern, the fallbacks, hipGraph
training, and not one byte written outside the outputs and the workspace."""
import os
import sys

import numpy as np
import pytest
import torch
import torch.nn as nn
from torch.utils.data import DataLoader, TensorDataset

from whvi_amd import _hip, fused_mlp, weights
from whvi_amd.networks import WHVINetwork

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
from test_mlp_apply_gpu import SENT, _net, _placed, _same  # noqa: E402

pytestmark = pytest.mark.gpu
DEV = "cuda"


def _loss_grads(net, x, y, S, fused, seed=1, x_grad=False):
    """One training pass (loss + backward) with the flag ``fused``: (loss, forward output, parameter gradients, grad_x)."""
    net.train()
    net.train_samples = S
    net.set_fused_training(fused)
    if any(getattr(m, "inkernel_rng", False) for m in net.modules()):
        net.set_inkernel_rng(True)              # a fresh generator, seeded from torch's below
    net.zero_grad(set_to_none=True)
    xx = x.detach().clone().requires_grad_(x_grad)
    torch.manual_seed(seed)
    out = net(xx)
    torch.manual_seed(seed)
    loss = net.loss(xx, y, n=x.shape[0])
    xx.grad = None
    loss.backward()
    grads = {n: p.grad.clone() for n, p in net.named_parameters() if p.grad is not None}
    return loss.detach(), out.detach(), grads, (xx.grad.clone() if x_grad else None)


def _data(n_in, B, seed=2):
    g = torch.Generator(device=DEV).manual_seed(seed)
    return torch.randn(B, n_in, device=DEV, generator=g), torch.randn(B, 1, device=DEV, generator=g)


def _close(a, b, what, rtol=1e-3):
    """Parameter gradients of the two routes: same summands, different summation order (the output layer's s1 / s2 take a sum
    over D x S terms of both signs through the weight construction's chain: 6e-4 of their value seen apart at D = 256)."""
    assert a.shape == b.shape, what
    scale = float(b.abs().max())
    assert float((a - b).abs().max()) <= rtol * scale + 1e-30, (what, float((a - b).abs().max()), scale)


# ---- loss, forward output and routing
@pytest.mark.parametrize("n_in,D,S,B", [(1, 128, 1, 100), (6, 128, 1, 64), (3, 1024, 1, 256), (3, 1024, 16, 2000)])
def test_loss_and_output_are_the_batched_routes(n_in, D, S, B, hip_lib):
    net = _net(n_in, D)
    x, y = _data(n_in, B)
    l0, o0, g0, _ = _loss_grads(net, x, y, S, False)
    l1, o1, g1, _ = _loss_grads(net, x, y, S, True)
    _same(o1, o0)
    _same(l1, l0)
    assert set(g0) == set(g1) and len(g0) == len(list(net.parameters()))
    for k in g0:
        _close(g1[k], g0[k], k)


def test_one_forward_and_one_backward_launch(monkeypatch, hip_lib):
    def boom(*a, **k):
        raise AssertionError("the fused training pass took a three-launch route")
    for name in ("small_k_apply", "diag_apply", "diag_apply_bwd", "row_dot"):
        monkeypatch.setattr(_hip, name, boom)
    for cls in (weights.SmallKApplyFunction, weights.DiagApplyFunction, weights.RowDotFunction):
        monkeypatch.setattr(cls, "apply", boom)
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
    net = _net(3, 1024).train().set_fused_training(True)
    net.train_samples = 16
    x, y = _data(3, 4096)
    loss = net.loss(x, y, n=4096)
    loss.backward()
    assert seen == ["whvi::mlp_apply_kernel<float, 10, 4>", "whvi::mlp_apply_bwd_kernel<float, 10, 4, 1>"], seen
    assert torch.isfinite(loss) and all(p.grad is not None for p in net.parameters())


def test_config4_reference_fixture_with_the_flag(monkeypatch, hip_lib):
    """tests/golden/config4_golden.npz's network and recorded draws (the reference's loss, KL and every parameter gradient),
    replayed through the fused training pass: 1e-5 relative, the bar of test_config4_network_vs_reference_gpu."""
    from test_config_parity import run_config4_network
    calls = []
    bwd = _hip.mlp_apply_bwd

    def counted(*a, **k):
        calls.append(1)
        return bwd(*a, **k)
    with pytest.MonkeyPatch.context() as mp:
        mp.setattr(WHVINetwork, "fused_training", True)
        mp.setattr(_hip, "mlp_apply_bwd", counted)
        run_config4_network("cuda", monkeypatch, "batched")
    assert calls == [1]


# ---- gradients against float64
def _leaves(ops, need_x):
    return {k: (None if v is None else v.detach().clone().requires_grad_(k != "x" or need_x)) for k, v in ops.items()}


def _three_launch_grads(ops, g, mid_bias, relu, S, need_x):
    """The batched route's autograd Functions, composed as forward_batched composes them, on the same operands."""
    leaves = _leaves(ops, need_x)
    x, w_in, b_in = leaves["x"], leaves["w_in"], leaves["b_in"]
    n_mid = ops["s1"].shape[0]
    col = w_in.dim() == 2
    if col:
        h = x * w_in.unsqueeze(1)
        if b_in is not None:
            h = h + b_in
    else:
        h = weights.SmallKApplyFunction.apply(x, w_in, b_in, bool(relu & 1))
    for m in range(n_mid):
        bias = leaves["b_mid"][m] if (mid_bias >> m) & 1 else None
        h = weights.DiagApplyFunction.apply(h, leaves["s1"][m], leaves["s2"][m], leaves["u"][m], bias, S, True,
                                            m == 0 and col and bool(relu & 1), bool((relu >> (m + 1)) & 1))
    yv = weights.RowDotFunction.apply(h, leaves["w_out"], False)
    if leaves["b_out"] is not None:
        yv = yv + leaves["b_out"]
    yv = yv.view(S, -1)
    yv.backward(g)
    return yv.detach(), {k: (None if v is None else v.grad) for k, v in leaves.items()}


def _fused_grads(ops, g, mid_bias, relu, need_x):
    leaves = _leaves(ops, need_x)
    yv = fused_mlp.MLPApplyFunction.apply(leaves["x"], leaves["w_in"], leaves["b_in"], leaves["s1"], leaves["s2"], leaves["u"],
                                          leaves["b_mid"], leaves["w_out"], leaves["b_out"], mid_bias, relu)
    yv.backward(g)
    return yv.detach(), {k: (None if v is None else v.grad) for k, v in leaves.items()}


def _ref64(ops, g, mid_bias, relu, S, absolute):
    """The batched route's backward in float64 from the same float32 operands, activations and ReLU masks (the activations
    come from the route's own forward kernels); ``absolute``: every factor replaced by its absolute value."""
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
        for s in range(S):                      # one sample at a time: config 4's share is 3 GB per activation
            if col:
                a0 = x * w_in[s]
                if b_in is not None:
                    a0 = a0 + b_in
            else:
                a0 = _hip.small_k_apply(x, w_in[s:s + 1], b_in)[0]
            hs, masks = [torch.relu(a0) if relu & 1 else a0], []
            for m in range(n_mid):
                bias = b_mid[m] if (mid_bias >> m) & 1 else None
                z = _hip.diag_apply(hs[-1].unsqueeze(0), s1[m], s2[m], u[m][[0, 1 + s]], bias, n_samples=1)[0]
                masks.append(z > 0)
                hs.append(torch.relu(z) if (relu >> (m + 1)) & 1 else z)
            gs = f(g[s]).unsqueeze(1)
            d = gs * f(w_out[s])
            out["w_out"][s] = (f(hs[-1]) * gs).sum(0)
            out["b_out"] += gs.sum()
            for m in reversed(range(n_mid)):
                if (relu >> (m + 1)) & 1:
                    d = d * masks[m]
                out["w_mid"][m, s] = (d * f(hs[m])).sum(0)
                out["b_mid"][m] += d.sum(0)
                a, c, u0, uk = s1[m].double(), s2[m].double(), u[m, 0].double(), u[m, 1 + s].double()
                w = a * Dd * (u0 * c) + a * Dd * (uk * c)          # the diagonal: |s1| D (|u0 s2| + |uk s2|) in A
                d = d * ((a * Dd * (u0 * c)).abs() + (a * Dd * (uk * c)).abs() if absolute else w)
            if relu & 1:
                d = d * (a0 > 0)
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


def _operands(kin, D, n_mid, S, B, biases, seed):
    g = torch.Generator(device=DEV).manual_seed(seed)
    rnd = lambda *shape: torch.randn(*shape, device=DEV, generator=g)  # noqa: E731
    ops = {"x": rnd(B, kin), "w_in": rnd(S, D) if kin == 1 else rnd(S, D, kin), "b_in": rnd(D) * 0.3 if biases[0] else None,
           "s1": rnd(n_mid, D), "s2": rnd(n_mid, D), "u": rnd(n_mid, S + 1, D) * 0.3 / D,
           "b_mid": rnd(n_mid, D) * 0.3 if any(biases[1:-1]) else None, "w_out": rnd(S, D), "b_out": rnd(1) if biases[-1] else None}
    mid_bias = sum(1 << m for m in range(n_mid) if biases[1 + m])
    return ops, mid_bias, rnd(S, B)


def _within_bound(got, ref, A, what):
    err = (got.double() - ref).abs()
    bad = err > 1e-5 * A
    assert not bool(bad.any()), (what, int(bad.sum()), float(err.max()), float(A.max()))


def _check_bound(kin, D, n_mid, S, B, biases, relu, need_x, seed):
    ops, mid_bias, g = _operands(kin, D, n_mid, S, B, biases, seed)
    _check_bound_ops(ops, g, mid_bias, relu, S, need_x)


def _check_bound_ops(ops, g, mid_bias, relu, S, need_x):
    """Every gradient element of both routes inside |got - ref64| <= 1e-5 A64."""
    n_mid = ops["s1"].shape[0]
    yf, gf = _fused_grads(ops, g, mid_bias, relu, need_x)
    yb, gb = _three_launch_grads(ops, g, mid_bias, relu, S, need_x)
    if not need_x:
        assert gf["x"] is None and gb["x"] is None
    _same(yf, yb.contiguous())
    ref, A = _ref64(ops, g, mid_bias, relu, S, False), _ref64(ops, g, mid_bias, relu, S, True)
    for k, v in ops.items():
        if v is None or (k == "x" and not need_x):
            continue
        if k == "b_mid":                        # layers without a bias: the fused pass sums their (unused) gradient too
            rows = [m for m in range(n_mid) if (mid_bias >> m) & 1]
            for route, grads in (("fused", gf), ("batched", gb)):
                gm = grads[k] if grads[k] is not None else torch.zeros_like(v)
                _within_bound(gm[rows], ref[k][rows], A[k][rows], (route, k))
            continue
        for route, grads in (("fused", gf), ("batched", gb)):
            _within_bound(grads[k].reshape(ref[k].shape), ref[k], A[k], (route, k))


BOUND_CASES = [  # kin, log2d, n_mid, S, B, biases (first, mids..., last), relu bits, grad_x
    (1, 7, 1, 1, 100, (True, True, True), 3, True),          # toy
    (8, 7, 1, 1, 64, (True, True, True), 3, True),           # UCI
    (4, 10, 1, 1, 256, (True, True, True), 3, False),        # config 4's recipe
    (4, 7, 1, 5, 777, (False, False, False), 3, True),
    (4, 6, 2, 3, 1000, (True, False, True, False), 7, True),
    (1, 6, 2, 2, 257, (False, True, True, True), 5, True),
    (8, 8, 1, 4, 300, (True, False, False), 0, True),        # ReLUs removed
    (1, 8, 2, 1, 3, (True, True, False, True), 6, True),
    (4, 9, 1, 6, 1500, (False, True, True), 1, True),
    (1, 9, 2, 3, 513, (True, True, True, True), 7, False),
    (8, 9, 2, 2, 129, (True, True, True, True), 3, True),
    (4, 10, 2, 3, 999, (True, True, False, True), 7, True),
    (1, 10, 1, 7, 1025, (False, False, True), 2, True),
    (8, 10, 1, 2, 1, (True, True, True), 3, True),
]


@pytest.mark.parametrize("kin,log2d,n_mid,S,B,biases,relu,need_x", BOUND_CASES)
def test_gradients_inside_the_float64_bound(kin, log2d, n_mid, S, B, biases, relu, need_x, hip_lib):
    _check_bound(kin, 1 << log2d, n_mid, S, B, biases, relu, need_x, seed=7 + log2d * 13 + kin)


@pytest.mark.parametrize("packed,inkernel", [(True, False), (False, True), (True, True)])
def test_packed_parameters_and_inkernel_rng(packed, inkernel, hip_lib):
    net = _net(6, 256, n_mid=2)
    if packed:
        net.pack_parameters()
    if inkernel:
        net.set_inkernel_rng(True)
    x, y = _data(6, 300)
    l0, o0, g0, x0 = _loss_grads(net, x, y, 4, False, x_grad=True)
    seen = []
    bwd = _hip.mlp_apply_bwd

    def captured(g, *a, **k):
        seen.append((g.clone(), [None if t is None else t.clone() for t in a], dict(k)))
        return bwd(g, *a, **k)
    with pytest.MonkeyPatch.context() as mp:
        mp.setattr(_hip, "mlp_apply_bwd", captured)
        l1, o1, g1, x1 = _loss_grads(net, x, y, 4, True, x_grad=True)
    _same(o1, o0)
    _same(l1, l0)
    assert set(g0) == set(g1)
    for k in g0:
        _close(g1[k], g0[k], k)
    _close(x1, x0, "x")
    # the operands of the backward call that just ran, against float64
    (g, (xin, w_in, b_in, s1, s2, u, b_mid, w_out), kw), = seen
    ops = {"x": xin, "w_in": w_in, "b_in": b_in, "s1": s1, "s2": s2, "u": u, "b_mid": b_mid, "w_out": w_out, "b_out": None}
    _check_bound_ops(ops, g, kw["mid_bias"], kw["relu"], 4, True)


def test_config4_share_full_size(hip_lib):
    """45 730 rows x 16 samples at D = 1024: the float64 bound on both routes, and the pass's peak memory above its operands."""
    _check_bound(4, 1024, 1, 16, 45730, (True, True, True), 3, True, seed=11)
    net = _net(3, 1024)
    x, y = _data(3, 45730)
    net.train()
    net.train_samples = 16
    net.set_fused_training(True)
    for _ in range(2):                           # warm, then measure
        torch.cuda.synchronize()
        torch.cuda.reset_peak_memory_stats()
        base = torch.cuda.memory_allocated()
        loss = net.loss(x, y, n=45730)
        loss.backward()
        del loss
        torch.cuda.synchronize()
        peak = torch.cuda.max_memory_allocated() - base
    assert peak < 256 << 20, peak / 2 ** 20


def test_gradients_are_deterministic(hip_lib):
    net = _net(3, 1024)
    x, y = _data(3, 20000)
    runs = [_loss_grads(net, x, y, 8, True, x_grad=True) for _ in range(2)]
    for k in runs[0][2]:
        assert torch.equal(runs[0][2][k], runs[1][2][k]), k
    assert torch.equal(runs[0][3], runs[1][3])


@pytest.mark.parametrize("n_in,D", [(3, 128), (1, 256)])
def test_non_finite_rows_give_the_batched_pattern(n_in, D, hip_lib):
    net = _net(n_in, D)
    x, y = _data(n_in, 300)
    x[7, 0] = float("inf")
    x[100, n_in - 1] = float("nan")
    _, o0, g0, x0 = _loss_grads(net, x, y, 3, False, x_grad=True)
    _, o1, g1, x1 = _loss_grads(net, x, y, 3, True, x_grad=True)
    _same(o1, o0)
    for k in g0:
        assert torch.equal(torch.isfinite(g1[k]), torch.isfinite(g0[k])), k
    assert torch.equal(torch.isfinite(x1), torch.isfinite(x0))


# ---- where the training pass does not apply
def test_double_backward_raises(hip_lib):
    net = _net(3, 128).train().set_fused_training(True)
    x, y = _data(3, 50)
    loss = net.loss(x, y, n=50)
    with pytest.raises(RuntimeError, match="create_graph"):
        torch.autograd.grad(loss, list(net.parameters()), create_graph=True)


@pytest.mark.parametrize("args", [(3, 128, 3), (3, 2048, 1)])
def test_outside_the_range_takes_the_batched_route(args, monkeypatch, hip_lib):
    n_in, D, n_mid = args
    net = _net(n_in, D, n_mid=n_mid)
    x, y = _data(n_in, 64)
    l0, o0, g0, _ = _loss_grads(net, x, y, 2, False)

    def boom(*a, **k):
        raise AssertionError("the fused training pass ran outside its range")
    monkeypatch.setattr(_hip, "mlp_apply_bwd", boom)
    monkeypatch.setattr(_hip, "mlp_apply", boom)
    l1, o1, g1, _ = _loss_grads(net, x, y, 2, True)
    assert "whvi_mlp_apply_bwd's range" in fused_mlp.plan(net, x, 2, training=True)
    _same(o1, o0)
    _same(l1, l0)
    for k in g0:
        _same(g1[k], g0[k])


def test_inference_flag_alone_still_falls_back_when_a_graph_is_wanted(monkeypatch, hip_lib):
    net = _net(6, 128).set_fused_inference(True)

    def boom(*a, **k):
        raise AssertionError("a grad-wanting pass took a fused route without set_fused_training")
    monkeypatch.setattr(_hip, "mlp_apply_bwd", boom)
    monkeypatch.setattr(_hip, "mlp_apply", boom)
    x, y = _data(6, 50)
    net.train()
    loss = net.loss(x, y, n=50)
    loss.backward()
    assert torch.isfinite(loss)
    with torch.no_grad():
        assert "no autograd graph" in fused_mlp.plan(net, x, 2, training=True)


# ---- hipGraph training
@pytest.fixture
def warn_always():
    before = torch.is_warn_always_enabled()
    torch.set_warn_always(True)
    yield
    torch.set_warn_always(before)


class _Replay:
    """``torch.randn`` of an eager training run: the draws the graphed run copies into its static buffers, in layer order."""

    def __init__(self, draws):
        self.draws, self.i = draws, 0

    def __call__(self, *a, **k):
        t = self.draws[self.i]
        self.i += 1
        size = tuple(a[0]) if len(a) == 1 and isinstance(a[0], (tuple, list, torch.Size)) else tuple(a)
        assert tuple(t.shape) == size, (tuple(t.shape), size)
        return t.clone()


def _train(fused, graphed, tables, monkeypatch):
    from whvi_amd.evaluation import make_optimizer
    from whvi_amd.layers import WHVILinear
    from whvi_amd.networks import WHVIRegression
    torch.manual_seed(4)                         # the reference recipe's layers (test_train_trajectory_graphed_vs_reference_gpu)
    net = WHVIRegression([WHVILinear(3, 128, lambda_=3.0), nn.ReLU(), WHVILinear(128, 128, lambda_=3.0), nn.ReLU(),
                          WHVILinear(128, 1, lambda_=3.0)]).to(DEV).train()
    net.train_samples = 2
    net.set_fused_training(fused)
    init = {k: v.clone() for k, v in net.state_dict().items()}
    X, Y = _data(3, 24, seed=5)
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
    return init, torch.stack(losses), net.state_dict()


@pytest.mark.filterwarnings("error:The AccumulateGrad node's stream does not match:UserWarning")
def test_graphed_training_with_the_flag(monkeypatch, hip_lib, warn_always):
    g = torch.Generator(device=DEV).manual_seed(9)
    steps = 15                                   # 5 epochs x 3 batches
    # per layer (J, S, D): the stacked layer has J = 1 sub-matrix of D_in = 4, the square and the column layer D = 128
    tables = [torch.randn(steps, *shape, device=DEV, generator=g) for shape in ((32, 2, 4), (1, 2, 128), (1, 2, 128))]
    init, loss_g, state_g = _train(True, True, tables, monkeypatch)
    _, loss_e, state_e = _train(True, False, tables, monkeypatch)
    _, loss_b, state_b = _train(False, True, tables, monkeypatch)
    assert loss_g.shape == (steps,)
    _same(loss_g, loss_e)
    for k in state_g:
        _same(state_g[k], state_e[k])
    lr_sum = sum(0.05 * 0.05 * (1 + 0.0005 * t) ** -0.3 for t in range(steps))
    for k in state_g:
        ref, start, ours = state_b[k].double(), init[k].double(), state_g[k].double()
        moved = max(float((ref - start).abs().max()), lr_sum)
        assert float((ours - ref).abs().max()) <= 2e-2 * moved + 4e-7 * float(ref.abs().max()), k
    assert float((loss_g - loss_b).abs().max()) <= 1e-4 * float(loss_b.abs().max())


# ---- buffers
PAD = 4096


def _cases(n, seed):
    rng = np.random.default_rng(seed)
    out = []
    while len(out) < n:
        log2d, kin, n_mid = int(rng.integers(6, 11)), int(rng.choice([1, 4, 8])), int(rng.integers(1, 3))
        if _hip.mlp_apply_bwd_supported(kin, n_mid, 1 << log2d):
            out.append((len(out), log2d, kin, n_mid, int(rng.integers(1, 6)), int(rng.integers(1, 1200))))
    return out


@pytest.mark.parametrize("case,log2d,kin,n_mid,S,B", _cases(12, 8))
def test_stays_inside_its_buffers(case, log2d, kin, n_mid, S, B, hip_lib):
    rng = np.random.default_rng(2000 + case)
    D = 1 << log2d
    ops, mid_bias, g = _operands(kin, D, n_mid, S, B, [bool(rng.integers(0, 2)) for _ in range(n_mid + 2)], seed=case)
    relu = int(rng.integers(0, 1 << (n_mid + 1)))
    placed = {k: (None, None) if v is None else _placed(v, rng) for k, v in list(ops.items()) + [("g", g)]}
    before = {k: b.clone() for k, (b, _) in placed.items() if b is not None}
    need = int(_hip.lib().whvi_mlp_apply_bwd_workspace(S, B, kin, n_mid, log2d))
    outs = {"gwi": (S, D) if kin == 1 else (S, D, kin), "gwm": (n_mid, S, D), "gwo": (S, D), "gb": ((1 + n_mid) * D + 1,),
            "gx": (S, B, kin), "work": (need,)}
    bufs = {k: _placed(torch.full(shape, SENT, device=DEV), rng) for k, shape in outs.items()}
    ptr = lambda k: None if placed[k][1] is None else placed[k][1].data_ptr()  # noqa: E731
    optr = lambda k: bufs[k][1].data_ptr()  # noqa: E731
    rc = _hip.lib().whvi_mlp_apply_bwd_f32(optr("gwi"), optr("gwm"), optr("gwo"), optr("gb"), optr("gx"), optr("work"), need,
                                           ptr("g"), ptr("x"), kin, ptr("w_in"), ptr("b_in"), n_mid, ptr("s1"), ptr("s2"), ptr("u"),
                                           ptr("b_mid"), mid_bias, ptr("w_out"), S, B, log2d, relu, None)
    torch.cuda.synchronize()
    assert rc == 0, _hip.last_error()
    for k, (buf, view) in bufs.items():
        off = (view.data_ptr() - buf.data_ptr()) // 4
        assert bool((buf[:off] == SENT).all()) and bool((buf[off + view.numel():] == SENT).all()), k
        if k != "work":
            assert bool((view != SENT).all()), k
    for k, b in before.items():
        assert torch.equal(placed[k][0], b), k
    want = _hip.mlp_apply_bwd(g, ops["x"], ops["w_in"], ops["b_in"], ops["s1"], ops["s2"], ops["u"], ops["b_mid"], ops["w_out"],
                              mid_bias=mid_bias, relu=relu, need_grad_x=True)
    for k, w in zip(("gwi", "gwm", "gwo", "gb", "gx"), want):
        _same(bufs[k][1], w)
