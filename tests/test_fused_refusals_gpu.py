"""The refusals of the one-launch network passes that need a device, word for word, at the smallest covered shape (D = 64,
S = 2, B = 3, one square layer, a column and a K = 4 first layer): the four ``_hip`` wrappers refuse mis-shaped and float64
operands in Python, before any launch, and the next supported call returns the bits it returned before; the two ``plan()``
functions name the reasons that lie behind their device check.  Every launch made here is a valid one."""
import pytest
import torch
import torch.nn as nn

from whvi_amd import _hip, fused_fastfood, fused_mlp
from whvi_amd.layers import WHVILinear
from whvi_amd.networks import WHVIRegression

pytestmark = pytest.mark.gpu
DEV = "cuda"
D, S, B = 64, 2, 3

# wrapper: (the per-layer tensor's rows beyond S, backward?, the keyword of its boundary bits)
WRAPPERS = {"mlp_apply": (1, False, "relu"), "mlp_fastfood_apply": (0, False, "act_bits"),
            "mlp_apply_bwd": (1, True, "relu"), "mlp_fastfood_apply_bwd": (0, True, "act_bits")}


def _operands(name, first):
    extra, bwd, _ = WRAPPERS[name]
    g = torch.Generator(device=DEV).manual_seed(7)
    rnd = lambda *shape: torch.randn(*shape, device=DEV, generator=g)  # noqa: E731
    ops = {"x": rnd(B, first), "w_in": rnd(S, D) if first == 1 else rnd(S, D, first), "b_in": rnd(D) * 0.3, "s1": rnd(1, D),
           "s2": rnd(1, D), "mid": rnd(1, S + extra, D) * 0.3 / D, "b_mid": rnd(1, D) * 0.3, "w_out": rnd(S, D)}
    if bwd:
        return dict(g=rnd(S, B), **ops)
    return dict(ops, b_out=rnd(1))


def _call(name, ops):
    out = getattr(_hip, name)(*ops.values(), mid_bias=1, act="relu", **{WRAPPERS[name][2]: 3})
    return out if isinstance(out, tuple) else (out,)


@pytest.mark.parametrize("first", (1, 4))
@pytest.mark.parametrize("name", list(WRAPPERS))
def test_wrapper_refuses_in_python_and_the_next_call_is_unchanged(name, first, hip_lib):
    ops = _operands(name, first)
    before = [None if t is None else t.clone() for t in _call(name, ops)]
    mid = ops["mid"]
    shapes, dtype = f"{name}: operand shapes do not match", f"{name}: float32 CUDA tensors on one device only"
    refused = [({"mid": mid[:, :-1]}, shapes), ({"mid": torch.cat((mid, mid[:, :1]), dim=1)}, shapes),
               ({"x": torch.zeros((B, first + 1), device=DEV)}, shapes), ({"b_mid": torch.zeros((1, D + 1), device=DEV)}, shapes),
               ({"s1": ops["s1"].double()}, dtype), ({"x": ops["x"].double()}, dtype), ({"b_in": ops["b_in"].double()}, dtype)]
    for change, message in refused:
        with pytest.raises(RuntimeError) as err:
            _call(name, dict(ops, **change))
        assert str(err.value) == message, (name, list(change))
    after = _call(name, ops)
    assert len(after) == len(before)
    for a, b in zip(after, before):
        assert (a is None and b is None) or torch.equal(a, b), name


def _net(n_in, width, mode):
    return WHVIRegression([WHVILinear(n_in, width), nn.ReLU(), WHVILinear(width, width, mode=mode), nn.ReLU(),
                           WHVILinear(width, 1)]).to(DEV)


KINDS = {"reference": (fused_mlp, "fused pass", "square layers is outside whvi_mlp_apply_bwd's range"),
         "fastfood": (fused_fastfood, "fused fastfood pass", "fastfood layers is outside whvi_mlp_fastfood_apply_bwd's range")}


@pytest.mark.parametrize("n_in", (1, 3))
@pytest.mark.parametrize("mode", list(KINDS))
def test_plan_names_the_reasons_behind_the_device_check(mode, n_in, hip_lib):
    module, pass_name, bwd_range = KINDS[mode]
    net, x = _net(n_in, D, mode), torch.randn(B, n_in, device=DEV)
    assert any(p.requires_grad for p in net.parameters()) and torch.is_grad_enabled()
    assert module.plan(net, x, S) == f"an autograd graph is wanted (the {pass_name} has no backward)"
    assert isinstance(module.plan(net, x, S, training=True), module.Plan)
    with torch.no_grad():
        assert module.plan(net, x, S, training=True) == \
            "no autograd graph is wanted (the training pass is for passes that need one)"
        assert isinstance(module.plan(net, x, S), module.Plan)
        assert module.plan(net, x, 0) == f"0 samples x {B} rows: outside 1 .. 2^32 - 1 rows"
    assert module.plan(net.double(), x, S, training=True) == "parameters: float32 on the input's device only"
    if n_in == 1:                                     # inside the forward's range, outside the backward's
        wide = _net(1, 2048, mode)
        assert module.plan(wide, x, S, training=True) == f"hidden width 2048 with 1 {bwd_range}"
