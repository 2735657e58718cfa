"""The one-launch passes of a WHVI regression network whose square layers are fastfood layers: the predictive pass (opt-in:
``WHVINetwork.set_fused_inference()``) and the training pass, forward + backward (opt-in: ``WHVINetwork.set_fused_training()``)
-- the flags of ``whvi_amd.fused_mlp``.

A fastfood network -- ``[WHVILinear(n_in, D), act, WHVILinear(D, D, mode="fastfood"), act, ..., WHVILinear(D, 1)]`` -- has the
outer shape of ``fused_mlp``'s networks, but each square layer applies the paper's operator ``s1 * H(g_k * H(s2 * h))``
(``whvi_amd.fastfood``) instead of a diagonal.  On the batched route every layer moves the ``(S, batch, D)`` activations through
HBM: ``small_k_apply`` (or the column layer's product) writes them, ``fused_shs`` reads and writes them, a torch add per bias and
a torch pass per activation that no launch folds read and write them, ``row_dot`` reads them.  ``whvi_mlp_fastfood_apply_f32``
(whvi_amd/csrc/mlp_fastfood_apply.hip) keeps each row in registers, runs both transforms of every square layer there, and
reads ``x`` and writes ``y`` only.  Every layer's operands come from the ``_mc_operands`` the batched route's ``forward_mc``
calls, in module order, so the draws are the same; the kernel repeats the arithmetic of the launches it replaces (the fused
kernel's butterfly network, the bias as its own add), so the result is bit-identical to ``forward_batched`` without the flag.

Training: ``FastfoodMLPApplyFunction`` wraps the same launch in an autograd Function that saves only its inputs.  Its backward
is one call of ``whvi_mlp_fastfood_apply_bwd_f32`` (whvi_amd/csrc/mlp_fastfood_apply_bwd.hpp), which recomputes every row's
hidden vectors with the forward's arithmetic and applies the batched route's backward formulas (``FastfoodFunction.backward``,
and per boundary the activation backward that route runs there); the batch sums run in a fixed order (bit-identical gradients
on every run).  They differ from the batched route's gradients only by summation order; the loss is bit-identical.  The
gradient w.r.t. every sample's ``g_k`` goes back through ``_mc_operands`` to ``g_mu`` and ``g_rho`` by autograd.  There is no
double backward.

``match``, ``plan`` and ``run`` are ``fused_mlp``'s in form and meaning, on the same shared code (``whvi_amd._fused_net``); the
training plan's range is ``whvi_mlp_fastfood_apply_bwd_f32``'s.  Here are the fastfood layers' checks and their operands' layout."""
from typing import List, NamedTuple, Union

import torch
import torch.nn as nn

from whvi_amd import _fused_net, _hip
from whvi_amd._fused_net import _act_bits, _first_layer, _output_layer, _scan
from whvi_amd.fastfood import WHVIFastfoodMatrix
from whvi_amd.weights import WHVIColumnMatrix, WHVISquarePow2Matrix, WHVIStackedMatrix

__all__ = ["Plan", "FastfoodMLPApplyFunction", "match", "plan", "run"]


class Plan(NamedTuple):
    first: nn.Module                 # WHVIStackedMatrix (K = D_in = 4 / 8) or WHVIColumnMatrix (n_in = 1)
    kind: int                        # _hip.MLP_FIRST_K4 / _K8 / _COLUMN
    n_in: int
    mids: List[nn.Module]            # WHVIFastfoodMatrix, 1 .. 4 of them
    last: nn.Module                  # transposed WHVIColumnMatrix (D -> 1)
    layers: List[nn.Module]          # the WHVILinear modules in order
    D: int
    act: str                         # the activation kind at every activated boundary: "relu", "sigmoid" or "tanh"
    act_bits: int                    # bit 0: the activation behind the first layer, bit 1 + m: behind square layer m


def match(net) -> Union[Plan, str]:
    """The plan of the one-launch fastfood pass for ``net``'s module list, or why it has none."""
    scan = _scan(net)
    if isinstance(scan, str):
        return scan
    layers, act_after, act, _ = scan
    subs = [m.weight_submodule for m in layers]
    first, mids, last = subs[0], subs[1:-1], subs[-1]
    for i in (0, len(subs) - 1):
        w = subs[i]
        if not isinstance(w, (WHVIStackedMatrix, WHVIColumnMatrix)):
            return f"layer {i}: {type(w).__name__} is not a stacked or column WHVI matrix"
        if getattr(w, "hip_apply", True) is False:
            return f"layer {i}: faithful dataflow is on (hip_apply = False)"
    kinds = {type(w).__name__ for w in mids}
    if not any(isinstance(w, WHVIFastfoodMatrix) for w in mids):
        return "no fastfood square layer (mode='fastfood'): the reference-mode networks are fused_mlp's"
    for j, w in enumerate(mids):
        if isinstance(w, WHVISquarePow2Matrix):
            return f"layer {1 + j}: WHVISquarePow2Matrix among fastfood layers: the pass takes one square layer kind " \
                   f"({' and '.join(sorted(kinds))} mixed)"
        if not isinstance(w, WHVIFastfoodMatrix):
            return f"layer {1 + j}: {type(w).__name__} is not a fastfood square layer"
    head = _first_layer(first)
    if isinstance(head, str):
        return head
    D, kind, n_in = head
    for j, w in enumerate(mids):
        if w.D != D:
            return f"layer {1 + j}: width {w.D} differs from the first layer's {D}"
    reason = _output_layer(last, D)
    if reason is not None:
        return reason
    if not _hip.mlp_fastfood_apply_supported(kind, len(mids), D):
        return f"hidden width {D} with {len(mids)} fastfood layers is outside whvi_mlp_fastfood_apply's range"
    return Plan(first, kind, n_in, list(mids), last, layers, D, act or "relu", _act_bits(act_after))


_KIND = _fused_net.Kind("fused fastfood pass", "fastfood layers is outside whvi_mlp_fastfood_apply_bwd's range",
                        _hip.mlp_fastfood_apply_bwd_supported)


def plan(net, x: torch.Tensor, n_samples: int, training: bool = False) -> Union[Plan, str]:
    """``match(net)`` plus the checks of this call, ``fused_mlp.plan``'s (``_fused_net.check_call``); the training plan's range is
    ``_hip.mlp_fastfood_apply_bwd_supported``."""
    return _fused_net.check_call(_KIND, match(net), x, n_samples, training)


class FastfoodMLPApplyFunction(torch.autograd.Function):
    """``y (S, B) = mlp_fastfood_apply(x, w_in, b_in, s1, s2, g, b_mid, w_out, b_out)`` (whvi_mlp_fastfood_apply_f32) with a
    backward: one call of ``whvi_mlp_fastfood_apply_bwd_f32`` that recomputes the hidden vectors instead of reading saved ones
    (only the inputs are saved).  ``s1, s2`` (n_mid, D), ``g`` (n_mid, S, D): every sample's ``g_k``, whose gradient is returned
    as is.  First order only."""

    @staticmethod
    def forward(ctx, x, w_in, b_in, s1, s2, g, b_mid, w_out, b_out, mid_bias, act_bits, act="relu"):
        ctx.mid_bias, ctx.act_bits, ctx.act = int(mid_bias), int(act_bits), act
        ctx.save_for_backward(x, w_in, b_in, s1, s2, g, b_mid, w_out, b_out)
        return _hip.mlp_fastfood_apply(x, w_in, b_in, s1, s2, g, b_mid, w_out, b_out, mid_bias=mid_bias, act_bits=act_bits,
                                       act=act)

    @staticmethod
    def backward(ctx, gy):
        _fused_net.refuse_double_backward("FastfoodMLPApplyFunction")
        x, w_in, b_in, s1, s2, g, b_mid, w_out, b_out = ctx.saved_tensors
        gw_in, gs1, gs2, gg, gw_out, gb, gx = _hip.mlp_fastfood_apply_bwd(gy, x, w_in, b_in, s1, s2, g, b_mid, w_out,
                                                                          mid_bias=ctx.mid_bias, act_bits=ctx.act_bits,
                                                                          need_grad_x=ctx.needs_input_grad[0], act=ctx.act)
        n_mid, S, D = gg.shape
        grad_x = gx.sum(dim=0) if gx is not None else None
        grad_b_in, grad_b_mid, grad_b_out = _fused_net.bias_grads(gb, n_mid, D, b_in, b_mid, b_out)
        return grad_x, gw_in, grad_b_in, gs1, gs2, gg, grad_b_mid, gw_out, grad_b_out, None, None, None


def _apply(x, w_in, b_in, s1, s2, g, b_mid, w_out, b_out, mid_bias, act_bits, act):
    return _hip.mlp_fastfood_apply(x, w_in, b_in, s1, s2, g, b_mid, w_out, b_out, mid_bias=mid_bias, act_bits=act_bits, act=act)


def _stack(mids, drawn):
    """``s1, s2`` (n_mid, D) and ``g`` (n_mid, S, D) of the fastfood layers (copies at every depth)."""
    return torch.stack([w.s1 for w in mids]), torch.stack([w.s2 for w in mids]), torch.stack(drawn)


def run(net, p: Plan, x: torch.Tensor, n_samples: int, training: bool = False) -> torch.Tensor:
    """The pass (``_fused_net.launch``): each layer's draws in module order (``_mc_operands``, as ``forward_mc`` makes them),
    then ONE launch (``training``: through ``FastfoodMLPApplyFunction``, for a plan of ``plan(..., training=True)``).
    Returns ``(batch, 1, S)`` in forward_batched's layout; sets ``net._pass_kl`` as the batched route does -- to None, because
    fastfood layers report no in-pass KL."""
    y, _, _ = _fused_net.launch(p, x, n_samples, _stack, FastfoodMLPApplyFunction.apply if training else _apply)
    net._pass_kl = None
    return y
