"""Every refusal of the one-launch network passes (whvi_amd/fused_mlp.py, whvi_amd/fused_fastfood.py) word for word, without a
GPU: ``match`` of both modules and both forms of ``plan()`` (``training`` False / True) on host tensors, over a table of networks.
The table holds whole reason strings, compared with ``==``; ``None`` stands for "a Plan"."""
import pytest
import torch
import torch.nn as nn

NO_FASTFOOD = "no fastfood square layer (mode='fastfood'): the reference-mode networks are fused_mlp's"
SAME = object()            # fused_fastfood.match gives fused_mlp.match's reason (the shared scan of the module list, mostly)


def _fastfood_at(i):
    return f"layer {i}: WHVIFastfoodMatrix (mode='fastfood'?) is not a reference-mode WHVI matrix"


def _L(n_in, n_out, **kw):
    from whvi_amd.layers import WHVILinear
    return WHVILinear(n_in, n_out, **kw)


def _seq(*mods):
    from whvi_amd.networks import WHVIRegression
    return WHVIRegression(list(mods))


def _net(n_in, D, n_mid=1, act=nn.ReLU, modes=None, out=1):
    mods = [_L(n_in, D)]
    for mode in modes or ["reference"] * n_mid:
        mods += [act(), _L(D, D, mode=mode)]
    return _seq(*mods, act(), _L(D, out))


def _cosine():
    from whvi_amd.activations import Cosine
    return Cosine()


def _hip_apply_off(net, i):
    net.sequential[i].weight_submodule.hip_apply = False
    return net


def _faithful_square(net):
    net.sequential[2].weight_submodule.faithful_dataflow = True
    return net


FF = ["fastfood"]
# name: (the network, fused_mlp.match's answer, fused_fastfood.match's answer)
NETS = {
    "config 4": (lambda: _net(3, 1024), None, NO_FASTFOOD),
    "toy sigmoid": (lambda: _net(1, 128, act=nn.Sigmoid), None, NO_FASTFOOD),
    "fastfood": (lambda: _net(3, 128, modes=FF), _fastfood_at(1), None),
    "fastfood toy sigmoid": (lambda: _net(1, 128, act=nn.Sigmoid, modes=FF), _fastfood_at(1), None),
    "fastfood, reference": (
        lambda: _net(3, 64, modes=["fastfood", "reference"]), _fastfood_at(1),
        "layer 2: WHVISquarePow2Matrix among fastfood layers: the pass takes one square layer kind (WHVIFastfoodMatrix and "
        "WHVISquarePow2Matrix mixed)"),
    "reference, fastfood": (
        lambda: _net(3, 64, modes=["reference", "fastfood"]), _fastfood_at(2),
        "layer 1: WHVISquarePow2Matrix among fastfood layers: the pass takes one square layer kind (WHVIFastfoodMatrix and "
        "WHVISquarePow2Matrix mixed)"),
    "K = 2": (lambda: _net(2, 128), "first layer: 2 inputs pad to K = 2 (4 or 8 only)", NO_FASTFOOD),
    "K = 16": (lambda: _net(9, 128), "first layer: 9 inputs pad to K = 16 (4 or 8 only)", NO_FASTFOOD),
    "K = 2, fastfood": (lambda: _net(2, 128, modes=FF), _fastfood_at(1), "first layer: 2 inputs pad to K = 2 (4 or 8 only)"),
    "K = 16, fastfood": (lambda: _net(9, 128, modes=FF), _fastfood_at(1), "first layer: 9 inputs pad to K = 16 (4 or 8 only)"),
    "column of 96": (lambda: _net(1, 96), "first layer: hidden width 96 is not a power of two", NO_FASTFOOD),
    "column of 96, fastfood": (lambda: _seq(_L(1, 96), _L(128, 128, mode="fastfood"), _L(128, 1)), _fastfood_at(1),
                               "first layer: hidden width 96 is not a power of two"),
    "stacked of 100": (lambda: _net(3, 100),
                       "layer 1: WHVIStackedMatrix is not a square power-of-two WHVI matrix (hidden width 100?)", NO_FASTFOOD),
    "cosine": (lambda: _seq(_L(3, 128), _cosine(), _L(128, 128), _cosine(), _L(128, 1)),
               "module 1: Cosine is neither WHVILinear nor nn.ReLU / nn.Sigmoid / nn.Tanh", SAME),
    "relu then tanh": (lambda: _seq(_L(3, 64), nn.ReLU(), _L(64, 64), nn.Tanh(), _L(64, 1)),
                       "module 3: nn.Tanh after nn.ReLU: the fused passes take one activation kind per network", SAME),
    "sigmoid then relu, fastfood": (
        lambda: _seq(_L(3, 64), nn.Sigmoid(), _L(64, 64, mode="fastfood"), nn.ReLU(), _L(64, 1)),
        "module 3: nn.ReLU after nn.Sigmoid: the fused passes take one activation kind per network", SAME),
    "leading relu": (lambda: _seq(nn.ReLU(), _L(3, 64), _L(64, 64), _L(64, 1)),
                     "module 0: an nn.ReLU is only fused between two WHVI layers (one per boundary)", SAME),
    "trailing tanh": (lambda: _seq(_L(3, 64), _L(64, 64), _L(64, 1), nn.Tanh()),
                      "module 3: an nn.Tanh is only fused between two WHVI layers (one per boundary)", SAME),
    "two relus at one boundary": (lambda: _seq(_L(3, 64), nn.ReLU(), nn.ReLU(), _L(64, 64), _L(64, 1)),
                                  "module 2: an nn.ReLU is only fused between two WHVI layers (one per boundary)", SAME),
    "sigmoid and tanh at one boundary": (
        lambda: _seq(_L(3, 64), nn.Sigmoid(), nn.Tanh(), _L(64, 64), _L(64, 1)),
        "module 2: nn.Tanh after nn.Sigmoid: the fused passes take one activation kind per network", SAME),
    "two layers": (lambda: _seq(_L(3, 64), nn.ReLU(), _L(64, 1)),
                   "2 WHVI layers: the fused pass needs a first layer, 1 .. 4 square layers and an output layer", SAME),
    "five square layers": (lambda: _net(3, 64, n_mid=5), "5 square layers: at most 4", SAME),
    "five fastfood layers": (lambda: _net(3, 64, modes=FF * 5), "5 square layers: at most 4", SAME),
    "square layer of 128 in 64": (lambda: _seq(_L(3, 64), nn.ReLU(), _L(128, 128), nn.ReLU(), _L(64, 1)),
                                  "layer 1: width 128 differs from the first layer's 64", NO_FASTFOOD),
    "fastfood layer of 128 in 64": (lambda: _seq(_L(3, 64), nn.ReLU(), _L(128, 128, mode="fastfood"), nn.ReLU(), _L(64, 1)),
                                    _fastfood_at(1), "layer 1: width 128 differs from the first layer's 64"),
    "output layer of 128 in 64": (lambda: _seq(_L(3, 64), nn.ReLU(), _L(64, 64), nn.ReLU(), _L(128, 1)),
                                  "output layer: width 128 differs from the hidden width 64", NO_FASTFOOD),
    "hip_apply off, first": (lambda: _hip_apply_off(_net(3, 128), 0), "layer 0: faithful dataflow is on (hip_apply = False)", SAME),
    "hip_apply off, last": (lambda: _hip_apply_off(_net(3, 128), 4), "layer 2: faithful dataflow is on (hip_apply = False)", SAME),
    "hip_apply off, last, fastfood": (lambda: _hip_apply_off(_net(3, 128, modes=FF), 4), _fastfood_at(1),
                                      "layer 2: faithful dataflow is on (hip_apply = False)"),
    "faithful square layer": (lambda: _faithful_square(_net(3, 128)),
                              "layer 1: faithful dataflow is on (the diagonal route is switched off)", NO_FASTFOOD),
    "two outputs": (lambda: _net(3, 128, out=2), "output layer: WHVIStackedMatrix is not WHVILinear(D, 1) (one output only)",
                    NO_FASTFOOD),
    "two outputs, fastfood": (lambda: _net(3, 128, out=2, modes=FF), _fastfood_at(1),
                              "output layer: WHVIStackedMatrix is not WHVILinear(D, 1) (one output only)"),
    "D = 4096": (lambda: _net(3, 4096), "hidden width 4096 with 1 square layers is outside whvi_mlp_apply's range", NO_FASTFOOD),
    "D = 4096, fastfood": (lambda: _net(3, 4096, modes=FF), _fastfood_at(1),
                           "hidden width 4096 with 1 fastfood layers is outside whvi_mlp_fastfood_apply's range"),
    "D = 2048, K = 8": (lambda: _net(8, 2048), "hidden width 2048 with 1 square layers is outside whvi_mlp_apply's range",
                        NO_FASTFOOD),
    "D = 2048, two fastfood layers": (lambda: _net(1, 2048, modes=FF * 2), _fastfood_at(1),
                                      "hidden width 2048 with 2 fastfood layers is outside whvi_mlp_fastfood_apply's range"),
}
# plan() of the module that matches, on a host input, training or not: the first check of the call
ON_HOST = {
    "config 4": "input: needs a float32 CUDA (batch, 3) tensor",
    "toy sigmoid": "input: needs a float32 CUDA (batch, 1) tensor",
    "fastfood": "input: needs a float32 CUDA (batch, 3) tensor",
    "fastfood toy sigmoid": "input: needs a float32 CUDA (batch, 1) tensor",
}


@pytest.mark.parametrize("name", list(NETS))
def test_match_and_plan_give_the_reason_word_for_word(name):
    from whvi_amd import fused_fastfood, fused_mlp
    make, mlp_reason, ff_reason = NETS[name]
    net = make()
    x = torch.randn(5, 3)
    for module, reason in ((fused_mlp, mlp_reason), (fused_fastfood, mlp_reason if ff_reason is SAME else ff_reason)):
        got = module.match(net)
        if reason is None:
            assert isinstance(got, module.Plan), (name, module.__name__, got)
            reason = ON_HOST[name]                              # a network that matches is refused for this call's input
        else:
            assert got == reason, (name, module.__name__)       # a refused network: plan() hands match's reason on
        assert module.plan(net, x, 4, training=True) == reason, (name, module.__name__)
        with torch.no_grad():
            assert module.plan(net, x, 4) == reason, (name, module.__name__)


def test_each_network_matches_in_one_module_at_most():
    for name, (_, mlp_reason, ff_reason) in NETS.items():
        assert mlp_reason is not None or ff_reason is not None, name
        assert (name in ON_HOST) == (mlp_reason is None or ff_reason is None), name
