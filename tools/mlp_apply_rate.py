#!/usr/bin/env python3
"""tools/mlp_apply_rate.py -- the predictive pass of the reference's network shapes on the fused route (one whvi_mlp_apply
launch, WHVINetwork.set_fused_inference) against the batched three-launch route, eager and as hipGraph replays
(GraphedPredictor), in one process.

For every shape the two routes' outputs are first checked to be torch.equal for the same generator state; only then are they
timed, alternately (route A, route B, route A, ...) with HIP events around `--iters` back-to-back passes, `--repeats` times.
Prints one JSON object: per shape and route the median / min / max milliseconds per pass over the repeats.
``--fastfood``: the square layer is WHVILinear(D, D, mode="fastfood") -- the fused route is then one whvi_mlp_fastfood_apply
launch (whvi_amd/fused_fastfood.py), the batched route small_k_apply / fused_shs / torch bias add / row_dot.  ``--no-bias``:
every layer without its bias.

    python tools/mlp_apply_rate.py [--iters 20] [--repeats 7] [--shapes toy,uci,config4] [--fastfood] [--no-bias]"""
import argparse
import json
import os
import statistics
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

import torch  # noqa: E402
import torch.nn as nn  # noqa: E402

SHAPES = {                      # name: (n_in, D, batch, samples)
    "toy": (1, 128, 500, 64),           # the toy notebook's 1 -> 128 -> 128 -> 1, eval_samples = 64
    "uci": (6, 128, 1000, 64),          # src/evaluation.py's WHVILinear(n_in, 128) network on a UCI-sized test set
    "config4": (3, 1024, 45730, 16),    # BASELINE config 4
    "k8_1024": (8, 1024, 45730, 16),    # config 4's rows with 8 inputs: the K = 8, D = 1024 instantiation
}


ACTS = {"relu": nn.ReLU, "sigmoid": nn.Sigmoid, "tanh": nn.Tanh}    # --act: the activation at both boundaries


def _net(n_in, D, act="relu", fastfood=False, bias=True):
    from whvi_amd.layers import WHVILinear
    from whvi_amd.networks import WHVIRegression
    torch.manual_seed(0)
    net = WHVIRegression([WHVILinear(n_in, D, bias=bias), ACTS[act](),
                          WHVILinear(D, D, bias=bias, mode="fastfood" if fastfood else "reference"), ACTS[act](),
                          WHVILinear(D, 1, bias=bias)])
    with torch.no_grad():
        for name, p in net.named_parameters():
            if name.endswith(("g_mu", "s1", "s2", "bias")):
                p.normal_(0.0, 0.3)
        if fastfood:
            net.sequential[2].weight_submodule.s1.mul_(1.0 / D)    # the two unnormalised transforms grow a row by D
    return net.cuda().eval()


def _time(fn, iters):
    start, end = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    start.record()
    for _ in range(iters):
        fn()
    end.record()
    end.synchronize()
    return start.elapsed_time(end) / iters


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--iters", type=int, default=20)
    ap.add_argument("--repeats", type=int, default=7)
    ap.add_argument("--act", choices=sorted(ACTS), default="relu", help="the activation at both boundaries (sigmoid: the toy "
                    "notebook's own WHVI model at the toy shape)")
    ap.add_argument("--shapes", default="toy,uci,config4")
    ap.add_argument("--fastfood", action="store_true", help="a fastfood square layer (whvi_mlp_fastfood_apply)")
    ap.add_argument("--no-bias", action="store_true", help="every layer without its bias")
    args = ap.parse_args()
    from whvi_amd import _hip
    from whvi_amd.graphs import GraphedPredictor
    result = {"gpu": torch.cuda.get_device_name(0), "act": args.act, "fastfood": args.fastfood, "bias": not args.no_bias,
              "iters": args.iters, "repeats": args.repeats, "shapes": {}}
    for name in args.shapes.split(","):
        n_in, D, B, S = SHAPES[name]
        net = _net(n_in, D, args.act, args.fastfood, not args.no_bias)
        x = torch.randn(B, n_in, device="cuda")
        outs = []
        for fused in (False, True):
            net.set_fused_inference(fused)
            torch.manual_seed(1)
            with torch.no_grad():
                outs.append(net.forward_batched(x, S))
        kernel = _hip.last_kernel()
        want = ("whvi::mlp_fastfood_apply_kernel<",) if args.fastfood else ("whvi::mlp_apply_kernel<", "whvi::mlp_smooth_apply_kernel<")
        if not (kernel.startswith(want) and torch.equal(outs[0], outs[1])):
            raise SystemExit(f"{name}: the fused pass ({kernel}) does not reproduce the three-launch route")
        del outs
        routes = {}

        def eager(fused):
            def go():
                net.set_fused_inference(fused)
                with torch.no_grad():
                    net.forward_batched(x, S)
            return go
        graphs = {}
        for fused in (False, True):
            net.set_fused_inference(fused)
            graphs[fused] = GraphedPredictor(net, x, S)
        fns = {"three_launch_eager": eager(False), "fused_eager": eager(True),
               "three_launch_graph": graphs[False].graph.replay, "fused_graph": graphs[True].graph.replay}
        for fn in fns.values():
            _time(fn, 3)                                       # warm
        times = {k: [] for k in fns}
        for _ in range(args.repeats):
            for k, fn in fns.items():                          # alternately, in one process
                times[k].append(_time(fn, args.iters))
        for k, ts in times.items():
            routes[k] = {"median_ms": statistics.median(ts), "min_ms": min(ts), "max_ms": max(ts)}
        routes["kernel"] = kernel
        routes["shape"] = {"n_in": n_in, "D": D, "batch": B, "samples": S}
        result["shapes"][name] = routes
        del graphs, fns
        torch.cuda.empty_cache()
    print(json.dumps(result))


if __name__ == "__main__":
    main()
