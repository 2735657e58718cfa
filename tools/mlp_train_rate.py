#!/usr/bin/env python3
"""tools/mlp_train_rate.py -- one training pass (loss + backward) of the reference's network shapes on the fused route
(whvi_mlp_apply forward + whvi_mlp_apply_bwd backward, WHVINetwork.set_fused_training) against the batched three-launch route,
eager and as hipGraph replays, in one process.

For every shape the two routes' losses are first checked to be torch.equal for the same generator state, and their parameter
gradients to agree to 1e-3 of each tensor's largest entry (a stacked layer's sub-matrices taken as one tensor per name); only then are they timed, alternately (route A, route B, ...) with
HIP events around `--iters` back-to-back passes, `--repeats` times.  A graph replay is one captured loss + backward (gradients
accumulate into the static .grad buffers; the timing is what matters).  Also reports each route's peak allocation above the
memory held before an eager pass.  Prints one JSON object: per shape and route the median / min / max milliseconds per pass.

``--fastfood``: the square layer is WHVILinear(D, D, mode="fastfood") -- the fused route is then whvi_mlp_fastfood_apply forward +
whvi_mlp_fastfood_apply_bwd backward (whvi_amd/fused_fastfood.py), the batched route small_k_apply / the column product, fused_shs
and its backward's launches, a torch add per bias, a torch pass per unfolded activation, row_dot.

    python tools/mlp_train_rate.py [--iters 20] [--repeats 7] [--act relu] [--fastfood]
                                   [--shapes toy,uci,config4_recipe,mc128,config4_share]"""
import argparse
import json
import os
import re
import statistics
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

import torch  # noqa: E402
import torch.nn as nn  # noqa: E402

SHAPES = {                          # name: (n_in, D, batch, samples)
    "toy": (1, 128, 100, 1),            # the toy notebook's 1 -> 128 -> 128 -> 1 training step
    "uci": (6, 128, 64, 1),             # src/evaluation.py's UCI recipe, batch 64
    "config4_recipe": (3, 1024, 256, 1),    # BASELINE config 4's training recipe
    "mc128": (3, 1024, 256, 128),       # bench.py's mc128 training shape
    "config4_share": (3, 1024, 45730, 16),  # config 4's share: 45 730 rows x 16 samples
}


ACTS = {"relu": nn.ReLU, "sigmoid": nn.Sigmoid, "tanh": nn.Tanh}    # --act: the activation at both boundaries


def _net(n_in, D, act="relu", fastfood=False):
    from whvi_amd.layers import WHVILinear
    from whvi_amd.networks import WHVIRegression
    torch.manual_seed(0)
    mid = WHVILinear(D, D, bias=True, mode="fastfood" if fastfood else "reference")
    net = WHVIRegression([WHVILinear(n_in, D, bias=True), ACTS[act](), mid, ACTS[act](), WHVILinear(D, 1, bias=True)])
    with torch.no_grad():
        for name, p in net.named_parameters():
            if name.endswith(("g_mu", "s1", "s2", "bias")):
                p.normal_(0.0, 0.3)
        if fastfood:                    # keep the layer's output O(1): each unnormalised transform grows a row by sqrt(D)
            mid.weight_submodule.s1.mul_(1.0 / D)
    return net.cuda().train()


def _time(fn, iters):
    start, end = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    start.record()
    for _ in range(iters):
        fn()
    end.record()
    end.synchronize()
    return start.elapsed_time(end) / iters


def _step(net, x, y, fused):
    net.set_fused_training(fused)
    loss = net.loss(x, y, n=x.shape[0])
    loss.backward()
    return loss


def _graph(net, x, y, fused):
    side = torch.cuda.Stream()
    side.wait_stream(torch.cuda.current_stream())
    with torch.cuda.stream(side):
        for _ in range(3):
            _step(net, x, y, fused)
    torch.cuda.current_stream().wait_stream(side)
    g = torch.cuda.CUDAGraph()
    with torch.cuda.graph(g):
        _step(net, x, y, fused)
    return g


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--iters", type=int, default=20)
    ap.add_argument("--repeats", type=int, default=7)
    ap.add_argument("--act", choices=sorted(ACTS), default="relu", help="the activation at both boundaries (sigmoid: the toy "
                    "notebook's own WHVI model at the toy shape)")
    ap.add_argument("--fastfood", action="store_true", help="a fastfood square layer (whvi_mlp_fastfood_apply_bwd)")
    ap.add_argument("--shapes", default=",".join(SHAPES))
    args = ap.parse_args()
    from whvi_amd import _hip
    entry = "mlp_fastfood_apply_bwd" if args.fastfood else "mlp_apply_bwd"
    want = ("whvi::mlp_fastfood_apply_bwd_kernel<",) if args.fastfood else ("whvi::mlp_apply_bwd_kernel<", "whvi::mlp_smooth_apply_bwd_kernel<")
    result = {"gpu": torch.cuda.get_device_name(0), "act": args.act, "fastfood": args.fastfood, "iters": args.iters,
              "repeats": args.repeats, "shapes": {}}
    for name in args.shapes.split(","):
        n_in, D, B, S = SHAPES[name]
        net = _net(n_in, D, args.act, args.fastfood)
        net.train_samples = S
        x, y = torch.randn(B, n_in, device="cuda"), torch.randn(B, 1, device="cuda")
        ref, kernels = {}, []
        bwd = getattr(_hip, entry)

        def noted(*a, **k):                                    # (the backward runs on autograd's thread: ask there)
            out = bwd(*a, **k)
            kernels.append(_hip.last_kernel())
            return out
        setattr(_hip, entry, noted)
        for fused in (False, True):
            net.zero_grad(set_to_none=True)
            torch.manual_seed(1)
            loss = _step(net, x, y, fused)
            grads = {}                                         # a stacked layer's sub-matrices as ONE tensor per parameter name,
            for pname, p in net.named_parameters():            # as pack_parameters lays them out: a sub-matrix whose hidden units
                key = re.sub(r"weight_matrices\.\d+\.", "weight_matrices.*.", pname)     # are all inactive has rounding noise only
                grads.setdefault(key, []).append(p.grad.flatten())
            ref[fused] = (loss.detach(), [torch.cat(v) for v in grads.values()])
        setattr(_hip, entry, bwd)
        kernel = kernels[-1] if kernels else ""
        ok = len(kernels) == 1 and kernel.startswith(want) and torch.equal(ref[False][0], ref[True][0])
        for a, b in zip(ref[False][1], ref[True][1]):
            ok = ok and float((a - b).abs().max()) <= 1e-3 * float(b.abs().max())
        if not ok:
            raise SystemExit(f"{name}: the fused training pass ({kernels}) does not reproduce the three-launch route")
        del ref, loss
        routes = {}
        for fused in (False, True):                           # peak allocation of one eager pass above what is held
            net.zero_grad(set_to_none=True)
            _step(net, x, y, fused)
            torch.cuda.synchronize()
            torch.cuda.reset_peak_memory_stats()
            base = torch.cuda.memory_allocated()
            _step(net, x, y, fused)
            torch.cuda.synchronize()
            routes[("fused" if fused else "three_launch") + "_peak_mib"] = (torch.cuda.max_memory_allocated() - base) / 2 ** 20

        def eager(fused):
            return lambda: _step(net, x, y, fused)
        graphs = {fused: _graph(net, x, y, fused) for fused in (False, True)}
        fns = {"three_launch_eager": eager(False), "fused_eager": eager(True),
               "three_launch_graph": graphs[False].replay, "fused_graph": graphs[True].replay}
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
        net.zero_grad(set_to_none=True)
        torch.cuda.empty_cache()
    print(json.dumps(result))


if __name__ == "__main__":
    main()
