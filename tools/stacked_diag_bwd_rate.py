#!/usr/bin/env python3
"""tools/stacked_diag_bwd_rate.py -- what the one-launch backward of the stacked diagonal route
(``WHVIStackedMatrix.diag_blocks_backward``, whvi_diag_apply_stacked_bwd_f32) buys over the torch-op backward it replaces.
The protocol of tools/stacked_diag_rate.py: one process, operands resident, HIP events on the launch stream, a warm-up per
route (clocks ramp), then the routes ALTERNATE over the repeats; median and min-max per route.  Both routes run the same
forward launch (``diag_blocks`` on), so a measurement is forward + backward of one pass and the difference is the backward's.
Values (the output and every gradient) are compared before anything is timed.  Beside every number: ``copy_probe``,
whvi_stream_copy_probe moving the bytes the backward launch moves (``g``, the columns of ``x`` under a written column, the
whole ``grad_x`` where the input wants one) with no arithmetic, and the allocator's peak during ``backward()`` both ways.

    python tools/stacked_diag_bwd_rate.py --out profiles/r23/stacked_diag_bwd_rate.json

Shapes: tools/stacked_diag_rate.py's seven -- five layers (``forward_mc`` + ``backward`` of ``(out * cot).sum() + KL``; a
per-sample input wants its gradient, a shared one is data) and the energy / naval networks (``loss(x, y).backward()``)."""
import argparse
import json
import os
import statistics
import sys

import torch
import torch.nn as nn

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
from whvi_amd import _hip  # noqa: E402
from whvi_amd.layers import WHVILinear  # noqa: E402
from whvi_amd.networks import WHVIRegression  # noqa: E402
from stacked_diag_rate import LAYER_SHAPES, NET_SHAPES, probe  # noqa: E402


def measure(routes, repeats, warmup):
    def timed(name):
        e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        e0.record()
        routes[name]()
        e1.record()
        e1.synchronize()
        return e0.elapsed_time(e1)

    for name in routes:
        for _ in range(warmup):
            timed(name)
    times = {name: [] for name in routes}
    for _ in range(repeats):
        for name in routes:                                         # alternating: one measurement of each route per repeat
            times[name].append(timed(name))
    return {name: {"ms_median": statistics.median(ts), "ms_min": min(ts), "ms_max": max(ts), "ms": ts} for name, ts in times.items()}


def report(out):
    r = out["routes"]
    out["speedup"] = r["flag_off"]["ms_median"] / r["flag_on"]["ms_median"]
    out["flag_on_max_below_flag_off_min"] = r["flag_on"]["ms_max"] < r["flag_off"]["ms_min"]
    print(f"{out['name']:28s} " + "; ".join(f"{n} {v['ms_median']:.3f} ms [{v['ms_min']:.3f}-{v['ms_max']:.3f}]" for n, v in r.items()) +
          f"; speedup {out['speedup']:.2f}; backward peak on {out['backward_peak_MiB']['flag_on']:.1f} MiB, off "
          f"{out['backward_peak_MiB']['flag_off']:.1f} MiB; max gradient difference / max|ref| {out['max_relative_difference']:.1e}",
          flush=True)
    return out


def backward_peak(make_loss):
    loss = make_loss()
    torch.cuda.synchronize()
    torch.cuda.reset_peak_memory_stats()
    base = torch.cuda.memory_allocated()
    loss.backward()
    torch.cuda.synchronize()
    return (torch.cuda.max_memory_allocated() - base) / 2 ** 20


def relative(a, b):
    return float((a.double() - b.double()).abs().max()) / max(float(b.abs().max()), 1e-300)


def one_layer(name, n_in, n_out, S, B, per_sample, repeats, warmup):
    dev = torch.device("cuda", 0)
    torch.manual_seed(n_in + n_out)
    layer = WHVILinear(n_in, n_out, bias=True).to(dev)
    w = layer.weight_submodule
    w.diag_blocks = True
    x = torch.randn((S, B, n_in) if per_sample else (B, n_in), device=dev, requires_grad=per_sample)
    cot = torch.randn(S, B, n_out, device=dev)
    live = min(w.D_in, -(-n_out // 4) * 4)                           # columns of x under a written column
    moved = 4.0 * (S * B * n_out + (S if per_sample else 1) * B * live + (S * B * w.D_in if per_sample else 0))
    params = list(layer.parameters())

    def make_loss(flag):
        w.diag_blocks_backward = flag
        torch.manual_seed(1)
        out = layer.forward_mc(x, S, relu_in=per_sample)
        return (out * cot).sum() + layer._mc_kl

    def run(flag):
        for t in params + [x]:
            t.grad = None
        make_loss(flag).backward()

    grads = []
    for flag in (True, False):
        run(flag)
        grads.append([t.grad.clone() for t in params + ([x] if per_sample else [])])
    run(True)
    kernel = _hip.last_kernel()
    diff = max(relative(a, b) for a, b in zip(*grads))
    del grads
    peaks = {}
    for flag in (True, False):
        for t in params + [x]:
            t.grad = None
        peaks["flag_on" if flag else "flag_off"] = backward_peak(lambda: make_loss(flag))
    out = {"name": name, "n_in": n_in, "n_out": n_out, "D_in": w.D_in, "n_blocks": w.stack, "n_samples": S, "batch": B,
           "per_sample_input": per_sample, "bytes_moved_by_the_backward_launch": moved, "last_kernel": kernel,
           "max_relative_difference": diff, "backward_peak_MiB": peaks,
           "routes": measure({"flag_on": lambda: run(True), "flag_off": lambda: run(False), "copy_probe": probe(moved, dev)},
                             repeats, warmup)}
    return report(out)


def one_net(name, n_in, S, B, repeats, warmup):
    dev = torch.device("cuda", 0)
    torch.manual_seed(n_in)
    net = WHVIRegression([WHVILinear(n_in, 128, bias=True), nn.ReLU(), WHVILinear(128, 128, bias=True), nn.ReLU(),
                          WHVILinear(128, 2, bias=True)], train_samples=S).to(dev).train()
    x, y = torch.randn(B, n_in, device=dev), torch.randn(B, 2, device=dev)
    # what the two stacked layers' backward launches move (the square layer between them has whvi_diag_apply_bwd either way)
    first = net.sequential[0].weight_submodule
    moved = 4.0 * (S * B * 2 + S * B * 4 + S * B * 128)              # the output layer: g, one chunk of h, grad_h
    if getattr(first, "D_in", 0) > 8:
        moved += 4.0 * (S * B * 128 + B * first.D_in)                # the naval first layer: g and the shared input

    def make_loss(flag):
        net.set_stacked_diagonal(True, backward=flag)
        torch.manual_seed(1)
        return net.loss(x, y, n=10 * B)

    def run(flag):
        net.zero_grad(set_to_none=True)
        make_loss(flag).backward()

    grads = []
    for flag in (True, False):
        run(flag)
        grads.append([p.grad.clone() for p in net.parameters()])
    diff = max(relative(a, b) for a, b in zip(*grads))
    del grads
    peaks = {}
    for flag in (True, False):
        net.zero_grad(set_to_none=True)
        peaks["flag_on" if flag else "flag_off"] = backward_peak(lambda: make_loss(flag))
    out = {"name": name + " network, training pass", "n_in": n_in, "n_samples": S, "batch": B,
           "bytes_moved_by_the_backward_launches": moved, "max_relative_difference": diff, "backward_peak_MiB": peaks,
           "routes": measure({"flag_on": lambda: run(True), "flag_off": lambda: run(False), "copy_probe": probe(moved, dev)},
                             repeats, warmup)}
    return report(out)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--repeats", type=int, default=9)
    ap.add_argument("--warmup", type=int, default=20)
    ap.add_argument("--out", default=None)
    args = ap.parse_args()
    assert args.repeats >= 7, "at least 7 alternating repeats"
    results = [one_layer(*shape, args.repeats, args.warmup) for shape in LAYER_SHAPES]
    results += [one_net(*shape, args.repeats, args.warmup) for shape in NET_SHAPES]
    doc = {"tool": "tools/stacked_diag_bwd_rate.py", "argv": sys.argv[1:], "device": torch.cuda.get_device_name(0),
           "repeats": args.repeats, "warmup": args.warmup, "results": results}
    if args.out:
        os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
        with open(args.out, "w") as f:
            json.dump(doc, f, indent=1)
    return 0


if __name__ == "__main__":
    sys.exit(main())
