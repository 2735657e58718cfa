#!/usr/bin/env python3
"""tools/stacked_diag_rate.py -- what the one-launch stacked diagonal route (``WHVIStackedMatrix.diag_blocks``,
whvi_diag_apply_stacked_f32) buys over the route it replaces (``WBarFunction`` weights + ``torch.matmul``).  The protocol of
tools/fastfood_stacked_rate.py: one process, operands resident, HIP events on the launch stream, a warm-up per route (clocks
ramp), then the routes ALTERNATE over the repeats; median and min-max per route.  Beside every number: ``copy_probe``,
whvi_stream_copy_probe moving the bytes the one launch moves (the input read once, n_out floats per row written) with no
arithmetic.

    python tools/stacked_diag_rate.py --out profiles/r22/stacked_diag_rate.json

Shapes (all under ``torch.no_grad()``, the predictive pass):
  layers    ``WHVILinear(n_in, n_out, bias=True).forward_mc`` alone: the naval first layer 16 -> 128 on a shared (1000, 16)
            input and the two-target output layer 128 -> 2 on (64, 1000, 128) activations (64 samples, 1000 rows: the UCI
            evaluation); 1024 -> 2 at 16 x 45730; 128 -> 512 at 16 x 8192 (per-sample input) and 16 -> 1024 at 16 x 8192 (shared);
  networks  the whole predictive pass of the energy (8 features) and naval (16) networks n_in -> 128 -> 128 -> 2, biases and
            ReLUs, 64 samples, 1000 rows, ``set_stacked_diagonal`` on against off (the energy network's first layer keeps
            whvi_small_k_apply either way).
Both routes draw the same way, so the draws are part of both times."""
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

# (name, n_in, n_out, samples, rows, per-sample input)
LAYER_SHAPES = (("naval first layer", 16, 128, 64, 1000, False), ("two-target output layer", 128, 2, 64, 1000, True),
                ("config-4-sized output layer", 1024, 2, 16, 45730, True), ("widening layer", 128, 512, 16, 8192, True),
                ("wide first layer", 16, 1024, 16, 8192, False))
NET_SHAPES = (("energy", 8, 64, 1000), ("naval", 16, 64, 1000))


def measure(routes, repeats, warmup):
    def timed(name):
        e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        e0.record()
        out = routes[name]()
        e1.record()
        e1.synchronize()
        del out
        return e0.elapsed_time(e1)

    for name in routes:
        for _ in range(warmup):
            timed(name)
    times = {name: [] for name in routes}
    for _ in range(repeats):
        for name in routes:                                         # alternating: one measurement of each route per repeat
            times[name].append(timed(name))
    return {name: {"ms_median": statistics.median(ts), "ms_min": min(ts), "ms_max": max(ts), "ms": ts} for name, ts in times.items()}


def probe(n_bytes, dev):
    half = max(16, int(n_bytes) // 2 // 16 * 16)                    # the probe reads `half` bytes and writes as many
    src = torch.empty(half, dtype=torch.uint8, device=dev).random_()
    dst = torch.empty_like(src)
    return lambda: _hip.stream_copy_probe(src, dst)


def report(out):
    r = out["routes"]
    out["speedup"] = r["flag_off"]["ms_median"] / r["flag_on"]["ms_median"]
    out["flag_on_max_below_flag_off_min"] = r["flag_on"]["ms_max"] < r["flag_off"]["ms_min"]
    out["flag_on_over_copy"] = r["flag_on"]["ms_median"] / r["copy_probe"]["ms_median"]
    print(f"{out['name']:28s} " + "; ".join(f"{n} {v['ms_median']:.3f} ms [{v['ms_min']:.3f}-{v['ms_max']:.3f}]" for n, v in r.items()) +
          f"; speedup {out['speedup']:.2f}, flag on / copy {out['flag_on_over_copy']:.2f}, same values: {out['same_values']}", flush=True)
    return out


def same(a, b):
    return bool(((a == b) | (a.isnan() & b.isnan())).all())


def one_layer(name, n_in, n_out, S, B, per_sample, repeats, warmup):
    dev = torch.device("cuda", 0)
    torch.manual_seed(n_in + n_out)
    layer = WHVILinear(n_in, n_out, bias=True).to(dev)
    w = layer.weight_submodule
    x = torch.randn((S, B, n_in) if per_sample else (B, n_in), device=dev)
    moved = 4.0 * (x.numel() + S * B * n_out)

    def run(flag):
        w.diag_blocks = flag
        with torch.no_grad():
            return layer.forward_mc(x, S)

    torch.manual_seed(1)
    on = run(True)
    kernel = _hip.last_kernel()
    torch.manual_seed(1)
    same_values = same(on, run(False))
    del on
    out = {"name": name, "n_in": n_in, "n_out": n_out, "D_in": w.D_in, "n_blocks": w.stack, "n_samples": S, "batch": B,
           "per_sample_input": per_sample, "bytes_moved_by_the_launch": moved, "kernel": kernel, "same_values": same_values,
           "routes": measure({"flag_on": lambda: run(True), "flag_off": lambda: run(False), "copy_probe": probe(moved, dev)},
                             repeats, warmup)}
    out["flag_on_TBps_median"] = moved / out["routes"]["flag_on"]["ms_median"] / 1e9
    return report(out)


def one_net(name, n_in, S, B, repeats, warmup):
    dev = torch.device("cuda", 0)
    torch.manual_seed(n_in)
    net = WHVIRegression([WHVILinear(n_in, 128, bias=True), nn.ReLU(), WHVILinear(128, 128, bias=True), nn.ReLU(),
                          WHVILinear(128, 2, bias=True)], eval_samples=S).to(dev).eval()
    x = torch.randn(B, n_in, device=dev)
    # what the flag-on pass moves: x once, the two (S, B, 128) activations written and read, the (S, B, 2) result
    moved = 4.0 * (x.numel() + 4 * S * B * 128 + S * B * 2)

    def run(flag):
        net.set_stacked_diagonal(flag)
        with torch.no_grad():
            return net.forward_batched(x, S)

    torch.manual_seed(1)
    on = run(True)
    torch.manual_seed(1)
    same_values = same(on, run(False))
    out = {"name": name + " network, predictive pass", "n_in": n_in, "n_samples": S, "batch": B, "bytes_moved_by_the_pass": moved,
           "same_values": same_values,
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
    doc = {"tool": "tools/stacked_diag_rate.py", "argv": sys.argv[1:], "device": torch.cuda.get_device_name(0),
           "repeats": args.repeats, "warmup": args.warmup, "results": results}
    if args.out:
        os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
        with open(args.out, "w") as f:
            json.dump(doc, f, indent=1)
    return 0


if __name__ == "__main__":
    sys.exit(main())
