#!/usr/bin/env python3
"""tools/fused_bwd_rate.py -- what the one-launch backward of the fused pipeline (whvi_fused_shs_bwd_f32,
``FastfoodFunction(..., fused_backward=True)``) buys over the chain it replaces.  One process, inputs resident, HIP events on
the launch stream, a warm-up of 30 backward passes per route (clocks ramp), then the two routes ALTERNATE over the repeats;
median and min-max per route.  The yardstick is the flag-off route of the same run.

    python tools/fused_bwd_rate.py --out profiles/r11/fused_bwd_rate.json

Shapes (D, samples, batch): config 3's (2048, 64, 8192); (512, 64, 32768) and (4096, 64, 4096) at the same 4 GiB per
activation; one small shape (1024, 1, 256), where a launch cannot fill the chip.  Every pass is the backward of
``FastfoodFunction`` with all of x, a, b, c wanting a gradient (its forward runs outside the timed region).  Per route also the
allocator's peak above what is held before the backward.  ``TBps`` of the fused route is 12 * D bytes per row -- x and
grad_y read, grad_x written -- over the median time of the whole backward (both launches and the allocations)."""
import argparse
import json
import os
import statistics
import sys

import torch

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
from whvi_amd import _hip  # noqa: E402
from whvi_amd.fastfood import FastfoodFunction  # noqa: E402

SHAPES = ((2048, 64, 8192), (512, 64, 32768), (4096, 64, 4096), (1024, 1, 256))


def one_shape(d, S, batch, repeats, warmup):
    dev = torch.device("cuda", 0)
    rows = S * batch
    g = torch.Generator(device=dev).manual_seed(d)
    x = torch.randn(rows, d, device=dev, generator=g).requires_grad_()
    gy = torch.randn(rows, d, device=dev, generator=g)
    a, c = (torch.randn(d, device=dev, generator=g).mul_(0.01).requires_grad_() for _ in range(2))
    b = torch.randn(S, d, device=dev, generator=g).requires_grad_()
    kernels, peaks, times = {}, {}, {"chain": [], "fused": []}

    def backward(flag, timed):
        y = FastfoodFunction.apply(x, a, b, c, S, batch, False, False, flag)
        e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        if timed == "peak":
            torch.cuda.synchronize()
            torch.cuda.reset_peak_memory_stats(dev)
            held = torch.cuda.memory_allocated(dev)
        e0.record()
        grads = torch.autograd.grad(y, (x, a, b, c), gy)
        e1.record()
        e1.synchronize()
        if timed == "peak":
            return torch.cuda.max_memory_allocated(dev) - held
        del grads
        return e0.elapsed_time(e1)

    # the backward runs on autograd's thread and whvi_last_kernel is per thread: a hook on x asks there
    seen = []
    hook = x.register_hook(lambda grad: seen.append(_hip.last_kernel()))
    for name, flag in (("chain", False), ("fused", True)):
        peaks[name] = backward(flag, "peak")
        kernels[name] = seen[-1]
    hook.remove()
    for name, flag in (("chain", False), ("fused", True)):
        for _ in range(warmup):
            backward(flag, None)
    for _ in range(repeats):
        for name, flag in (("chain", False), ("fused", True)):      # alternating: one measurement of each route per repeat
            times[name].append(backward(flag, "time"))
    act = 4.0 * rows * d
    out = {"D": d, "n_samples": S, "batch": batch, "rows": rows, "activation_bytes": act, "kernels": kernels,
           "workspace_bytes": int(_hip.lib().whvi_fused_shs_bwd_workspace(S, batch, d.bit_length() - 1)), "routes": {}}
    for name, ts in times.items():
        med = statistics.median(ts)
        out["routes"][name] = {"ms_median": med, "ms_min": min(ts), "ms_max": max(ts), "ms": ts,
                               "peak_bytes_above_held": peaks[name], "peak_activations": peaks[name] / act}
    f = out["routes"]["fused"]
    f["TBps_median"], f["TBps_min"], f["TBps_max"] = (3 * act / t / 1e9 for t in (f["ms_median"], f["ms_max"], f["ms_min"]))
    out["speedup"] = out["routes"]["chain"]["ms_median"] / f["ms_median"]
    out["fused_max_below_chain_min"] = f["ms_max"] < out["routes"]["chain"]["ms_min"]
    print(f"D={d:5d} S={S:3d} B={batch:6d}: chain {out['routes']['chain']['ms_median']:.3f} ms "
          f"[{out['routes']['chain']['ms_min']:.3f}-{out['routes']['chain']['ms_max']:.3f}], peak "
          f"{out['routes']['chain']['peak_activations']:.2f} A; fused {f['ms_median']:.3f} ms [{f['ms_min']:.3f}-{f['ms_max']:.3f}], "
          f"peak {f['peak_activations']:.2f} A, {f['TBps_median']:.2f} TB/s at 12 D bytes per row; speedup {out['speedup']:.2f}",
          flush=True)
    return out


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--repeats", type=int, default=9)
    ap.add_argument("--warmup", type=int, default=30)
    ap.add_argument("--out", default=None)
    args = ap.parse_args()
    assert args.repeats >= 7, "at least 7 alternating repeats"
    results = [one_shape(d, S, batch, args.repeats, args.warmup) for d, S, batch in SHAPES]
    doc = {"tool": "tools/fused_bwd_rate.py", "argv": sys.argv[1:], "device": torch.cuda.get_device_name(0),
           "repeats": args.repeats, "warmup": args.warmup, "results": results}
    if args.out:
        os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
        with open(args.out, "w") as f:
            json.dump(doc, f, indent=1)
    return 0


if __name__ == "__main__":
    sys.exit(main())
