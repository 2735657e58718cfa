#!/usr/bin/env python3
"""tools/fused_bwd_rate.py -- what the one-launch backward of the fused pipeline (whvi_fused_shs_bwd_f32 / _f16 / _bf16,
``FastfoodFunction(..., fused_backward=True)``) buys over the chain it replaces.  One process, inputs resident, HIP events on
the launch stream, a warm-up of 30 backward passes per route (clocks ramp), then the routes ALTERNATE over the repeats;
median and min-max per route.  The yardstick is the flag-off route of the same run.

    python tools/fused_bwd_rate.py --out profiles/r11/fused_bwd_rate.json
    python tools/fused_bwd_rate.py --dtype float16 --out profiles/r12/fused_bwd16_rate.json
    python tools/fused_bwd_rate.py --dtype bfloat16 --out profiles/r12/fused_bwd16_rate_bf16.json

Shapes (D, samples, batch): config 3's (2048, 64, 8192); (512, 64, 32768) and (4096, 64, 4096) at the same bytes per
activation (4 GiB in float32, 2 GiB in 16 bits); one small shape (1024, 1, 256), where a launch cannot fill the chip.  Every pass
is the backward of ``FastfoodFunction`` with all of x, a, b, c wanting a gradient (its forward runs outside the timed region).
Per route also the allocator's peak above what is held before the backward.  ``TBps`` of the fused route is 3 activations --
x and grad_y read, grad_x written: 12 * D bytes per row in float32, 6 * D in 16 bits -- over the median time of the whole
backward (both launches and the allocations).

Routes.  float32: ``chain`` (flag off) and ``fused``.  ``--dtype float16 | bfloat16`` (``keep_half`` activations, float32
parameters): ``fused`` is the 16-bit launch (both flags), ``chain`` is ``keep_half`` with the flag off -- two float32 upcasts
and the float32 chain -- ``fused_f32_upcast`` is the float32 one-launch backward on tensors upcast outside the timed region
(what the 16-bit launch would cost at 12 * D bytes per row), and ``copy_probe`` is ``whvi_stream_copy_probe`` moving the same
6 * D bytes per row (3 * D read, 3 * D written) with no arithmetic."""
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
DTYPES = {"float32": torch.float32, "float16": torch.float16, "bfloat16": torch.bfloat16}


def one_shape(d, S, batch, repeats, warmup, dtype=torch.float32):
    dev = torch.device("cuda", 0)
    rows = S * batch
    half = dtype != torch.float32
    g = torch.Generator(device=dev).manual_seed(d)
    x = torch.randn(rows, d, device=dev, generator=g).to(dtype).requires_grad_()
    gy = torch.randn(rows, d, device=dev, generator=g).to(dtype)
    # (16-bit: a and b at 1 / sqrt(D) so that fp16 results stay finite)
    vec_scale = d ** -0.5 if half else 0.01
    a = torch.randn(d, device=dev, generator=g).mul_(vec_scale).requires_grad_()
    c = torch.randn(d, device=dev, generator=g).mul_(1.0 if half else 0.01).requires_grad_()
    b = torch.randn(S, d, device=dev, generator=g).mul_(vec_scale if half else 1.0).requires_grad_()
    kernels, peaks = {}, {}
    elem = 2 if half else 4
    act = float(elem) * rows * d

    # every route: (x, grad_y, keep_half, fused_backward) of one FastfoodFunction backward
    routes = {"chain": (x, gy, half, False), "fused": (x, gy, half, True)}
    if half:
        x32, gy32 = x.detach().float().requires_grad_(), gy.float()
        routes["fused_f32_upcast"] = (x32, gy32, False, True)
        probe_src = torch.empty(3 * rows * d, dtype=torch.uint8, device=dev).random_()
        probe_dst = torch.empty_like(probe_src)
    times = {name: [] for name in routes}

    def backward(name, timed):
        xr, gr, keep_half, fused = routes[name]
        y = FastfoodFunction.apply(xr, a, b, c, S, batch, False, keep_half, fused)
        e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        if timed == "peak":
            torch.cuda.synchronize()
            torch.cuda.reset_peak_memory_stats(dev)
            held = torch.cuda.memory_allocated(dev)
        e0.record()
        grads = torch.autograd.grad(y, (xr, a, b, c), gr)
        e1.record()
        e1.synchronize()
        if timed == "peak":
            return torch.cuda.max_memory_allocated(dev) - held
        del grads
        return e0.elapsed_time(e1)

    def probe():
        e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        e0.record()
        _hip.stream_copy_probe(probe_src, probe_dst)
        e1.record()
        e1.synchronize()
        return e0.elapsed_time(e1)

    # the backward runs on autograd's thread and whvi_last_kernel is per thread: a hook on x asks there
    for name in routes:
        seen = []
        hook = routes[name][0].register_hook(lambda grad: seen.append(_hip.last_kernel()))
        peaks[name] = backward(name, "peak")
        kernels[name] = seen[-1]
        hook.remove()
    for name in routes:
        for _ in range(warmup):
            backward(name, None)
    if half:
        times["copy_probe"] = []
        for _ in range(warmup):
            probe()
    for _ in range(repeats):
        for name in routes:                                         # alternating: one measurement of each route per repeat
            times[name].append(backward(name, "time"))
        if half:
            times["copy_probe"].append(probe())
    out = {"D": d, "n_samples": S, "batch": batch, "rows": rows, "dtype": str(dtype).replace("torch.", ""),
           "activation_bytes": act, "kernels": kernels,
           "workspace_bytes": int(_hip.lib().whvi_fused_shs_bwd_workspace(S, batch, d.bit_length() - 1)), "routes": {}}
    for name, ts in times.items():
        med = statistics.median(ts)
        out["routes"][name] = {"ms_median": med, "ms_min": min(ts), "ms_max": max(ts), "ms": ts}
        if name in peaks:
            out["routes"][name].update(peak_bytes_above_held=peaks[name], peak_activations=peaks[name] / act)
    for name in ("fused", "copy_probe"):
        if name in out["routes"]:                                   # 3 activations of this dtype: x, grad_y, grad_x
            r = out["routes"][name]
            r["TBps_median"], r["TBps_min"], r["TBps_max"] = (3 * act / t / 1e9 for t in (r["ms_median"], r["ms_max"], r["ms_min"]))
    f = out["routes"]["fused"]
    out["speedup"] = out["routes"]["chain"]["ms_median"] / f["ms_median"]
    out["fused_max_below_chain_min"] = f["ms_max"] < out["routes"]["chain"]["ms_min"]
    print(f"{out['dtype']} D={d:5d} S={S:3d} B={batch:6d}: chain {out['routes']['chain']['ms_median']:.3f} ms "
          f"[{out['routes']['chain']['ms_min']:.3f}-{out['routes']['chain']['ms_max']:.3f}], peak "
          f"{out['routes']['chain']['peak_activations']:.2f} A; fused {f['ms_median']:.3f} ms [{f['ms_min']:.3f}-{f['ms_max']:.3f}], "
          f"peak {f['peak_activations']:.2f} A, {f['TBps_median']:.2f} TB/s at {3 * elem} D bytes per row; speedup {out['speedup']:.2f}",
          flush=True)
    for name in ("fused_f32_upcast", "copy_probe"):
        if name in out["routes"]:
            r = out["routes"][name]
            print(f"    {name}: {r['ms_median']:.3f} ms [{r['ms_min']:.3f}-{r['ms_max']:.3f}]" +
                  (f", peak {r['peak_activations']:.2f} A (of 16 bits)" if "peak_activations" in r else "") +
                  (f", {r['TBps_median']:.2f} TB/s" if "TBps_median" in r else ""), flush=True)
    return out


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--repeats", type=int, default=9)
    ap.add_argument("--warmup", type=int, default=30)
    ap.add_argument("--dtype", choices=sorted(DTYPES), default="float32")
    ap.add_argument("--out", default=None)
    args = ap.parse_args()
    assert args.repeats >= 7, "at least 7 alternating repeats"
    results = [one_shape(d, S, batch, args.repeats, args.warmup, DTYPES[args.dtype]) for d, S, batch in SHAPES]
    doc = {"tool": "tools/fused_bwd_rate.py", "argv": sys.argv[1:], "device": torch.cuda.get_device_name(0),
           "repeats": args.repeats, "warmup": args.warmup, "results": results}
    if args.out:
        os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
        with open(args.out, "w") as f:
            json.dump(doc, f, indent=1)
    return 0


if __name__ == "__main__":
    sys.exit(main())
