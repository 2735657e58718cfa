#!/usr/bin/env python3
"""tools/fastfood_stacked16_rate.py -- what the one-launch rectangular fastfood layer on 16-bit activations
(whvi_fused_shs_stacked_f16 / _bf16, ``FastfoodStackedFunction`` with ``keep_half``) buys over the route it replaces.  The
protocol of tools/fastfood_stacked_rate.py: one process, inputs resident, HIP events on the launch stream, a warm-up of 30
passes per route (clocks ramp), then the routes ALTERNATE over the repeats; median and min-max per route.  The yardstick is
the composed route of the same run.

    python tools/fastfood_stacked16_rate.py --out profiles/r18/fastfood_stacked16_rate.json

Routes, per storage type (float16, bfloat16):
  ``launch``     ``_hip.fused_shs_stacked16``: a row read once, J segments written -- (1 + J) * D * 2 bytes per row (J * D * 2
                 with a shared input, which stays in cache);
  ``composed``   what ``FastfoodStackedFunction`` runs under ``keep_half`` where the launch does not exist: ``torch.cat`` of J
                 per-block passes of ``whvi_amd.fastfood._pipeline(..., keep_half=True)`` -- J 16-bit launches that each read
                 the row and write D, a concatenation that reads and writes J * D again, and with a shared input one
                 ``x.repeat(n_samples, 1)`` per block in front (the 16-bit launch has no shared-source form);
  ``copy_probe`` ``whvi_stream_copy_probe`` moving the same (1 + J) * D * 2 bytes per row with no arithmetic (half of them read,
                 half written).
Shapes (D, J, samples, batch, shared input): (1024, 4, 16, 8192) with its own and with a shared ``x``; (2048, 2, 16, 8192);
(128, 4, 64, 1000).  ``TBps`` counts (1 + J) * D * 2 bytes per row over the route's time.  The bar is relative:
``launch_max_below_composed_min`` -- the launch's slowest repeat against the composed route's fastest."""
import argparse
import json
import os
import statistics
import sys

import torch

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
from whvi_amd import _hip  # noqa: E402
from whvi_amd.fastfood import _pipeline  # noqa: E402

SHAPES = ((1024, 4, 16, 8192, False), (1024, 4, 16, 8192, True), (2048, 2, 16, 8192, False), (128, 4, 64, 1000, False))
DTYPES = {"float16": torch.float16, "bfloat16": torch.bfloat16}


def one_shape(dtype_name, d, J, S, batch, shared, repeats, warmup):
    dev = torch.device("cuda", 0)
    dtype = DTYPES[dtype_name]
    rows = S * batch
    g = torch.Generator(device=dev).manual_seed(d + J)
    x = torch.randn(batch if shared else rows, d, device=dev, generator=g).to(dtype)
    a = torch.randn(J, d, device=dev, generator=g).mul_(d ** -0.5)
    b = torch.randn(J, S, d, device=dev, generator=g).mul_(d ** -0.5)
    c = torch.randn(J, d, device=dev, generator=g)
    moved = 2.0 * rows * d * (1 + J)
    probe_src = torch.empty(int(moved) // 2, dtype=torch.uint8, device=dev).random_()
    probe_dst = torch.empty_like(probe_src)

    routes = {
        "launch": lambda: _hip.fused_shs_stacked16(x, a, b, c, S, batch, shared=shared),
        "composed": lambda: torch.cat([_pipeline(x, a[j], b[j], c[j], S, batch, shared, True) for j in range(J)], dim=1),
        "copy_probe": lambda: _hip.stream_copy_probe(probe_src, probe_dst),
    }

    def timed(name):
        e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        e0.record()
        out = routes[name]()
        e1.record()
        e1.synchronize()
        del out
        return e0.elapsed_time(e1)

    y = routes["launch"]()
    kernel = _hip.last_kernel()
    same = bool(torch.equal(y + 0.0, routes["composed"]() + 0.0))
    del y
    for name in routes:
        for _ in range(warmup):
            timed(name)
    times = {name: [] for name in routes}
    for _ in range(repeats):
        for name in routes:                                         # alternating: one measurement of each route per repeat
            times[name].append(timed(name))
    out = {"dtype": dtype_name, "D": d, "n_blocks": J, "n_samples": S, "batch": batch, "rows": rows, "shared_x": shared,
           "bytes_moved": moved, "kernel": kernel, "launch_equals_composed": same, "routes": {}}
    for name, ts in times.items():
        med = statistics.median(ts)
        out["routes"][name] = {"ms_median": med, "ms_min": min(ts), "ms_max": max(ts), "ms": ts,
                               "TBps_median": moved / med / 1e9, "TBps_min": moved / max(ts) / 1e9, "TBps_max": moved / min(ts) / 1e9}
    r = out["routes"]
    out["speedup"] = r["composed"]["ms_median"] / r["launch"]["ms_median"]
    out["launch_max_below_composed_min"] = r["launch"]["ms_max"] < r["composed"]["ms_min"]
    out["launch_over_copy"] = r["launch"]["ms_median"] / r["copy_probe"]["ms_median"]
    print(f"{dtype_name:8s} D={d:5d} J={J} S={S:3d} B={batch:5d} shared={int(shared)}: " +
          "; ".join(f"{n} {v['ms_median']:.3f} ms [{v['ms_min']:.3f}-{v['ms_max']:.3f}] {v['TBps_median']:.2f} TB/s" for n, v in r.items()) +
          f"; speedup {out['speedup']:.2f}, launch / copy {out['launch_over_copy']:.2f}, slowest launch below fastest composed: "
          f"{out['launch_max_below_composed_min']}, same values: {same}", flush=True)
    return out


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--repeats", type=int, default=9)
    ap.add_argument("--warmup", type=int, default=30)
    ap.add_argument("--dtypes", default="float16,bfloat16")
    ap.add_argument("--out", default=None)
    args = ap.parse_args()
    assert args.repeats >= 7, "at least 7 alternating repeats"
    results = [one_shape(name, *shape, args.repeats, args.warmup) for name in args.dtypes.split(",") for shape in SHAPES]
    doc = {"tool": "tools/fastfood_stacked16_rate.py", "argv": sys.argv[1:], "device": torch.cuda.get_device_name(0),
           "repeats": args.repeats, "warmup": args.warmup, "results": results}
    if args.out:
        os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
        with open(args.out, "w") as f:
            json.dump(doc, f, indent=1)
    return 0


if __name__ == "__main__":
    sys.exit(main())
