#!/usr/bin/env python3
"""tools/fused16_rate.py -- what the one-launch 16-bit fused pipeline (whvi_fused_shs_ex_f16 / _bf16) buys over the two
routes a user had before it, and how far it is from the copy ceiling.  One process, inputs resident, HIP events on the launch
stream, a warm-up of 30 launches per route (clocks ramp), then the routes ALTERNATE over the repeats; median and min-max per
route.

    python tools/fused16_rate.py --out profiles/r10/fused16_rate.json            # D = 2048 (config 3's shape), 512, 4096, 8192
    rocprofv3 --kernel-trace --stats -d DIR -o fused16 -- python tools/fused16_rate.py --d 2048 --out DIR/rate_under_trace.json

Shapes: (64 samples, batch, D) rows in 16 bits, 2 GiB in place (batch = 8192 at D = 2048).  Routes:
  fused16   the new launch, in place: 2 bytes read + 2 written per element
  upcast    x.float() -> whvi_fused_shs_ex_f32 in place -> .to(16 bit): (2+4) + (4+4) + (4+2) bytes
  chain     the unfused 16-bit chain: three multiplies and two fwht_rows, each reading 2 and writing 2 (five roundings)
  copy16    whvi_stream_copy_probe at the same bytes: the ceiling
  fused32 / copy32   the f32 fused kernel and the copy probe on the upcast buffer (4 GiB): the ratio the f32 kernel reaches
Rates are ALGORITHMIC bytes of the 16-bit problem (4 * rows * D) over the median time, for every 16-bit route."""
import argparse
import json
import os
import statistics
import sys

import torch

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
from whvi_amd import _hip  # noqa: E402

S = 64


def measure(routes, repeats, warmup, inner):
    for fn in routes.values():
        for _ in range(warmup):
            fn()
    torch.cuda.synchronize()
    times = {k: [] for k in routes}
    for _ in range(repeats):
        for name, fn in routes.items():                      # alternating: one measurement of every route per repeat
            e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
            e0.record()
            for _ in range(inner):
                fn()
            e1.record()
            e1.synchronize()
            times[name].append(e0.elapsed_time(e1) / inner)
    return times


def one_shape(dtype, d, gib, repeats, warmup, inner):
    dev = torch.device("cuda", 0)
    rows = int(gib * (1 << 30)) // (2 * d)
    batch = rows // S
    rows = batch * S
    g = torch.Generator(device=dev).manual_seed(d)
    x = torch.randn(rows, d, device=dev, generator=g).to(dtype)
    sign = lambda *shape: (torch.randint(0, 2, shape, device=dev, generator=g).float() * 2 - 1)     # noqa: E731
    a, b, c = sign(d), sign(S, d) / d, sign(d)               # an orthogonal map: values keep their size over any number of launches
    a16, b16, c16 = a.to(dtype), b.to(dtype), c.to(dtype)
    x32 = x.float()
    t = torch.empty_like(x)
    t3, b3 = t.view(S, batch, d), b16.view(S, 1, d)
    kernels = {}

    def fused16():
        _hip.fused_shs(x, a, b, c, n_samples=S, sample_stride=batch, out=x)

    def fused32():
        _hip.fused_shs(x32, a, b, c, n_samples=S, sample_stride=batch, out=x32)

    def upcast():
        w = x.float()
        _hip.fused_shs(w, a, b, c, n_samples=S, sample_stride=batch, out=w)
        return w.to(dtype)

    def chain():
        torch.mul(x, c16, out=t)
        _hip.fwht_rows(t, out=t)
        torch.mul(t3, b3, out=t3)
        _hip.fwht_rows(t, out=t)
        torch.mul(t, a16, out=t)

    routes = {"fused16": fused16, "upcast": upcast, "chain": chain, "copy16": lambda: _hip.stream_copy_probe(x, out=x),
              "fused32": fused32, "copy32": lambda: _hip.stream_copy_probe(x32, out=x32)}
    fused16()
    kernels["fused16"] = _hip.last_kernel()
    fused32()
    kernels["fused32"] = _hip.last_kernel()
    times = measure(routes, repeats, warmup, inner)
    alg = 4.0 * rows * d
    out = {"dtype": str(dtype).replace("torch.", ""), "D": d, "rows": rows, "n_samples": S, "batch": batch,
           "algorithmic_bytes": alg, "kernels": kernels, "routes": {}}
    for name, ts in times.items():
        nbytes = alg * (2 if name.endswith("32") else 1)     # the f32 routes move 4-byte elements
        med = statistics.median(ts)
        out["routes"][name] = {"ms_median": med, "ms_min": min(ts), "ms_max": max(ts), "TBps_median": nbytes / med / 1e9,
                               "TBps_min": nbytes / max(ts) / 1e9, "TBps_max": nbytes / min(ts) / 1e9, "ms": ts}
    r = out["routes"]
    out["fused16_over_copy16"] = r["copy16"]["ms_median"] / r["fused16"]["ms_median"]
    out["fused32_over_copy32"] = r["copy32"]["ms_median"] / r["fused32"]["ms_median"]
    out["speedup_vs_upcast"] = r["upcast"]["ms_median"] / r["fused16"]["ms_median"]
    out["speedup_vs_chain"] = r["chain"]["ms_median"] / r["fused16"]["ms_median"]
    out["faster_than_both_max_below_min"] = r["fused16"]["ms_max"] < min(r["upcast"]["ms_min"], r["chain"]["ms_min"])
    print(f"{out['dtype']:9s} D={d:5d} rows={rows}: fused16 {r['fused16']['TBps_median']:.2f} TB/s "
          f"[{r['fused16']['TBps_min']:.2f}-{r['fused16']['TBps_max']:.2f}] = {out['fused16_over_copy16']:.3f} x copy "
          f"({r['copy16']['TBps_median']:.2f}); f32 fused {out['fused32_over_copy32']:.3f} x copy; "
          f"{out['speedup_vs_upcast']:.2f} x upcast route, {out['speedup_vs_chain']:.2f} x 16-bit chain; "
          f"max below their min: {out['faster_than_both_max_below_min']}", flush=True)
    return out


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--d", type=int, nargs="*", default=[2048, 512, 4096, 8192])
    ap.add_argument("--dtypes", nargs="*", default=["float16", "bfloat16"])
    ap.add_argument("--gib", type=float, default=2.0)
    ap.add_argument("--repeats", type=int, default=9)
    ap.add_argument("--warmup", type=int, default=30)
    ap.add_argument("--inner", type=int, default=3)
    ap.add_argument("--out", default=None)
    args = ap.parse_args()
    assert args.repeats >= 7, "at least 7 alternating repeats"
    results = [one_shape(getattr(torch, dt), d, args.gib, args.repeats, args.warmup, args.inner) for d in args.d for dt in args.dtypes]
    doc = {"tool": "tools/fused16_rate.py", "argv": sys.argv[1:], "device": torch.cuda.get_device_name(0),
           "repeats": args.repeats, "warmup": args.warmup, "launches_per_measurement": args.inner, "results": results}
    if args.out:
        os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
        with open(args.out, "w") as f:
            json.dump(doc, f, indent=1)
    return 0


if __name__ == "__main__":
    sys.exit(main())
