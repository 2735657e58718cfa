#!/usr/bin/env python3
"""tools/fastfood_stacked_layer_rate.py -- what folding the bias, the ReLU and the narrowing into the rectangular fastfood
layer's launch (whvi_fused_shs_stacked_layer_f32, ``WHVIFastfoodStackedMatrix.fused_epilogue``) buys over the passes it
replaces.  The protocol of tools/fastfood_stacked_rate.py: one process, inputs resident, HIP events on the launch stream, a
warm-up of 30 passes per route (clocks ramp), then the routes ALTERNATE over the repeats; median and min-max per route.  The
yardstick is the unfolded route of the same run.

    python tools/fastfood_stacked_layer_rate.py --out profiles/r16/fastfood_stacked_layer_rate.json
    python tools/fastfood_stacked_layer_rate.py --dtype float16 bfloat16 --out profiles/r20/fastfood_stacked_layer16_rate.json

``--dtype float16 | bfloat16`` (default float32; several may be given, one result per shape and dtype): the 16-bit launch
``_hip.fused_shs_stacked_layer16`` (``WHVIFastfoodStackedMatrix.fused_epilogue16``) against what the layer runs
with that flag off -- ``_hip.fused_shs_stacked16``, ``+ bias.to(dtype)``, ``torch.relu``, the ``.contiguous()`` -- with 2-byte
activations throughout, float32 vectors and bias.  There the folded values are NOT the unfolded ones (one rounding instead of
up to three): ``folded_equals_unfolded`` is recorded as it comes out and ``folded_equals_float32_launch_cast_once`` holds the
folded launch to ``_hip.fused_shs_stacked_layer(x.float(), ...).to(dtype)``.

Routes:
  ``folded``       ``_hip.fused_shs_stacked_layer`` with a bias and ``relu_out`` (and ``n_cols`` where the shape is narrowed): a row
                   read once, ``n_cols`` columns written;
  ``unfolded``     what the layer runs without the flag: ``_hip.fused_shs_stacked``, then ``+ bias``, then ``torch.relu`` -- each
                   a pass that reads and writes J * D per row -- and, on a narrowed shape, the ``.contiguous()`` of the
                   ``[:, :n_cols]`` view that the next layer pays;
  ``folded_bias``  the new launch with nothing but the bias;
  ``launch_add``   ``_hip.fused_shs_stacked`` then ``+ bias``;
  ``copy_probe``   ``whvi_stream_copy_probe`` moving (1 + J) * D * 4 bytes per row with no arithmetic (half read, half written).
Shapes (D, J, samples, batch, shared input, n_cols): (1024, 4, 16, 8192) with its own and with a shared ``x``; (128, 4, 64,
1000); (2048, 2, 16, 4096); (256, 4, 16, 8192) narrowed to 800 columns.  ``TBps`` counts (D + n_cols) * 4 bytes per row -- what
the folded launch moves -- over the route's time.  Acceptance: at (1024, 4, 16, 8192) with its own ``x`` the folded launch's
slowest repeat lies below the unfolded route's fastest."""
import argparse
import json
import os
import statistics
import sys

import torch

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
from whvi_amd import _hip  # noqa: E402

SHAPES = ((1024, 4, 16, 8192, False, None), (1024, 4, 16, 8192, True, None), (128, 4, 64, 1000, False, None),
          (2048, 2, 16, 4096, False, None), (256, 4, 16, 8192, False, 800))


def one_shape(d, J, S, batch, shared, n_cols, repeats, warmup, dtype=torch.float32):
    dev = torch.device("cuda", 0)
    rows = S * batch
    narrowed = n_cols is not None
    n_cols = J * d if n_cols is None else n_cols
    g = torch.Generator(device=dev).manual_seed(d + J)
    half = dtype != torch.float32
    size = 2 if half else 4
    launch, layer = (_hip.fused_shs_stacked16, _hip.fused_shs_stacked_layer16) if half else (_hip.fused_shs_stacked, _hip.fused_shs_stacked_layer)
    x = torch.randn(batch if shared else rows, d, device=dev, generator=g).to(dtype)
    a = torch.randn(J, d, device=dev, generator=g).mul_(0.01)
    c = torch.randn(J, d, device=dev, generator=g).mul_(0.01)
    b = torch.randn(J, S, d, device=dev, generator=g)
    bias = torch.randn(1, J * d, device=dev, generator=g).mul_(0.1)
    moved = float(size) * rows * (d + n_cols)
    probe_src = torch.empty(size // 2 * rows * d * (1 + J), dtype=torch.uint8, device=dev).random_()
    probe_dst = torch.empty_like(probe_src)

    def unfolded(relu):
        y = launch(x, a, b, c, S, batch, shared=shared) + (bias.to(dtype) if half else bias)
        if relu:
            y = torch.relu(y)
        return y[:, :n_cols].contiguous() if narrowed else y

    routes = {
        "folded": lambda: layer(x, a, b, c, S, batch, bias=bias, n_cols=n_cols, relu_out=True, shared=shared),
        "unfolded": lambda: unfolded(True),
        "folded_bias": lambda: layer(x, a, b, c, S, batch, bias=bias, n_cols=n_cols, shared=shared),
        "launch_add": lambda: unfolded(False),
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

    y = routes["folded"]()
    kernel = _hip.last_kernel()
    same = bool(torch.equal(y + 0.0, routes["unfolded"]() + 0.0)) and bool(torch.equal(routes["folded_bias"](), routes["launch_add"]()))
    cast_once = None
    if half:
        ref = _hip.fused_shs_stacked_layer(x.float(), a, b, c, S, batch, bias=bias, n_cols=n_cols, relu_out=True, shared=shared).to(dtype)
        cast_once = bool(torch.equal(y + 0.0, ref + 0.0))
        del ref
    del y
    for name in routes:
        for _ in range(warmup):
            timed(name)
    times = {name: [] for name in routes}
    for _ in range(repeats):
        for name in routes:                                         # alternating: one measurement of each route per repeat
            times[name].append(timed(name))
    out = {"dtype": str(dtype).replace("torch.", ""), "D": d, "n_blocks": J, "n_samples": S, "batch": batch, "rows": rows, "shared_x": shared, "n_cols": n_cols,
           "bytes_moved": moved, "copy_probe_bytes": 2.0 * probe_src.numel(), "kernel": kernel, "folded_equals_unfolded": same,
           "routes": {}}
    if half:
        out["folded_equals_float32_launch_cast_once"] = cast_once
    for name, ts in times.items():
        med = statistics.median(ts)
        out["routes"][name] = {"ms_median": med, "ms_min": min(ts), "ms_max": max(ts), "ms": ts,
                               "TBps_median": moved / med / 1e9, "TBps_min": moved / max(ts) / 1e9, "TBps_max": moved / min(ts) / 1e9}
    r = out["routes"]
    out["speedup"] = r["unfolded"]["ms_median"] / r["folded"]["ms_median"]
    out["folded_max_below_unfolded_min"] = r["folded"]["ms_max"] < r["unfolded"]["ms_min"]
    out["speedup_bias_only"] = r["launch_add"]["ms_median"] / r["folded_bias"]["ms_median"]
    out["folded_bias_max_below_launch_add_min"] = r["folded_bias"]["ms_max"] < r["launch_add"]["ms_min"]
    out["folded_over_copy"] = r["folded"]["ms_median"] / r["copy_probe"]["ms_median"]
    print(f"{out['dtype']} D={d:5d} J={J} S={S:3d} B={batch:5d} shared={int(shared)} n_cols={n_cols}: " +
          "; ".join(f"{n} {v['ms_median']:.3f} ms [{v['ms_min']:.3f}-{v['ms_max']:.3f}]" for n, v in r.items()) +
          f"; speedup {out['speedup']:.2f} (bias only {out['speedup_bias_only']:.2f}), folded / copy {out['folded_over_copy']:.2f}, "
          f"slowest folded below fastest unfolded: {out['folded_max_below_unfolded_min']}, same values: {same}", flush=True)
    return out


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--repeats", type=int, default=9)
    ap.add_argument("--warmup", type=int, default=30)
    ap.add_argument("--out", default=None)
    ap.add_argument("--dtype", nargs="+", default=["float32"], choices=("float32", "float16", "bfloat16"))
    args = ap.parse_args()
    assert args.repeats >= 7, "at least 7 alternating repeats"
    results = [one_shape(*shape, args.repeats, args.warmup, getattr(torch, name)) for name in args.dtype for shape in SHAPES]
    doc = {"tool": "tools/fastfood_stacked_layer_rate.py", "argv": sys.argv[1:], "device": torch.cuda.get_device_name(0),
           "repeats": args.repeats, "warmup": args.warmup, "results": results}
    if args.out:
        os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
        with open(args.out, "w") as f:
            json.dump(doc, f, indent=1)
    return 0


if __name__ == "__main__":
    sys.exit(main())
