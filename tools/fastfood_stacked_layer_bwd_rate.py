#!/usr/bin/env python3
"""tools/fastfood_stacked_layer_bwd_rate.py -- what the one-launch backward of the rectangular fastfood layer with its epilogue
(whvi_fused_shs_stacked_layer_bwd_f32, ``FastfoodStackedLayerFunction(..., fused_backward=True, fused_epilogue_backward=True)``)
buys over the composed backward it replaces.  One process, inputs resident, HIP events on the launch stream around the whole
backward of ``FastfoodStackedLayerFunction`` (its forward runs outside the timed region), a warm-up of 30 backward passes per
route (clocks ramp), then the routes ALTERNATE over the repeats; median and min-max per route.  The yardstick is the composed
route of the same run.

    python tools/fastfood_stacked_layer_bwd_rate.py --out profiles/r17/fastfood_stacked_layer_bwd_rate.json

Routes: ``launch`` (both backward flags on); ``composed`` (``fused_backward`` on, ``fused_epilogue_backward`` off:
``threshold_backward``, the row sum, ``F.pad``, ``relu(x)``, whvi_fused_shs_stacked_bwd_f32, ``threshold_backward`` -- what the
layer ran before the launch existed and still runs without the flag); ``copy_probe``: ``whvi_stream_copy_probe`` moving the
launch's bytes (half read, half written) with no arithmetic.  Per route also the allocator's peak above what is held before the
backward.  The launch's bytes per row: ``4 * (n_cols * (1 + relu_out) + D * (x not shared) + D * (grad_x wanted))``.

Shapes (D, J, samples, batch, shared x, n_cols): (1024, 4, 16, 8192) with an input of its own and with a shared one;
(128, 4, 64, 1000); (2048, 2, 16, 4096); (256, 4, 16, 8192) narrowed to 800 columns -- each with a bias and both ReLUs, and the
first also with a bias only (a case the Function keeps composed -- this measurement is why -- so there both routes are timed as
the calls themselves: ``_hip.fused_shs_stacked_layer_bwd`` against ``grad_y.sum(0)`` and ``_hip.fused_shs_stacked_bwd``).  All of x, a, b, c, bias want a gradient, except at the shared shape: a shared x that wants a
gradient keeps the composed backward on every route, so there x is data -- a network's first layer.

``--dtype float16 bfloat16`` times the same six shapes on 16-bit activations instead (whvi_fused_shs_stacked_layer_bwd_f16 / _bf16,
``FastfoodStackedLayer16Function(..., fused_backward=True, fused_backward16=True, fused_epilogue_backward16=True)``): ``launch`` has
all three backward flags on, ``composed`` has ``fused_epilogue_backward16`` off (the 16-bit ``threshold_backward``, the float32 row
sum, ``F.pad``, ``relu(x)``, whvi_fused_shs_stacked_bwd_f16 / _bf16, ``threshold_backward``), 2 bytes an element; the bias-only
row is ``_hip.fused_shs_stacked_layer_bwd16`` against ``grad_y.sum(0, dtype=float32)`` and ``_hip.fused_shs_stacked_bwd16``.

    python tools/fastfood_stacked_layer_bwd_rate.py --dtype float16 bfloat16 --out profiles/r21/fastfood_stacked_layer_bwd16_rate.json

A 16-bit shape that ``FastfoodStackedLayer16Function.backward`` routes back to the composed backward (``_layer_bwd16_pays``: four
blocks with the bias sum, or D = 2048, on more than 256 blocks of cached bytes -- this measurement is why) is timed as the calls
themselves as well: ``_hip.fused_shs_stacked_layer_bwd16`` against the composed backward's passes called by hand.  ``--sweep``
(with ``--dtype``) times the shapes that decision rests on instead of the six: nine ``(D, J)`` at a 16 MiB activation, and
(128, 4) from 195 rows to 2^20.

Without ``--dtype`` the float32 measurement above runs, unchanged."""
import argparse
import json
import os
import statistics
import sys

import torch
import torch.nn.functional as F

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
from whvi_amd import _hip  # noqa: E402
from whvi_amd.fastfood import FastfoodStackedLayer16Function, FastfoodStackedLayerFunction, _layer_bwd16_pays  # noqa: E402

# (D, J, samples, batch, shared x, n_cols, relu_in, relu_out)
SHAPES = ((1024, 4, 16, 8192, False, 4096, True, True), (1024, 4, 16, 8192, False, 4096, False, False),
          (1024, 4, 16, 8192, True, 4096, True, True), (128, 4, 64, 1000, False, 512, True, True),
          (2048, 2, 16, 4096, False, 4096, True, True), (256, 4, 16, 8192, False, 800, True, True))
ROUTES = {"launch": True, "composed": False}                        # fused_epilogue_backward (16-bit: fused_epilogue_backward16)
DTYPES = {"float16": torch.float16, "bfloat16": torch.bfloat16}
# --sweep: (D, J) at rows * D = 2^23 (a 16 MiB 16-bit activation, 64 samples), then (128, 4) over sizes; bias and both ReLUs
SWEEP = tuple((d, J, 64, (1 << 23) // d // 64, False, J * d, True, True)
              for d, J in ((64, 4), (128, 4), (256, 4), (512, 4), (1024, 4), (128, 2), (128, 3), (512, 2), (1024, 3), (2048, 2))) + \
    tuple((128, 4, S, B, False, 512, True, True) for S, B in ((3, 65), (16, 256), (64, 250), (64, 4000), (16, 65536)))


def one_shape(d, J, S, batch, shared, n_cols, relu_in, relu_out, repeats, warmup, dtype=torch.float32):
    dev = torch.device("cuda", 0)
    rows = S * batch
    half = dtype != torch.float32
    size = 2.0 if half else 4.0                                    # bytes of an activation element
    family = "fused_layer_bwd16_kernel" if half else "fused_shs_stacked_layer_bwd_kernel"
    g = torch.Generator(device=dev).manual_seed(d + J)
    x = torch.randn(batch if shared else rows, d, device=dev, generator=g).to(dtype).requires_grad_(not shared)
    gy = torch.randn(rows, n_cols, device=dev, generator=g).to(dtype)
    a = torch.randn(J, d, device=dev, generator=g).mul_(0.01).requires_grad_()
    c = torch.randn(J, d, device=dev, generator=g).mul_(0.01).requires_grad_()
    b = torch.randn(J, S, d, device=dev, generator=g).requires_grad_()
    bias = torch.randn(1, J * d, device=dev, generator=g).mul_(0.01).requires_grad_()
    wanted = (a, b, c, bias) if shared else (x, a, b, c, bias)
    act = size * rows * d
    moved = size * rows * (n_cols * (2 if relu_out else 1) + (0 if shared else d) + (0 if shared else d))
    probe_src = torch.empty(int(moved) // 2, dtype=torch.uint8, device=dev).random_()
    probe_dst = torch.empty_like(probe_src)
    times = {name: [] for name in ROUTES}
    times["copy_probe"] = []
    kernels, peaks = {}, {}

    # a bias and nothing else to fold: the Function keeps that case composed (this measurement is why), so both routes are the
    # calls themselves -- the launch, and the row sum followed by the launch without an epilogue -- with no autograd around them
    direct = not (relu_in or relu_out or n_cols < J * d)
    if half and not _layer_bwd16_pays(d, J, S, batch, n_cols, relu_out, shared, not shared, True):
        direct = True                                               # (routed back by the Function: the calls themselves)
    y16 = None
    if half and direct and relu_out:
        y16 = _hip.fused_shs_stacked_layer16(x.detach(), a.detach(), b.detach(), c.detach(), S, batch, bias=bias.detach(),
                                             n_cols=n_cols, relu_in=relu_in, relu_out=True, shared=shared)

    def composed16(xd, ad, bd, cd):
        """FastfoodStackedLayer16Function's composed backward, pass by pass."""
        gm = (torch.ops.aten.threshold_backward(gy, y16, 0) if relu_out else gy).contiguous()
        gb = F.pad(gm.sum(dim=0, dtype=torch.float32), (0, J * d - n_cols))
        if n_cols < J * d:
            gm = F.pad(gm, (0, J * d - n_cols))
        xin = torch.relu(xd) if relu_in else xd
        out = _hip.fused_shs_stacked_bwd16(gm, xin, ad, bd, cd, S, batch, shared=shared, need_x=not shared)
        gx = torch.ops.aten.threshold_backward(out[0], xin, 0) if relu_in and out[0] is not None else out[0]
        return (gx,) + tuple(out[1:]) + (gb,)

    def run(name):
        if not direct:
            if half:
                y = FastfoodStackedLayer16Function.apply(x, a, b, c, bias, n_cols, relu_in, relu_out, S, batch, shared, True, True,
                                                         ROUTES[name])
            else:
                y = FastfoodStackedLayerFunction.apply(x, a, b, c, bias, n_cols, relu_in, relu_out, S, batch, shared, True,
                                                       ROUTES[name])
            return lambda: torch.autograd.grad(y, wanted, gy)
        xd, ad, bd, cd = (t.detach() for t in (x, a, b, c))
        if half and ROUTES[name]:
            return lambda: (_hip.fused_shs_stacked_layer_bwd16(gy, y16, xd, ad, bd, cd, S, batch, n_cols=n_cols, relu_in=relu_in,
                                                               relu_out=relu_out, shared=shared, need_x=not shared, need_bias=True),
                            kernels.__setitem__(name, _hip.last_kernel()))
        if half:
            return lambda: (composed16(xd, ad, bd, cd), kernels.__setitem__(name, _hip.last_kernel()))
        if ROUTES[name]:
            return lambda: (_hip.fused_shs_stacked_layer_bwd(gy, None, xd, ad, bd, cd, S, batch, shared=shared, need_x=not shared,
                                                             need_bias=True), kernels.__setitem__(name, _hip.last_kernel()))
        return lambda: (gy.sum(dim=0), _hip.fused_shs_stacked_bwd(gy, xd, ad, bd, cd, S, batch, shared=shared, need_x=not shared),
                        kernels.__setitem__(name, _hip.last_kernel()))

    def backward(name, timed):
        go = run(name)
        e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        if timed == "peak":
            torch.cuda.synchronize()
            torch.cuda.reset_peak_memory_stats(dev)
            held = torch.cuda.memory_allocated(dev)
        e0.record()
        grads = go()
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

    # the backward runs on autograd's thread and whvi_last_kernel is per thread: a hook on a leaf asks there
    for name in ROUTES:
        seen = []
        hook = a.register_hook(lambda grad: seen.append(_hip.last_kernel()))
        peaks[name] = backward(name, "peak")
        if not direct:
            kernels[name] = seen[-1]
        hook.remove()
    assert family in kernels["launch"] and family not in kernels["composed"]
    for name in ROUTES:
        for _ in range(warmup):
            backward(name, None)
    for _ in range(warmup):
        probe()
    for _ in range(repeats):
        for name in ROUTES:                                         # alternating: one measurement of each route per repeat
            times[name].append(backward(name, "time"))
        times["copy_probe"].append(probe())
    out = {**({"dtype": str(dtype).replace("torch.", "")} if half else {}), "D": d, "n_blocks": J, "n_samples": S, "batch": batch, "rows": rows, "x_shared": shared, "x_wants_gradient": not shared,
           "n_cols": n_cols, "bias": True, "timed_through": "the calls" if direct else "the Function's backward", "relu_in": relu_in, "relu_out": relu_out, "activation_bytes": act,
           "launch_bytes": moved, "kernels": kernels,
           "workspace_bytes": int(_hip.lib().whvi_fused_shs_stacked_layer_bwd_workspace(S, batch, d.bit_length() - 1, J, 1)),
           "routes": {}}
    for name, ts in times.items():
        med = statistics.median(ts)
        out["routes"][name] = {"ms_median": med, "ms_min": min(ts), "ms_max": max(ts), "ms": ts}
        if name in peaks:
            out["routes"][name].update(peak_bytes_above_held=peaks[name], peak_activations=peaks[name] / act)
    for name in ("launch", "copy_probe"):
        r = out["routes"][name]
        r["TBps_median"], r["TBps_min"], r["TBps_max"] = (moved / t / 1e9 for t in (r["ms_median"], r["ms_max"], r["ms_min"]))
    f, co = out["routes"]["launch"], out["routes"]["composed"]
    out["speedup_over_composed"] = co["ms_median"] / f["ms_median"]
    out["passes_removed_ms"] = co["ms_median"] - f["ms_median"]
    out["launch_max_below_composed_min"] = f["ms_max"] < co["ms_min"]
    print(f"{str(dtype).replace('torch.', '') + ' ' if half else ''}D={d:5d} J={J} S={S:3d} B={batch:6d} shared={int(shared)} n_cols={n_cols} relu={int(relu_in)}{int(relu_out)}: launch "
          f"{f['ms_median']:.3f} ms [{f['ms_min']:.3f}-{f['ms_max']:.3f}], peak {f['peak_activations']:.2f} A, {f['TBps_median']:.2f} TB/s; "
          f"composed {co['ms_median']:.3f} ms [{co['ms_min']:.3f}-{co['ms_max']:.3f}], peak {co['peak_activations']:.2f} A; copy probe "
          f"{out['routes']['copy_probe']['ms_median']:.3f} ms; speedup {out['speedup_over_composed']:.2f}; slowest launch below "
          f"fastest composed: {out['launch_max_below_composed_min']}", flush=True)
    print(f"    kernels: {kernels}", flush=True)
    return out


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--repeats", type=int, default=9)
    ap.add_argument("--warmup", type=int, default=30)
    ap.add_argument("--out", default=None)
    ap.add_argument("--sweep", action="store_true", help="with --dtype: the shapes the routing condition rests on instead of the six")
    ap.add_argument("--dtype", nargs="+", choices=sorted(DTYPES), default=None,
                    help="time the 16-bit entries on these activation types instead of the float32 entry")
    args = ap.parse_args()
    assert args.repeats >= 9, "at least 9 alternating repeats"
    assert args.dtype is not None or not args.sweep, "--sweep times the 16-bit entries: give --dtype"
    if args.dtype is None:
        results = [one_shape(*shape, args.repeats, args.warmup) for shape in SHAPES]
    else:
        results = [one_shape(*shape, args.repeats, args.warmup, DTYPES[name]) for shape in (SWEEP if args.sweep else SHAPES)
                   for name in args.dtype]
    doc = {"tool": "tools/fastfood_stacked_layer_bwd_rate.py", "argv": sys.argv[1:], "device": torch.cuda.get_device_name(0),
           "repeats": args.repeats, "warmup": args.warmup, "results": results}
    if args.out:
        os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
        with open(args.out, "w") as f:
            json.dump(doc, f, indent=1)
    return 0


if __name__ == "__main__":
    sys.exit(main())
