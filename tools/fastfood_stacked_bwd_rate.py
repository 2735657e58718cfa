#!/usr/bin/env python3
"""tools/fastfood_stacked_bwd_rate.py -- what the one-launch backward of the rectangular fastfood layer
(whvi_fused_shs_stacked_bwd_f32, ``FastfoodStackedFunction(..., fused_backward=True)``) buys over the per-block loop it replaces.
One process, inputs resident, HIP events on the launch stream around the whole backward of ``FastfoodStackedFunction`` (its
forward runs outside the timed region), a warm-up of 30 backward passes per route (clocks ramp), then the routes ALTERNATE over
the repeats; median and min-max per route.  The yardstick is the per-block route of the same run.

    python tools/fastfood_stacked_bwd_rate.py --out profiles/r15/fastfood_stacked_bwd_rate.json
    python tools/fastfood_stacked_bwd_rate.py --dtype float16 --dtype bfloat16 --all-pairs --out profiles/r19/fastfood_stacked_bwd16_rate.json

Routes: ``launch`` (the flag on); ``per_block_fused`` (the flag on with ``_hip.fused_shs_stacked_bwd_supported`` answering no: the
loop over the blocks, each block one launch of whvi_fused_shs_bwd_f32 -- the route every shape took before the launch existed
and the fallback still takes); ``per_block_chain`` (the flag off); ``copy_probe``: ``whvi_stream_copy_probe`` moving the same
(2 + J) * D * 4 bytes per row (half read, half written) with no arithmetic.  Per route also the allocator's peak above what is
held before the backward.  ``TBps`` of the launch is (2 + J) activations -- x and the J segments of grad_y read, grad_x written
-- over the median time of the whole backward (both launches and the allocations).

Shapes (D, J, samples, batch, shared x): (1024, 4, 16, 8192) with an input of its own and with a shared one; (128, 4, 64, 1000);
(2048, 2, 16, 4096); one small shape (1024, 4, 1, 256), where a launch cannot fill the chip.  All of x, a, b, c want a gradient,
except at the shared shape: a shared x that wants a gradient keeps the loop on every route (FastfoodStackedFunction), so there
x is data -- a network's first layer -- and a, b, c want theirs.

``--dtype float16 | bfloat16`` (repeatable; tools/fused_bwd_rate.py is the model): the same shapes on 16-bit activations with
float32 a, b, c -- whvi_fused_shs_stacked_bwd_f16 / _bf16, DESIGN 5.2k.  ``launch``: ``keep_half``, ``fused_backward`` and
``fused_backward16``; ``per_block_fused``: the same flags with ``_hip.fused_shs_stacked_bwd16_supported`` answering no -- the loop
of whvi_fused_shs_bwd_f16 / _bf16 launches, the route before the launch existed; ``per_block_chain``: ``keep_half`` alone;
``copy_probe``: (2 + J) * D * 2 bytes per row.  ``--all-pairs`` adds one shape per shipped (D, J), 16 samples of 2^23 / D rows
with an input of its own, so that every pair of the support rule has its own verdict: a pair stays in the Python rule if the
launch's median is below the per-block route's in the same run."""
import argparse
import json
import os
import statistics
import sys

import torch

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
from whvi_amd import _hip  # noqa: E402
from whvi_amd.fastfood import FastfoodStackedFunction  # noqa: E402

SHAPES = ((1024, 4, 16, 8192, False), (1024, 4, 16, 8192, True), (128, 4, 64, 1000, False), (2048, 2, 16, 4096, False),
          (1024, 4, 1, 256, False))
# route -> ((keep_half, fused_backward, fused_backward16), launch allowed)
ROUTES32 = {"launch": ((False, True, False), True), "per_block_fused": ((False, True, False), False),
            "per_block_chain": ((False, False, False), False)}
ROUTES16 = {"launch": ((True, True, True), True), "per_block_fused": ((True, True, True), False),
            "per_block_chain": ((True, False, False), False)}
ALL_PAIRS = tuple((1 << L, J, 16, (1 << 23) >> L, False) for L in range(6, 11) for J in (2, 3, 4)) + ((2048, 2, 16, 4096, False),)
DTYPES = {"float32": torch.float32, "float16": torch.float16, "bfloat16": torch.bfloat16}


def one_shape(d, J, S, batch, shared, repeats, warmup, dtype=torch.float32):
    dev = torch.device("cuda", 0)
    rows = S * batch
    half = dtype != torch.float32
    esize = 2 if half else 4
    ROUTES = ROUTES16 if half else ROUTES32
    query = "fused_shs_stacked_bwd16_supported" if half else "fused_shs_stacked_bwd_supported"
    _SUPPORTED = getattr(_hip, query)
    g = torch.Generator(device=dev).manual_seed(d + J)
    x = torch.randn(batch if shared else rows, d, device=dev, generator=g).to(dtype).requires_grad_(not shared)
    gy = torch.randn(rows, J * d, device=dev, generator=g).to(dtype)
    a = torch.randn(J, d, device=dev, generator=g).mul_(0.01).requires_grad_()
    c = torch.randn(J, d, device=dev, generator=g).mul_(0.01).requires_grad_()
    b = torch.randn(J, S, d, device=dev, generator=g).requires_grad_()
    wanted = (a, b, c) if shared else (x, a, b, c)
    act = float(esize) * rows * d
    probe_src = torch.empty((2 + J) * rows * d * esize // 2, dtype=torch.uint8, device=dev).random_()
    probe_dst = torch.empty_like(probe_src)
    times = {name: [] for name in ROUTES}
    times["copy_probe"] = []
    kernels, peaks = {}, {}

    def backward(name, timed):
        flags, allowed = ROUTES[name]
        setattr(_hip, query, _SUPPORTED if allowed else (lambda *args: False))
        try:
            y = FastfoodStackedFunction.apply(x, a, b, c, S, batch, shared, *flags)
            e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
            if timed == "peak":
                torch.cuda.synchronize()
                torch.cuda.reset_peak_memory_stats(dev)
                held = torch.cuda.memory_allocated(dev)
            e0.record()
            grads = torch.autograd.grad(y, wanted, gy)
            e1.record()
            e1.synchronize()
        finally:
            setattr(_hip, query, _SUPPORTED)
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
        kernels[name] = seen[-1]
        hook.remove()
    for name in ROUTES:
        for _ in range(warmup):
            backward(name, None)
    for _ in range(warmup):
        probe()
    for _ in range(repeats):
        for name in ROUTES:                                         # alternating: one measurement of each route per repeat
            times[name].append(backward(name, "time"))
        times["copy_probe"].append(probe())
    out = {"dtype": str(dtype).replace("torch.", ""), "D": d, "n_blocks": J, "n_samples": S, "batch": batch, "rows": rows, "x_shared": shared, "x_wants_gradient": not shared,
           "activation_bytes": act, "kernels": kernels,
           "workspace_bytes": int(_hip.lib().whvi_fused_shs_stacked_bwd_workspace(S, batch, d.bit_length() - 1, J)), "routes": {}}
    for name, ts in times.items():
        med = statistics.median(ts)
        out["routes"][name] = {"ms_median": med, "ms_min": min(ts), "ms_max": max(ts), "ms": ts}
        if name in peaks:
            out["routes"][name].update(peak_bytes_above_held=peaks[name], peak_activations=peaks[name] / act)
    for name in ("launch", "copy_probe"):                           # (2 + J) activations: x, the J segments of grad_y, grad_x
        r = out["routes"][name]
        r["TBps_median"], r["TBps_min"], r["TBps_max"] = ((2 + J) * act / t / 1e9 for t in (r["ms_median"], r["ms_max"], r["ms_min"]))
    f, pb, ch = (out["routes"][n] for n in ("launch", "per_block_fused", "per_block_chain"))
    out["speedup_over_per_block_fused"] = pb["ms_median"] / f["ms_median"]
    out["speedup_over_per_block_chain"] = ch["ms_median"] / f["ms_median"]
    out["launch_max_below_per_block_fused_min"] = f["ms_max"] < pb["ms_min"]
    print(f"{out['dtype']} D={d:5d} J={J} S={S:3d} B={batch:6d} shared={int(shared)}: launch {f['ms_median']:.3f} ms [{f['ms_min']:.3f}-{f['ms_max']:.3f}], "
          f"peak {f['peak_activations']:.2f} A, {f['TBps_median']:.2f} TB/s at {esize * (2 + J)} D bytes per row; per-block fused "
          f"{pb['ms_median']:.3f} ms [{pb['ms_min']:.3f}-{pb['ms_max']:.3f}], peak {pb['peak_activations']:.2f} A; per-block chain "
          f"{ch['ms_median']:.3f} ms [{ch['ms_min']:.3f}-{ch['ms_max']:.3f}], peak {ch['peak_activations']:.2f} A; copy probe "
          f"{out['routes']['copy_probe']['ms_median']:.3f} ms; speedup {out['speedup_over_per_block_fused']:.2f} / "
          f"{out['speedup_over_per_block_chain']:.2f}; slowest launch below fastest per-block fused: "
          f"{out['launch_max_below_per_block_fused_min']}", flush=True)
    print(f"    kernels: {kernels}", flush=True)
    return out


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--repeats", type=int, default=9)
    ap.add_argument("--warmup", type=int, default=30)
    ap.add_argument("--dtype", action="append", choices=sorted(DTYPES), default=None, help="repeatable; default float32")
    ap.add_argument("--all-pairs", action="store_true", help="also one shape per shipped (D, J)")
    ap.add_argument("--out", default=None)
    args = ap.parse_args()
    assert args.repeats >= 9, "at least 9 alternating repeats"
    shapes = SHAPES + (ALL_PAIRS if args.all_pairs else ())
    results = [one_shape(*shape, args.repeats, args.warmup, DTYPES[name]) for name in (args.dtype or ["float32"]) for shape in shapes]
    doc = {"tool": "tools/fastfood_stacked_bwd_rate.py", "argv": sys.argv[1:], "device": torch.cuda.get_device_name(0),
           "repeats": args.repeats, "warmup": args.warmup, "results": results}
    if args.out:
        os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
        with open(args.out, "w") as f:
            json.dump(doc, f, indent=1)
    return 0


if __name__ == "__main__":
    sys.exit(main())
