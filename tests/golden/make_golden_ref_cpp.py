"""tests/golden/make_golden_ref_cpp.py -- ref_cpp_golden.npz: the reference's own compiled C++ FWHT (oracle/_ref, built by
oracle/build_ref.py) on the inputs of tests/test_oracle.py's two comparisons with it, so those tests run on any checkout.

    python tests/golden/make_golden_ref_cpp.py

Only DATA is written: each input and the reference's output for it.
  rand_<kind>_<rows>x<d>_{in,out}  kind = f32 / i32: torch.Generator seed 3, the shapes of test_bit_equal_to_compiled_reference
  wrap_<kind>_{in,out}             kind = i32 / i64: the overflowing rows of test_integer_overflow_wraps_like_the_reference"""
import os
import sys

import numpy as np

HERE = os.path.dirname(os.path.abspath(__file__))
ROOT = os.path.dirname(os.path.dirname(HERE))
SHAPES = ((19, 1024), (3, 4096), (7, 1), (5, 2), (40, 32))


def wrap_inputs():
    """Rows near +/-2^30 (int32) resp. +/-2^62 (int64), D = 4096: twelve doublings overflow both types."""
    rng = np.random.default_rng(2 ** 30)
    d, rows = 4096, 6
    mag = rng.integers((1 << 30) - 4096, (1 << 30) + 4096, (rows, d))
    x32 = (mag * rng.choice([-1, 1], (rows, d))).astype(np.int32)
    x64 = ((mag.astype(np.int64) << 32) * rng.choice([-1, 1], (rows, d))).astype(np.int64)
    return x32, x64


def main():
    sys.path.insert(0, ROOT)
    import torch
    import oracle
    ref = oracle.load_reference_cpp()
    if ref is None:
        sys.exit("needs oracle/_ref (python oracle/build_ref.py)")
    out = {}
    g = torch.Generator().manual_seed(3)
    for rows, d in SHAPES:
        for kind, x in (("f32", torch.randn(rows, d, generator=g)),
                        ("i32", torch.randint(-8, 8, (rows, d), generator=g, dtype=torch.int32))):
            out[f"rand_{kind}_{rows}x{d}_in"] = x.numpy()
            out[f"rand_{kind}_{rows}x{d}_out"] = ref.forward(x).numpy()
    for kind, x in zip(("i32", "i64"), wrap_inputs()):
        out[f"wrap_{kind}_in"] = x
        out[f"wrap_{kind}_out"] = ref.forward(torch.from_numpy(x)).numpy()
    np.savez_compressed(os.path.join(HERE, "ref_cpp_golden.npz"), **out)


if __name__ == "__main__":
    main()
