"""tests/golden/make_golden_toy_sigmoid.py -- fixture of the toy notebook's own WHVI model from the LIVE reference (build
container only).

    python oracle/build_ref.py && python tests/golden/make_golden_toy_sigmoid.py

Same rules as make_golden.py / make_golden_r4.py (whose import set-up it reuses): the reference's Python package is imported
from where it lies (/root/reference), ``fwht_cpp`` is the reference's own compiled C++ FWHT (oracle/_ref), runs on the CPU,
and only DATA is written.

toy_sigmoid_golden.npz -- the second WHVI model of experiments/Toy example.ipynb,

    torch.manual_seed(1)
    WHVIRegression([WHVILinear(1, 128, lambda_=1.0), nn.Sigmoid(), WHVILinear(128, 128, lambda_=2.5), nn.Sigmoid(),
                    WHVILinear(128, 1, lambda_=5.0)], sigma=0.1)

on the notebook's data (np.random.seed(0); 128 points on [-1, 2) minus (0.6, 1.4); the notebook's polynomial plus
N(0, exp(-3)) noise), full batch, one training sample:
  init_params / param_names   the parameters as constructed (flat, named_parameters order)
  eps                         every draw of the recorded passes in draw order, (n, 128): per pass and sample, the first,
                              square and output layer
  loss / mnll / kl / grads    the first step's ELBO, its two terms and every parameter gradient (flat)
  losses / final_params       STEPS steps of the notebook's recipe: Adam(lr = 1e-3) under LambdaLR((1 + 0.0005 t)^-0.3),
                              loss, backward, step, scheduler step, zero_grad -- the loss of every step, the parameters after
  x_test / pred               eval-mode predictions, EVAL_SAMPLES samples, of the notebook's test grid (every 25th point of
                              linspace(-2, 3, 1000)) with the trained parameters, (40, 1, EVAL_SAMPLES)"""
import os
import sys

sys.dont_write_bytecode = True      # importing the reference must not leave __pycache__ files in its checkout

import numpy as np

HERE = os.path.dirname(os.path.abspath(__file__))
ROOT = os.path.dirname(os.path.dirname(HERE))
REFERENCE = "/root/reference"
STEPS, EVAL_SAMPLES = 20, 8


def notebook_data():
    """The notebook's training set (cells 1 and 3): x (n, 1), y (n, 1) float32, and its test function."""
    np.random.seed(0)
    xs_poly = [-2.0, -1.5, -0.8, 0.0, 0.5, 1.4, 2.0, 2.7, 3.0]
    ys_poly = [1.2, 1.5, 2.0, 0.5, -0.5, 1.2, 0.0, 1.0, 1.3]
    coef = np.linalg.solve(np.vander(xs_poly, len(xs_poly)), ys_poly)
    x = np.random.rand(128) * 3 - 1
    x = x[np.where((x < 0.6) | (x > 1.4))]
    y = np.polyval(coef, x) + np.random.randn(len(x)) * np.sqrt(np.exp(-3))
    return x.reshape(-1, 1).astype(np.float32), y.reshape(-1, 1).astype(np.float32)


def main():
    ref_so_dir = os.path.join(ROOT, "oracle", "_ref")
    if not os.path.isdir(REFERENCE) or not os.path.isdir(ref_so_dir):
        sys.exit("needs the reference tree and oracle/_ref (python oracle/build_ref.py)")
    sys.path[:0] = [ref_so_dir, REFERENCE, ROOT]

    import torch
    import torch.nn as nn
    import fwht_cpp
    assert os.path.dirname(fwht_cpp.__file__) == ref_so_dir, fwht_cpp.__file__
    sys.path.insert(0, HERE)
    from make_golden import bind_reference_src
    bind_reference_src(REFERENCE)
    from src.layers import WHVILinear
    from src.networks import WHVIRegression

    torch.set_num_threads(1)
    x_np, y_np = notebook_data()
    x, y = torch.from_numpy(x_np), torch.from_numpy(y_np)
    torch.manual_seed(1)
    net = WHVIRegression([WHVILinear(1, 128, lambda_=1.0), nn.Sigmoid(), WHVILinear(128, 128, lambda_=2.5), nn.Sigmoid(),
                          WHVILinear(128, 1, lambda_=5.0)], sigma=0.1)
    out = {"x": x_np, "y": y_np,
           "param_names": np.array("\n".join(n for n, _ in net.named_parameters())),
           "init_params": np.concatenate([p.detach().numpy().reshape(-1) for p in net.parameters()])}

    real_randn = torch.randn
    recorded = []

    def recording_randn(*a, **k):
        t = real_randn(*a, **k)
        recorded.append(t.detach().clone())
        return t

    optimizer = torch.optim.Adam(net.parameters(), lr=1e-3)
    scheduler = torch.optim.lr_scheduler.LambdaLR(optimizer, lambda t: (1 + 0.0005 * t) ** (-0.3))
    net.train()
    losses = []
    torch.randn = recording_randn
    try:
        for step in range(STEPS):
            loss = net.loss(x, y, n=len(x))
            loss.backward()
            if step == 0:
                out["loss"] = loss.detach().numpy()
                out["mnll"] = net.current_mnll.detach().numpy()
                out["kl"] = net.current_kl.detach().numpy()
                out["grads"] = np.concatenate([p.grad.numpy().reshape(-1) for p in net.parameters()])
            losses.append(float(loss.detach()))
            optimizer.step()
            scheduler.step()
            net.zero_grad(set_to_none=True)
        out["final_params"] = np.concatenate([p.detach().numpy().reshape(-1) for p in net.parameters()])
        x_test = torch.linspace(-2, 3, 1000).reshape(-1, 1)[::25].contiguous()
        net.eval_samples = EVAL_SAMPLES
        net.eval()
        with torch.no_grad():
            pred = net(x_test)
    finally:
        torch.randn = real_randn
    assert len(recorded) == 3 * (STEPS + EVAL_SAMPLES) and all(tuple(e.shape) == (128,) for e in recorded)
    out["losses"] = np.array(losses, dtype=np.float32)
    out["eps"] = np.stack([e.numpy() for e in recorded])
    out["x_test"], out["pred"] = x_test.numpy(), pred.numpy()
    path = os.path.join(HERE, "toy_sigmoid_golden.npz")
    np.savez_compressed(path, **out)
    print("toy_sigmoid_golden.npz: rows", len(x_np), "loss", float(out["loss"]), "last loss", losses[-1], "pred",
          tuple(pred.shape), "bytes", os.path.getsize(path))


if __name__ == "__main__":
    main()
