"""The host references of the training-step kernels (tools/train_aux_ref.py), without a GPU.

tests/test_train_aux_gpu.py holds whvi_reparam_kl_f32, whvi_reparam_kl_philox_f32, whvi_reparam_kl_bwd_f32, whvi_gauss_mnll_f32
and whvi_gauss_mnll_bwd_f32 to these references, element by element.  Here the references themselves are checked, and the bounds:

  * Philox4x32-10 against Random123's three known-answer vectors; the uniform map over all 2^24 inputs (minimum 2^-25, maximum
    1.0, reached once); no counter used twice inside a launch, none shared by two launches on one state.
  * Each float64 closed form against torch float64 autograd on the CPU over the reference's own op chain (softplus, cat,
    kl_diag_normal; torch.distributions.Normal.log_prob), 1e-12 relative.
  * ATTAINABLE: a float32 numpy emulation of each kernel's operation order stays inside the GPU test's bound on the GPU test's
    own case list.  The worst error-to-bound ratios are printed (``-s``).
  * DISCRIMINATING: the same emulation with one thing wrong leaves the bound on at least one case of that list --
      (a) log(1 + exp(rho)) for log1p(exp(rho)),            (b) the backward's sample loop one sample short,
      (d) grad_sigma without ``- count``,                   (e) Philox counter words i and (j << 16 | z) exchanged,
      (f) eight samples drawn as eight calls instead of two calls of four.
    (c) -- sigmoid(rho) applied above softplus' threshold of 20 as well -- CANNOT be separated from float32 rounding, at
    rho just above 20 or at 25: 1 - sigmoid(rho) <= 2.1e-9 there, far below half an ulp of 1 (6e-8), so 1 / (1 + expf(-rho)) IS
    1.0f and the mutated kernel returns the same bits.  test_sigmoid_above_the_threshold_is_the_same_float32 states exactly
    that; in float64 the two forms differ by 2.1e-9 relative, a thousandth of the bound.  The backward's threshold branch is
    therefore a saving of one expf, not something a float32 test can pin, and no separable case exists to keep.
The mutations stand in for mutating the shipped kernels on a GPU, which this suite does not do."""
import os
import sys

import numpy as np
import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(ROOT, "tools"))
import train_aux_ref as ta  # noqa: E402

B = ta.BOUNDS


# ---- Philox ---------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("counter,key,want", ta.KNOWN_ANSWERS, ids=("zeros", "ones", "pi"))
def test_philox_known_answers(counter, key, want):
    got = ta.philox4x32_10(*counter, *key)
    assert tuple(int(w) for w in got) == want


def test_philox_is_vectorised_over_counters_and_keys():
    counters = np.array([c for c, _, _ in ta.KNOWN_ANSWERS], dtype=np.uint32).T
    keys = np.array([k for _, k, _ in ta.KNOWN_ANSWERS], dtype=np.uint32).T
    got = np.stack(ta.philox4x32_10(*counters, *keys), axis=1)
    assert np.array_equal(got, np.array([w for _, _, w in ta.KNOWN_ANSWERS], dtype=np.uint32))


def test_uniform_map_over_all_24_bit_inputs():
    top = np.arange(1 << 24, dtype=np.uint32)
    u = ta.uniform24(top << np.uint32(8))
    assert u.dtype == np.float32
    assert float(u.min()) == 2.0 ** -25 and int(u.argmin()) == 0
    assert float(u.max()) == 1.0 and int((u == 1.0).sum()) == 1 and int(u.argmax()) == (1 << 24) - 1
    assert np.array_equal(u, ta.uniform24((top << np.uint32(8)) | np.uint32(0xFF)))          # the low eight bits do not count
    assert bool((np.diff(u) >= 0).all())


def test_no_counter_is_used_twice():
    J, S, D = 2, 17, 300
    for offset in (0, 2 ** 32 - 1):
        lo, hi = ta.counter_set(offset, J, S, D)
        calls = J * ((S + 7) // 8) * ta.CALLS_PER_BLOCK * D
        assert lo.size == hi.size == calls
        assert len(set(zip(lo.tolist(), hi.tolist()))) == calls
        lo2, hi2 = ta.counter_set(offset + ta.CALLS_PER_BLOCK, J, S, D)                       # the next launch on the same state
        assert not set(zip(lo.tolist(), hi.tolist())) & set(zip(lo2.tolist(), hi2.tolist()))


def test_eps_reference_layout_and_moments():
    J, S, D = 3, 21, 1000
    eps, rad = ta.eps_reference(1234, 0, J, S, D)
    assert eps.shape == rad.shape == (J, S, D) and eps.dtype == np.float64
    assert bool((np.abs(eps) <= rad).all()) and float(rad.max()) <= np.sqrt(2 * 25 * np.log(2.0)) + 1e-12
    assert abs(float(eps.mean())) < 4 / np.sqrt(eps.size) and abs(float(eps.var()) - 1.0) < 4 * np.sqrt(2 / eps.size)
    assert np.unique(eps).size == eps.size
    # one element, by hand: matrix 2, sample 13 (block 1, q = 5: call 1, its second normal), column 999, offset carrying into word 3
    off = 2 ** 32 - 1
    one = ta.eps_reference(0x123456789ABCDEF0, off, J, S, D)[0][2, 13, 999]
    x = ta.philox4x32_10(999, (2 << 16) | 1, (off + 1) & 0xFFFFFFFF, (off + 1) >> 32, 0x9ABCDEF0, 0x12345678)
    u1, u2 = ta.uniform24(x[0]), ta.uniform24(x[1])
    want = np.sqrt(-2.0 * np.log(np.float64(u1))) * np.sin(np.float64(np.float32(np.float32(6.283185307179586) * u2)))
    assert abs(one - want) <= 4e-16 * abs(want)
    # a shorter launch is a prefix in every axis
    assert np.array_equal(ta.eps_reference(1234, 0, 2, 9, 257)[0], eps[:2, :9, :257])


# ---- closed forms against torch float64 autograd over the reference's op chain -----------------------------------------------------
def _close(got, want, rel=1e-12):
    got, want = np.asarray(got, dtype=np.float64), np.asarray(want, dtype=np.float64)
    assert got.shape == want.shape
    assert bool((np.abs(got - want) <= rel * np.abs(want)).all()), float((np.abs(got - want) / np.abs(want)).max())


@pytest.mark.parametrize("case", [c for c in ta.BWD_CASES if c["D"] in (1, 257)], ids=lambda c: c["id"])
def test_reparam_closed_forms_vs_torch_float64(case):
    import torch
    import torch.nn.functional as F
    from whvi_amd.utils import kl_diag_normal
    inp = ta.reparam_inputs(case)
    J, D = case["J"], case["D"]
    lam = float(np.float32(case["lam"]))
    mu = torch.from_numpy(inp["mu"]).double().requires_grad_()
    rho = torch.from_numpy(inp["rho"]).double().requires_grad_()
    eps = torch.from_numpy(inp["eps"]).double()
    sigma = F.softplus(rho)
    u = torch.cat((mu.unsqueeze(1), sigma.unsqueeze(1) * eps), dim=1)
    kl = torch.stack([kl_diag_normal(mu[j], sigma[j], torch.zeros(D, dtype=torch.float64),
                                     torch.full((D,), lam, dtype=torch.float64)) for j in range(J)])
    ref = ta.reparam_kl_reference(inp["mu"], inp["rho"], inp["eps"], case["lam"])
    _close(ref.sigma, sigma.detach().numpy())
    _close(ref.u, u.detach().numpy())
    _close(ref.kl, kl.detach().numpy())
    assert bool((ref.Y_kl >= np.abs(ref.kl)).all())
    gu = torch.zeros_like(u) if inp["gu"] is None else torch.from_numpy(inp["gu"]).double()
    gk = torch.zeros_like(kl) if inp["gk"] is None else torch.from_numpy(inp["gk"]).double()
    want_mu, want_rho = torch.autograd.grad((u, kl), (mu, rho), (gu, gk))
    bwd = ta.reparam_kl_bwd_reference(inp["gu"], inp["gk"], inp["mu"], inp["rho"], inp["eps"], case["lam"])
    # autograd adds the terms the closed form adds, in another order: relative to the yardstick, not to a cancelled sum
    assert bool((np.abs(bwd.grad_mu - want_mu.numpy()) <= 1e-12 * bwd.Y_mu).all())
    assert bool((np.abs(bwd.grad_rho - want_rho.numpy()) <= 1e-12 * bwd.Y_rho).all())
    assert bool((bwd.Y_mu >= np.abs(bwd.grad_mu)).all()) and bool((bwd.Y_rho >= np.abs(bwd.grad_rho) * (1 - 1e-15)).all())


@pytest.mark.parametrize("case", [c for c in ta.MNLL_CASES if c["m"] <= 100], ids=lambda c: c["id"])
def test_mnll_closed_form_vs_torch_float64(case):
    import torch
    inp = ta.mnll_inputs(case)
    m, n_out, n_mc = case["m"], case["n_out"], case["n_mc"]
    yh = torch.from_numpy(inp["dense"]).double().requires_grad_()
    sg = torch.tensor(float(np.float32(inp["sigma"])), dtype=torch.float64, requires_grad=True)
    y = torch.from_numpy(inp["y"]).double()
    total = 0.0
    for o in range(n_out):                                      # the reference's loop over outputs (src/likelihoods.py:18-29)
        total = total + torch.distributions.Normal(yh[:, o, :], sg).log_prob(y[:, o].reshape(m, 1)).sum()
    loss = float(np.float32(inp["scale"])) * total
    g = float(np.float32(inp["g"]))
    w_yh, w_sg = torch.autograd.grad(loss, (yh, sg), torch.tensor(g, dtype=torch.float64))
    y3 = np.broadcast_to(inp["y"][:, :, None], (m, n_out, n_mc))
    ref = ta.gauss_mnll_reference(y3, inp["dense"], inp["sigma"], inp["scale"], inp["g"])
    assert abs(ref.loss - loss.item()) <= 1e-12 * ref.Y_loss and ref.Y_loss >= abs(ref.loss)
    assert bool((np.abs(ref.grad_yhat - w_yh.numpy()) <= 1e-12 * ref.Y_yhat).all())
    assert abs(ref.grad_sigma - float(w_sg)) <= 1e-12 * ref.Y_sigma and ref.Y_sigma >= abs(ref.grad_sigma)
    # the view of the buffer is the dense array, and the kernel's walk of it is the buffer's memory order
    assert np.array_equal(inp["view"](inp["base"]), inp["dense"])
    if case["layout"] != "gaps":
        assert np.array_equal(inp["walk"](inp["dense"]).ravel(), inp["base"].ravel())


# ---- the bounds: attainable and discriminating ------------------------------------------------------------------------------------
def _forward_ratios(case, mutate=None):
    inp = ta.reparam_inputs(case)
    ref = ta.reparam_kl_reference(inp["mu"], inp["rho"], inp["eps"], case["lam"])
    sigma, u, kl = ta.emulate_reparam_kl(inp["mu"], inp["rho"], inp["eps"], case["lam"], mutate)
    above = inp["rho"] > np.float32(ta.SOFTPLUS_THRESHOLD)
    assert np.array_equal(sigma[above], inp["rho"][above]) and np.array_equal(u[:, 0], inp["mu"])
    assert np.array_equal(u[:, 1:], sigma[:, None, :] * inp["eps"])
    return {"sigma": ta.worst_ratio(sigma, ref.sigma, ref.sigma, B["sigma"]), "kl": ta.worst_ratio(kl, ref.kl, ref.Y_kl, B["kl"])}


def _backward_ratios(case, mutate=None):
    inp = ta.reparam_inputs(case)
    sigma = ta.emulate_reparam_kl(inp["mu"], inp["rho"], inp["eps"], case["lam"])[0]
    ref = ta.reparam_kl_bwd_reference(inp["gu"], inp["gk"], inp["mu"], inp["rho"], inp["eps"], case["lam"])
    gmu, grho = ta.emulate_reparam_kl_bwd(inp["gu"], inp["gk"], inp["mu"], inp["rho"], inp["eps"], sigma, case["lam"], mutate)
    return {"grad_mu": ta.worst_ratio(gmu, ref.grad_mu, ref.Y_mu, B["grad_mu"]),
            "grad_rho": ta.worst_ratio(grho, ref.grad_rho, ref.Y_rho, B["grad_rho"])}


def _mnll_ratios(case, mutate=None):
    inp = ta.mnll_inputs(case)
    shape = (case["m"], case["n_out"], case["n_mc"])
    y3 = np.broadcast_to(inp["y"][:, :, None], shape)
    ref = ta.gauss_mnll_reference(y3, inp["dense"], inp["sigma"], inp["scale"], inp["g"])
    walk = inp["walk"]
    loss, g_yh, g_sg = ta.emulate_gauss_mnll(walk(y3), walk(inp["dense"]), inp["sigma"], inp["scale"], inp["g"], mutate)
    return {"loss": ta.worst_ratio(loss, ref.loss, ref.Y_loss, B["loss"]),
            "grad_yhat": ta.worst_ratio(g_yh, walk(ref.grad_yhat).ravel(), walk(ref.Y_yhat).ravel(), B["grad_yhat"]),
            "grad_sigma": ta.worst_ratio(g_sg, ref.grad_sigma, ref.Y_sigma, B["grad_sigma"])}


def _worst(fn, cases, mutate=None):
    worst = {}
    for case in cases:
        for name, ratio in fn(case, mutate).items():
            if ratio > worst.get(name, (-1.0, ""))[0]:
                worst[name] = (ratio, case["id"])
    return worst


@pytest.mark.parametrize("fn,cases", [(_forward_ratios, ta.FWD_CASES), (_backward_ratios, ta.BWD_CASES),
                                      (_mnll_ratios, ta.MNLL_CASES)], ids=("reparam_kl", "reparam_kl_bwd", "gauss_mnll"))
def test_bounds_are_attainable(fn, cases):
    worst = _worst(fn, cases)
    for name, (ratio, where) in worst.items():
        print(f"emulation, worst |error| / bound of {name}: {ratio:.3f} at {where}")
    assert all(ratio <= 1.0 for ratio, _ in worst.values()), worst


def test_box_muller_in_float32_stays_inside_the_eps_bound():
    """numpy's float32 logarithm, square root, cosine and sine on the reference's uniforms and angle."""
    worst = 0.0
    for case in ta.PHILOX_CASES:
        J, S, D = case["J"], case["S"], case["D"]
        ref = ta.eps_reference(case["seed"], case["offset"], J, S, D)[0]
        got = _eps_float32(case["seed"], case["offset"], J, S, D)
        worst = max(worst, ta.worst_ratio(got, ref, np.abs(ref), B["eps"], ta.EPS_FLOOR))
    print(f"emulation, worst |error| / bound of eps: {worst:.3f}")
    assert worst <= 1.0


def _eps_float32(seed, offset, J, S, D):
    c = ta.counters(offset, J, S, D)
    Z, C = c[0].shape[1:3]
    x = ta.philox4x32_10(*c, np.uint32(seed & ta.MASK32), np.uint32(seed >> 32))
    out = np.empty((J, Z, C, 4, D), dtype=np.float32)
    for p in range(2):
        u1, u2 = ta.uniform24(x[2 * p]), ta.uniform24(x[2 * p + 1])
        rad = np.sqrt(np.float32(-2.0) * np.log(u1))
        angle = ta.TWO_PI_F32 * u2
        out[:, :, :, 2 * p], out[:, :, :, 2 * p + 1] = rad * np.cos(angle), rad * np.sin(angle)
    return out.reshape(J, Z * 8, D)[:, :S]


def test_mutation_a_naive_log_leaves_the_bounds():
    worst = _worst(_forward_ratios, ta.FWD_CASES, "naive_log")
    assert worst["sigma"][0] > 1e5 and worst["kl"][0] == np.inf, worst          # sigma = 0 below rho = -17: KL = +inf
    # with rho kept at or above 0, where 1 + exp(rho) loses nothing that matters, the mutant is inside: it is the small end
    case = ta.FWD_CASES[-1]
    inp = ta.reparam_inputs(case)
    rho = np.maximum(inp["rho"], np.float32(0.0))
    ref = ta.reparam_kl_reference(inp["mu"], rho, inp["eps"], case["lam"])
    kl = ta.emulate_reparam_kl(inp["mu"], rho, inp["eps"], case["lam"], "naive_log")[2]
    assert ta.worst_ratio(kl, ref.kl, ref.Y_kl, B["kl"]) <= 1.0


def test_mutation_b_short_sample_loop_leaves_the_bound():
    hit = [c["id"] for c in ta.BWD_CASES if _backward_ratios(c, "drop_last_sample")["grad_rho"] > 1.0]
    with_samples = [c["id"] for c in ta.BWD_CASES if c["S"] > 0 and c["grads"] != "kl_only"]
    assert hit == with_samples, (hit, with_samples)          # every case that has a sample to lose, lam = 1e-5 included


def test_sigmoid_above_the_threshold_is_the_same_float32():
    """Mutation (c) is not separable: see the module docstring."""
    for rho in (np.nextafter(np.float32(20.0), np.float32(np.inf)), np.float32(25.0), np.float32(30.0)):
        assert np.float32(1.0) / (np.float32(1.0) + np.exp(-rho)) == np.float32(1.0)
        assert 0.0 < 1.0 - 1.0 / (1.0 + np.exp(-np.float64(rho))) < 2.1e-9 < 2e-3 * B["grad_rho"]
    for case in ta.BWD_CASES:
        inp = ta.reparam_inputs(case)
        inp["rho"][:, -1] = 25.0
        assert int((inp["rho"] > 20.0).sum()) >= 2
        sigma = ta.emulate_reparam_kl(inp["mu"], inp["rho"], inp["eps"], case["lam"])[0]
        args = (inp["gu"], inp["gk"], inp["mu"], inp["rho"], inp["eps"], sigma, case["lam"])
        for a, b in zip(ta.emulate_reparam_kl_bwd(*args), ta.emulate_reparam_kl_bwd(*args, "sigmoid_everywhere")):
            assert np.array_equal(a.view(np.uint32), b.view(np.uint32))


def test_mutation_d_grad_sigma_without_count_leaves_the_bound():
    worst = _worst(_mnll_ratios, [c for c in ta.MNLL_CASES if c["m"] <= 5000], "no_count")
    assert worst["grad_sigma"][0] > 1.0 and worst["loss"][0] <= 1.0 and worst["grad_yhat"][0] <= 1.0, worst
    calibrated = [c for c in ta.MNLL_CASES if c["residuals"] == "calibrated" and c["m"] <= 5000]
    assert all(_mnll_ratios(c, "no_count")["grad_sigma"] > 1.0 for c in calibrated)


@pytest.mark.parametrize("mutate", ["swap_words", "eight_call"])
def test_mutations_e_f_counter_layout_leave_the_bound(mutate):
    outside = []
    for case in ta.PHILOX_CASES:
        J, S, D = case["J"], case["S"], case["D"]
        ref = ta.eps_reference(case["seed"], case["offset"], J, S, D)[0]
        got = ta.eps_reference(case["seed"], case["offset"], J, S, D, mutate)[0]
        if ta.worst_ratio(got, ref, np.abs(ref), B["eps"], ta.EPS_FLOOR) > 1.0:
            outside.append((J, S, D))
    # (1, 1, 1) is the one shape on which the counters coincide: i = j = z = 0 and sample 0 is call 0's first normal either way
    want = {s for s in ta.PHILOX_SHAPES if s[1] > 0 and s != (1, 1, 1)}
    assert set(outside) == want and len(outside) == 4 * len(want), outside
