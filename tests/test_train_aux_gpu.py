"""The small kernels every training step runs, element by element against float64 and against a host Philox.

whvi_reparam_kl_f32 (csrc/abi.hip), whvi_reparam_kl_philox_f32, whvi_reparam_kl_bwd_f32, whvi_gauss_mnll_f32 and
whvi_gauss_mnll_bwd_f32 (csrc/train_aux.hip) feed the loss and the gradients of g_mu, g_rho and the likelihood's sigma on every
route.  The references are tools/train_aux_ref.py's (numpy float64 closed forms on the float32 inputs; Philox4x32-10 + Box-Muller
restated on the host), the cases are its lists, the inputs are drawn on the host by numpy.random.default_rng.
tests/test_train_aux_host.py checks the references against torch float64 autograd and Random123's vectors, and shows on these
same cases that a float32 emulation of the kernels stays inside the bounds below and that five named mistakes leave them.

Bounds.  u = 2^-23 is one float32 ulp, relative.  The library is built without fast-math and with -ffp-contract=off; each
device math call is budgeted 4 ulp (the OpenCL full-profile limit).  A YARDSTICK is the reference's expression with every term
replaced by its absolute value, per element: a float32 evaluation errs by a small multiple of u times it however the terms cancel.

    sigma                    |d| <= 1e-6 sigma_ref      expf and log1pf at 4 ulp each: 9.5e-7; above the threshold bit-equal to rho
    u[:, 0]                  bit-equal to g_mu
    u[:, 1 + k]              bit-equal to float32(sigma_gpu * eps)      one multiply, contraction off
    kl (per matrix)          |d| <= 2e-6 Y_kl           Y_kl = sum_i 0.5 (|log lam| + |log sigma| + 1 + sigma / lam + mu^2 / lam)
    grad_mu (per element)    |d| <= 2e-6 Y_mu           Y_mu = |gu0| + |gk mu / lam|
    grad_rho (per element)   |d| <= 2e-6 Y_rho          Y_rho = (sum_k |gu eps| + |gk| 0.5 (1 / lam + 1 / sigma)) softplus'(rho)
    eps                      |d| <= 2e-6 |z_ref| + 1e-7 logf 4 ulp halved by the root, sqrtf 4 ulp, sincosf 4 ulp, one product: 1.3e-6;
                                                        the floor covers rad = 0 and a result next to a zero of sin / cos.  A
                                                        wrong constant, counter word or call layout moves values by O(1).
    MNLL loss                |d| <= 2e-6 Y_loss         Y_loss = |scale| sum(0.5 z^2 + |log sigma| + 0.5 log 2 pi)
    grad_yhat (per element)  |d| <= 1e-6 Y_yhat         Y_yhat = |g scale| / sigma^2 (|y| + |y_hat|)
    grad_sigma               |d| <= 2e-6 Y_sigma        Y_sigma = |g scale| / sigma (sum z^2 + count)

2e-6 with a sum-of-|terms| yardstick is test_row_dot_vs_matmul's constant.  Every output element is compared; every test prints
its worst |error| / bound before it asserts, and the module prints the worst per quantity when it is done (``-s``).

g_rho is uniform in [-30, 30] -- log1pf(expf(rho)) against a naive logf(1 + expf(rho)) shows below -17 -- with 20, the float
above and the float below planted in every row.  The gradient formulas assume a finite 1 / sigma (include/whvi_hip.h): below
g_rho = -88.7 they do not hold, and no case goes there."""
import os
import sys

import numpy as np
import pytest
import torch

from whvi_amd import _hip

sys.path.insert(0, os.path.join(os.path.dirname(os.path.dirname(os.path.abspath(__file__))), "tools"))
import train_aux_ref as ta  # noqa: E402

pytestmark = pytest.mark.gpu
DEV = "cuda"
B = ta.BOUNDS
SENTINEL = -776.0
WORST = {}


def _dev(a):
    return None if a is None else torch.from_numpy(np.ascontiguousarray(a)).to(DEV)


def _host(t):
    return t.detach().cpu().numpy()


def _bits(a):
    return np.ascontiguousarray(a, dtype=np.float32).view(np.uint32)


def _ratio(name, where, got, ref, yardstick, floor=0.0):
    """Print, record and return the worst |error| / bound of one output; the caller asserts it is at most 1."""
    got, ref = np.asarray(got), np.asarray(ref)
    assert got.shape == ref.shape, (name, got.shape, ref.shape)
    ratio = ta.worst_ratio(got, ref, yardstick, B[name], floor)
    print(f"{name} [{where}]: worst |error| / bound = {ratio:.4f} over {got.size} elements")
    if ratio > WORST.get(name, (-1.0, ""))[0]:
        WORST[name] = (ratio, where)
    return ratio


@pytest.fixture(scope="module", autouse=True)
def _report():
    yield
    for name, (ratio, where) in WORST.items():
        print(f"\nworst |error| / bound of {name} on the device: {ratio:.4f} at {where}", end="")
    print()


def _forward_checks(where, inp, ref, u, sigma, kl):
    """sigma, u, kl of either forward launch against the float64 forms (``ref`` computed on the eps that was used)."""
    mu, rho, eps = inp["mu"], inp["rho"], inp["eps"]
    J, D = mu.shape
    S = eps.shape[1]
    sigma, u, kl = _host(sigma), _host(u), _host(kl)
    assert sigma.shape == (J, D) and u.shape == (J, 1 + S, D) and kl.shape == (J,)
    above = rho > np.float32(ta.SOFTPLUS_THRESHOLD)
    assert np.array_equal(_bits(sigma[above]), _bits(rho[above])), "sigma above the threshold is rho itself"
    r_sigma = _ratio("sigma", where, sigma, ref.sigma, ref.sigma)
    r_kl = _ratio("kl", where, kl, ref.kl, ref.Y_kl)
    assert np.array_equal(_bits(u[:, 0]), _bits(mu)), "u[:, 0] is g_mu"
    assert np.array_equal(_bits(u[:, 1:]), _bits(sigma[:, None, :] * eps)), "u[:, 1 + k] is one float32 product"
    assert r_sigma <= 1.0 and r_kl <= 1.0


@pytest.mark.parametrize("case", ta.FWD_CASES, ids=lambda c: c["id"])
def test_reparam_kl_against_float64(case, hip_lib):
    inp = ta.reparam_inputs(case)
    u, sigma, kl = _hip.reparam_kl(_dev(inp["mu"]), _dev(inp["rho"]), _dev(inp["eps"]), case["lam"])
    ref = ta.reparam_kl_reference(inp["mu"], inp["rho"], inp["eps"], case["lam"])
    _forward_checks(case["id"], inp, ref, u, sigma, kl)


@pytest.mark.parametrize("case", ta.BWD_CASES, ids=lambda c: c["id"])
def test_reparam_kl_backward_against_float64(case, hip_lib):
    """sigma is the GPU forward's, as ReparamKLFunction saves it; the reference takes softplus(rho) in float64."""
    inp = ta.reparam_inputs(case)
    mu, rho, eps = _dev(inp["mu"]), _dev(inp["rho"]), _dev(inp["eps"])
    sigma = _hip.reparam_kl(mu, rho, eps, case["lam"])[1]
    grad_mu, grad_rho = _hip.reparam_kl_bwd(_dev(inp["gu"]), _dev(inp["gk"]), mu, rho, eps, sigma, case["lam"])
    ref = ta.reparam_kl_bwd_reference(inp["gu"], inp["gk"], inp["mu"], inp["rho"], inp["eps"], case["lam"])
    r_mu = _ratio("grad_mu", case["id"], _host(grad_mu), ref.grad_mu, ref.Y_mu)
    r_rho = _ratio("grad_rho", case["id"], _host(grad_rho), ref.grad_rho, ref.Y_rho)
    assert r_mu <= 1.0 and r_rho <= 1.0


@pytest.mark.parametrize("case", ta.PHILOX_CASES, ids=lambda c: c["id"])
def test_inkernel_draw_is_the_host_stream(case, hip_lib):
    """Two launches on one state: the draws are the host stream at ``offset`` and ``offset + 2``, the state reads
    [seed, offset + 2 k, 0] after k launches (S = 0 included), and u / sigma / kl are those of the reported eps."""
    J, S, D, seed, offset = (case[k] for k in ("J", "S", "D", "seed", "offset"))
    lam = 0.37
    inp = ta.reparam_inputs({"J": J, "S": S, "D": D, "lam": lam}, with_eps=False)
    mu, rho = _dev(inp["mu"]), _dev(inp["rho"])
    state = torch.tensor([seed, offset, 0], dtype=torch.int64, device=DEV)
    ratios = []
    for launch in range(2):
        u, sigma, kl, eps = _hip.reparam_kl_philox(mu, rho, S, lam, state)
        at = offset + ta.CALLS_PER_BLOCK * launch
        assert state.tolist() == [seed, at + ta.CALLS_PER_BLOCK, 0]
        want, _ = ta.eps_reference(seed, at, J, S, D)
        eps_host = _host(eps)
        assert eps_host.shape == (J, S, D)
        ratios.append(_ratio("eps", f"{case['id']}, launch {launch}", eps_host, want, np.abs(want), ta.EPS_FLOOR))
        inp["eps"] = eps_host
        _forward_checks(f"philox {case['id']}, launch {launch}", inp,
                        ta.reparam_kl_reference(inp["mu"], inp["rho"], eps_host, lam), u, sigma, kl)
        u2, sigma2, kl2 = _hip.reparam_kl(mu, rho, eps, lam)
        assert torch.equal(u, u2) and torch.equal(sigma, sigma2) and torch.equal(kl, kl2)
    assert max(ratios) <= 1.0


@pytest.mark.parametrize("case", ta.MNLL_CASES, ids=lambda c: c["id"])
def test_gauss_mnll_against_float64(case, hip_lib):
    """Loss, every element of grad_yhat and grad_sigma, with an incoming gradient of -1.7.  ``gaps``: the backward is called
    through the C ABI into a buffer full of a sentinel, and everything outside the view must still hold it."""
    m, n_out, n_mc, layout = (case[k] for k in ("m", "n_out", "n_mc", "layout"))
    inp = ta.mnll_inputs(case)
    base = _dev(inp["base"])
    y_hat = inp["view"](base)
    y = _dev(inp["y"]).reshape(m, n_out, 1).expand(m, n_out, n_mc)
    assert tuple(y_hat.shape) == (m, n_out, n_mc) and np.array_equal(_host(y_hat), inp["dense"])
    sigma = torch.tensor(inp["sigma"], dtype=torch.float32, device=DEV)
    g = torch.tensor(inp["g"], dtype=torch.float32, device=DEV)
    part = _hip.gauss_mnll(y, y_hat, sigma, inp["scale"])
    assert tuple(part.shape) == (ta.mnll_blocks(m * n_out * n_mc), 2)
    loss = part[0, 0] if part.size(0) == 1 else part[:, 0].sum()            # as GaussMNLLFunction.forward
    if layout == "gaps":
        buf = torch.full_like(base, SENTINEL)
        grad_yhat, grad_sigma = inp["view"](buf), torch.empty((), dtype=torch.float32, device=DEV)
        size, hs, ys = _hip._mnll_dims(y, y_hat)
        rc = _hip.lib().whvi_gauss_mnll_bwd_f32(grad_yhat.data_ptr(), grad_sigma.data_ptr(), g.data_ptr(), part.data_ptr(),
                                                y.data_ptr(), y_hat.data_ptr(), sigma.data_ptr(), size, hs, ys,
                                                float(inp["scale"]), _hip._stream(base))
        assert rc == 0, _hip.last_error()
        outside = _host(buf)[:, :, n_out:]
        assert outside.size == n_mc * m * (ta.MNLL_WIDE - n_out) and bool((outside == SENTINEL).all())
        assert not bool((_host(grad_yhat) == SENTINEL).any())
    else:
        grad_yhat, grad_sigma = _hip.gauss_mnll_bwd(g, part, y, y_hat, sigma, inp["scale"])
        assert grad_yhat.stride() == y_hat.stride()
    y3 = np.broadcast_to(inp["y"][:, :, None], (m, n_out, n_mc))
    ref = ta.gauss_mnll_reference(y3, inp["dense"], inp["sigma"], inp["scale"], inp["g"])
    r_loss = _ratio("loss", case["id"], _host(loss), ref.loss, ref.Y_loss)
    r_yhat = _ratio("grad_yhat", case["id"], _host(grad_yhat), ref.grad_yhat, ref.Y_yhat)
    r_sigma = _ratio("grad_sigma", case["id"], _host(grad_sigma), ref.grad_sigma, ref.Y_sigma)
    assert r_loss <= 1.0 and r_yhat <= 1.0 and r_sigma <= 1.0
