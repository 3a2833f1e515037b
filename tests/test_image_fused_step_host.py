"""CPU: the yardstick of the one-call image training step (tests/image_step_oracle.py) against image_grad_oracle.g21_yardstick, the
closed forms of csrc/gbnf_image_opt.hip against float64 autograd, the kink margin of the cases the GPU tests use, and the refusals of
the new entry points that need no device."""
import ctypes as C

import numpy as np
import pytest
import torch

import image_grad_oracle as igo
import image_step_oracle as iso


@pytest.mark.parametrize("name", igo.G21)
def test_helper_reproduces_the_g21_yardstick(name):
    cfg, data = igo.g21_load(name)
    glow = igo.g21_module(cfg, data, torch.device("cpu")).flows[0]
    nll_ref, ref = igo.g21_yardstick(glow, data["x"], data["noise"])
    nll, got = iso.module_yardstick(glow, data["x"], data["noise"])
    assert abs(nll - nll_ref) <= 1e-12 * abs(nll_ref)
    assert set(got) == set(ref) == set(dict(glow.named_parameters()))
    for nm, b in ref.items():
        assert np.abs(got[nm] - b).max() <= 1e-12 * max(float(np.abs(b).max()), 1.0), nm


@pytest.mark.parametrize("Cn", [4, 12, 48, 64])
def test_closed_forms_equal_float64_autograd(Cn):
    rng = np.random.RandomState(Cn)
    k, hw = 0.37, 49.0
    q, _ = np.linalg.qr(rng.standard_normal((Cn, Cn)))
    W = q * np.exp(0.1 * rng.standard_normal(Cn))[None, :]
    G = rng.standard_normal((Cn, Cn))
    # 1. the LU chain: loss = sum(G . W(lower, upper, log_s)) - k hw sum(log_s)
    f = {key: v.astype(np.float64) for key, v in iso.lu_factor(W).items()}
    t = {key: torch.tensor(f[key], dtype=torch.float64, requires_grad=key in ("lower", "upper", "log_s")) for key in f}
    loss = (torch.tensor(G) * iso.lu_compose(t["p"], t["sign_s"], t["lower"], t["upper"], t["log_s"])).sum() - k * hw * t["log_s"].sum()
    loss.backward()
    for got, key in zip(iso.np_lu_chain(G, f, k, hw), ("lower", "upper", "log_s")):
        ref = t[key].grad.numpy()
        assert np.abs(got - ref).max() <= 1e-10 * max(float(np.abs(ref).max()), 1.0), key
    # 2. the plain weight's log-det term
    Wt = torch.tensor(W, dtype=torch.float64, requires_grad=True)
    (-k * hw * torch.linalg.slogdet(Wt)[1]).backward()
    ref = Wt.grad.numpy()
    assert np.abs(iso.np_plain_logdet_grad(W, k, hw) - ref).max() <= 1e-10 * float(np.abs(ref).max())
    # 3. the learned top prior
    Cz = max(Cn // 2, 1)
    z = rng.standard_normal((3, Cz, 2, 5))
    bias = torch.tensor(0.3 * rng.standard_normal(2 * Cz), requires_grad=True)
    logs = torch.tensor(0.1 * rng.standard_normal(2 * Cz), requires_grad=True)
    h = bias * torch.exp(3.0 * logs)
    mu, lv = h[:Cz].view(1, -1, 1, 1), h[Cz:].view(1, -1, 1, 1)
    ll = (-0.5 * (lv + (torch.tensor(z) - mu) ** 2 * torch.exp(-lv))).sum(dim=[1, 2, 3])
    (k * -ll.mean()).backward()
    g_bias, g_logs = iso.np_top_grads(z, bias.detach().numpy(), logs.detach().numpy(), k)
    assert np.abs(g_bias - bias.grad.numpy()).max() <= 1e-10 * max(float(bias.grad.abs().max()), 1.0)
    assert np.abs(g_logs - logs.grad.numpy()).max() <= 1e-10 * max(float(logs.grad.abs().max()), 1.0)


@pytest.mark.parametrize("name", sorted(iso.STEP_CASES))
def test_step_cases_are_kink_free(name):
    sp, x, noise = iso.make_case(name)
    rows = igo.kink_report(sp, x, noise)
    assert rows and all(inside == 0 for inside, _ in rows), (name, rows)


def test_new_entry_points_refuse_a_null_trainer():
    """GBNF_ERR_INVALID before anything touches a device."""
    from gbnf_amd import native
    L = native.lib()
    n64 = C.c_int64(-7)
    h = native._OptHyper(kind=native.OPT_KIND["sgd"], step=1, lr=1e-3)
    one = C.c_void_p(256)            # (never dereferenced: the trainer is checked first)
    assert L.gbnf_image_trainer_bind_lu(None, 0, 0, one, one, one, one, one) == -1
    assert L.gbnf_image_trainer_bind_top(None, None, one, one) == -1
    assert L.gbnf_image_trainer_step_grad_floats(None, C.byref(n64)) == -1
    assert L.gbnf_image_trainer_step_workspace_bytes(None, 4, C.byref(n64)) == -1
    assert L.gbnf_image_trainer_apply_update(None, one, None, None, C.byref(h), one, None) == -1
    assert L.gbnf_image_trainer_nll_step(None, one, None, 4, 1.0, one, None, None, C.byref(h), one, one, 1 << 20, None) == -1
    assert b"null" in L.gbnf_last_error()
    assert n64.value == -7
