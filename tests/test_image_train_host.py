"""Host: the yardstick of the image training path (tests/image_grad_oracle.py) against the oracle, the ReLU kink margin of every
listed (case, seed), InvertibleConv1x1.composed_weight_tensor, and the new symbols in header, binding and library."""
import os
import re

import numpy as np
import pytest
import torch

import image_grad_oracle as igo
from oracle import gbnf_oracle as oracle

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
NEW_SYMBOLS = ("gbnf_image_trainer_create", "gbnf_image_trainer_destroy", "gbnf_image_trainer_trace_floats",
               "gbnf_image_trainer_workspace_bytes", "gbnf_image_trainer_forward", "gbnf_image_trainer_grad_floats",
               "gbnf_image_trainer_backward")


@pytest.mark.parametrize("name", sorted(igo.CASES))
def test_restatement_equals_oracle(name):
    sp, x, noise = igo.make_case(name, igo.CASES[name][3][0])
    z, z_mu, z_var, ld, ll = oracle.image_component_forward(sp, x, noise, dtype=torch.float64)
    with torch.no_grad():
        out = igo.forward(sp, igo.leaf_params(sp), x, noise)
    for key, ref in (("z", z), ("z_mu", z_mu), ("z_var", z_var), ("ldj", ld), ("ll", ll)):
        got = out[key].numpy()
        assert np.abs(got - ref).max() <= 1e-12 * max(1.0, float(np.abs(ref).max())), key


@pytest.mark.parametrize("name,seed", igo.CASE_SEEDS)
def test_no_relu_unit_inside_the_kink_margin(name, seed):
    """No ReLU pre-activation within 1e-5 * max|y| of zero, per activation tensor, in float64: an f32 kernel may legitimately take
    such a unit the other way, and one flipped unit moves a gradient by about 1/(n H W) of its scale."""
    sp, x, noise = igo.make_case(name, seed)
    rows = igo.kink_report(sp, x, noise)
    assert rows and all(units > 0 for _, units in rows)
    assert [inside for inside, _ in rows] == [0] * len(rows)


def test_restatement_gradients_match_finite_differences():
    """The yardstick's own gradients against central differences of its float64 forward (a few entries per tensor)."""
    sp, x, noise = igo.make_case("B", 1)
    rng = np.random.RandomState(3)
    out, g = igo.grads(sp, x, noise, None, np.ones(x.shape[0]))
    for path in list(g)[::3]:
        idx = tuple(int(rng.randint(0, d)) for d in g[path].shape)
        vals = []
        for sgn in (1.0, -1.0):
            P = igo.leaf_params(sp)
            with torch.no_grad():
                P[path][idx] += sgn * 1e-6
                vals.append(float(igo.forward(sp, P, x, noise)["ldj_noperm"].sum()))
        fd = (vals[0] - vals[1]) / 2e-6
        assert abs(fd - g[path][idx]) <= 1e-5 * max(1.0, abs(fd)), (path, fd, g[path][idx])


@pytest.mark.parametrize("name", igo.G21)
def test_restatement_gradients_match_the_reference(name):
    """The yardstick's float64 gradients against the reference's own f32 CPU autograd (fixtures g21): 1e-5 of each tensor's
    largest entry."""
    cfg, data = igo.g21_load(name)
    m = igo.g21_module(cfg, data, torch.device("cpu"))
    nll, grads = igo.g21_yardstick(m.flows[0], data["x"], data["noise"])
    assert abs(nll - float(data["nll"])) <= 1e-6 * abs(nll)
    ref = {k[len("grad."):]: data[k] for k in data.files if k.startswith("grad.")}
    assert set(grads) == set(ref)
    for k, b in ref.items():
        a = grads[k].reshape(b.shape)
        assert np.abs(a - b).max() <= 1e-5 * float(np.abs(b).max()), (k, float(np.abs(a - b).max()), float(np.abs(b).max()))


@pytest.mark.parametrize("lu", [False, True])
def test_composed_weight_tensor(lu):
    from gbnf_amd import image_glow
    torch.manual_seed(4)
    m = image_glow.InvertibleConv1x1(12, lu)
    with torch.no_grad():
        for p in m.parameters():
            p.add_(0.05 * torch.randn_like(p))
    w = m.composed_weight_tensor()
    assert w.dtype == torch.float32 and w.requires_grad and tuple(w.shape) == (12, 12)
    assert np.abs(w.detach().double().numpy() - m.composed_weight()).max() <= 1e-6
    ld = m.composed_log_det()
    assert abs(float(ld) - float(np.linalg.slogdet(m.composed_weight())[1])) <= 1e-5
    G = torch.randn(12, 12)
    (w * G).sum().backward()
    if not lu:
        assert np.abs(m.weight.grad.numpy() - G.numpy()).max() == 0.0
        return
    # float64 restatement of get_weight (models/layers.py:757-768)
    lower, upper, log_s = (t.detach().double().requires_grad_(True) for t in (m.lower, m.upper, m.log_s))
    mask = torch.tril(torch.ones(12, 12, dtype=torch.float64), -1)
    w64 = m.p.double() @ ((lower * mask + torch.eye(12, dtype=torch.float64)) @ (upper * mask.t() + torch.diag(m.sign_s.double() * torch.exp(log_s))))
    (w64 * G.double()).sum().backward()
    for mine, ref in ((m.lower.grad, lower.grad), (m.upper.grad, upper.grad), (m.log_s.grad, log_s.grad)):
        assert np.abs(mine.double().numpy() - ref.numpy()).max() <= 1e-5 * max(1.0, float(ref.abs().max()))


def test_new_symbols_in_header_binding_and_library():
    from gbnf_amd import native
    hdr = open(os.path.join(ROOT, "include", "gbnf.h")).read()
    for name in NEW_SYMBOLS:
        assert re.search(r"\bint\s+%s\s*\(" % name, hdr), f"{name} is not declared in include/gbnf.h"
        assert name in native.ABI_SYMBOLS, f"{name} is not in native.ABI_SYMBOLS"
    assert "typedef struct gbnf_image_trainer gbnf_image_trainer;" in hdr
    assert hasattr(native, "NativeImageTrainer")
    so = os.path.join(os.path.dirname(native.__file__), "libgbnf_hip.so")
    assert os.path.exists(so), "libgbnf_hip.so is not built"
    import ctypes
    L = ctypes.CDLL(so)
    for name in NEW_SYMBOLS:
        assert hasattr(L, name), f"{name} is not exported by libgbnf_hip.so"
