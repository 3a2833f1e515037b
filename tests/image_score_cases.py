"""Shared by tests/test_image_score_host.py and tests/test_hip_image_score.py: the mixture models of the image score tests and their
float64 yardstick (tests/image_grad_oracle.py::forward with x a leaf).

A model is one listed (case, seed) of ``igo.CASES`` as component 0; component j > 0 is component 0 with ``0.01 * randn`` added to
every FlowStep's ActNorm bias (``RandomState(perturbation seed)``, steps in order), so that the components' densities stay close and
every component's gradient truly enters the mixture's: independent seeds give one-hot responsibilities.  rho is the module's
"decreasing" initialisation, the weights rho / sum(rho).  Each model was checked in float64 to have no ReLU unit inside the kink
margin in any component and max_c r_c <= 0.9 in every row (tests/test_image_score_host.py re-asserts both).
"""
import copy

import numpy as np
import torch

import image_grad_oracle as igo

# name -> (case, seed of component 0, perturbation seeds of components 1 ..)
MIX_MODELS = {
    "A3": ("A", 1, (1, 2)),
    "D3": ("D", 2, (1, 2)),           # (three levels; D seed 1 with these perturbations puts two units inside the margin)
}
R_MAX = 0.9


def rho_decreasing(C):
    return np.maximum(1.0 / 2.0 ** np.arange(C, dtype=np.float64), 0.05)


def mixture_case(name):
    """-> (specs, log_w float64 (C,), x, noise)."""
    case, seed, pert = MIX_MODELS[name]
    sp, x, noise = igo.make_case(case, seed)
    specs = [sp]
    for s in pert:
        rng = np.random.RandomState(s)
        q = copy.deepcopy(sp)
        for lv in q["levels"]:
            for st in lv["steps"]:
                st["an_bias"] = (st["an_bias"] + 0.01 * rng.randn(*st["an_bias"].shape)).astype(np.float32)
        specs.append(q)
    rho = rho_decreasing(len(specs))
    return specs, np.log(rho / rho.sum()), x, noise


def component_yardstick(spec, x, noise, P=None):
    """float64: (ll (N,), d sum(ll) / dx) of one component with x a leaf."""
    xl = torch.tensor(np.asarray(x), dtype=torch.float64, requires_grad=True)
    out = igo.forward(spec, igo.leaf_params(spec) if P is None else P, xl, noise)
    out["ll"].sum().backward()
    return out["ll"].detach().numpy(), xl.grad.numpy()


def mixture_yardstick(specs, log_w, x, noise):
    """float64: dict(gx = d sum_n G / dx, G (N,), r (C, N), ll (C, N)) of G = logsumexp_c(log_w + ll_c), through autograd of the sum."""
    xl = torch.tensor(np.asarray(x), dtype=torch.float64, requires_grad=True)
    ll = torch.stack([igo.forward(sp, igo.leaf_params(sp), xl, noise)["ll"] for sp in specs])
    a = ll + torch.as_tensor(log_w, dtype=torch.float64).view(-1, 1)
    G = torch.logsumexp(a, dim=0)
    G.sum().backward()
    return {"gx": xl.grad.numpy(), "G": G.detach().numpy(), "r": torch.softmax(a, dim=0).detach().numpy(), "ll": ll.detach().numpy()}


def pre_adjoint_numpy(x, noise, g_logit_sq, g_ldj, bounds):
    """numpy restatement of the library's last adjoint: the gradient of the squeezed logits (n, 4C, H/2, W/2) and of ldj (n,) ->
    g_x (n, C, H, W):  g_x = (g_logit + g_ldj (2v - 1)) / (v (1 - v)) * bounds * 255 / 256  with v the forward's pre-logit value."""
    x = np.asarray(x, dtype=np.float64)
    n, C, H, W = x.shape
    u = (255.0 * x + (0.0 if noise is None else np.asarray(noise, dtype=np.float64))) / 256.0
    v = ((u * 2.0 - 1.0) * bounds + 1.0) / 2.0
    # un-squeeze: channel 4c + 2 (y & 1) + (x & 1), row y / 2, column x / 2
    g = np.asarray(g_logit_sq, dtype=np.float64).reshape(n, C, 2, 2, H // 2, W // 2).transpose(0, 1, 4, 2, 5, 3).reshape(n, C, H, W)
    return (g + np.asarray(g_ldj, dtype=np.float64).reshape(n, 1, 1, 1) * (2.0 * v - 1.0)) / (v * (1.0 - v)) * bounds * 255.0 / 256.0
