"""Yardstick of the one-call image training step (gbnf_image_trainer_nll_step): float64 autograd of the WHOLE loss
``k * mean_i(-(log_normal_diag(z, z_mu, z_var) + logdet))`` on ``image_grad_oracle.forward`` -- the log-determinants of the 1x1 matrices
and the learned top prior included, the LU re-parameterisation of ``image_grad_oracle.g21_yardstick`` available per step -- and numpy
restatements of the three closed forms the kernels of csrc/gbnf_image_opt.hip implement.  Helper, not a test."""
import numpy as np
import torch

import image_grad_oracle as igo

# The cases of the fused-step tests: those of image_grad_oracle.CASES (first listed seed) and case G, the widest 1x1 matrix the path
# allows (16 x 4 x 4 input, one level: C = 64).  name -> (input_size, synth keywords, batch, seed)
STEP_CASES = {name: igo.CASES[name][:3] + (igo.CASES[name][3][0],) for name in ("A", "B", "C", "D", "F")}
STEP_CASES["G"] = ((16, 4, 4), dict(h=16, K=1, L=1), 2, 1)


def make_case(name):
    """-> (spec, x, noise) of a STEP_CASES entry (image_grad_oracle.make_case's recipe)."""
    from gbnf_amd import synth
    size, kw, N, seed = STEP_CASES[name]
    return synth.synth_image_glow_spec(size, seed=seed, **kw), *synth.synth_image_batch(N, size, seed=100 + seed)


def pixels(spec):
    """Pixels of every level's map."""
    _, H, W = spec["input_size"]
    out = []
    for _ in spec["levels"]:
        H, W = H // 2, W // 2
        out.append(H * W)
    return out


def lu_factor(w):
    """A (C, C) matrix -> the float32 LU parameterisation of models/layers.py:737-749: dict(p, sign_s, lower, upper, log_s)."""
    p, lower, upper = torch.linalg.lu(torch.as_tensor(np.asarray(w), dtype=torch.float64))
    s = torch.diag(upper)
    f = {"p": p, "sign_s": torch.sign(s), "lower": lower, "upper": torch.triu(upper, 1), "log_s": torch.log(torch.abs(s))}
    return {k: v.numpy().astype(np.float32) for k, v in f.items()}


def lu_compose(p, sign_s, lower, upper, log_s):
    """get_weight of the LU form (models/layers.py:757-768) on torch tensors."""
    n = lower.shape[0]
    mask = torch.tril(torch.ones(n, n, dtype=lower.dtype), -1)
    return p @ ((lower * mask + torch.eye(n, dtype=lower.dtype)) @ (upper * mask.t() + torch.diag(sign_s * torch.exp(log_s))))


def step_yardstick(spec, x, noise, k=1.0, lu=None):
    """float64: (nll, {path: gradient}) with nll = -mean(ll) and the gradients those of k * nll with respect to EVERY leaf: the paths
    of image_grad_oracle.leaf_params (perm_w with its log-det term, the learn_top leaves).  ``lu``: {(level, step): lu_factor(...)}:
    those steps' perm_w is composed from the factors, whose paths (..., "lower" | "upper" | "log_s") replace it."""
    P = igo.leaf_params(spec)
    leaves = dict(P)
    for (l, s), f in (lu or {}).items():
        path = ("levels", l, "steps", s, "perm_w")
        t = {key: torch.tensor(np.asarray(f[key]), dtype=torch.float64) for key in ("p", "sign_s", "lower", "upper", "log_s")}
        for key in ("lower", "upper", "log_s"):
            t[key].requires_grad_(True)
            leaves[path[:-1] + (key,)] = t[key]
        P[path] = lu_compose(t["p"], t["sign_s"], t["lower"], t["upper"], t["log_s"])
        del leaves[path]
    nll = -igo.forward(spec, P, x, noise)["ll"].mean()
    (k * nll).backward()
    return float(nll.detach()), {path: (t.grad if t.grad is not None else torch.zeros_like(t)).numpy() for path, t in leaves.items()}


def module_yardstick(glow, x, noise, k=1.0):
    """``step_yardstick`` on an ImageGlow's parameters -> (nll, {state_dict name: gradient}); k = 1 is image_grad_oracle.g21_yardstick."""
    from gbnf_amd import image_glow
    sp = image_glow.image_spec_from_glow_module(glow)
    names = igo.state_names(glow)
    lu, extra = {}, {}
    for i, layer in enumerate(glow.flow.layers):
        inv = getattr(layer, "invconv", None)
        if inv is not None and inv.LU_decomposed:
            path = next(p for p, nm in names.items() if nm == f"flow.layers.{i}.invconv.weight")
            lu[(path[1], path[3])] = {key: getattr(inv, key).detach().double().cpu().numpy() for key in ("p", "sign_s", "lower", "upper", "log_s")}
            del names[path]
            extra.update({path[:-1] + (key,): f"flow.layers.{i}.invconv.{key}" for key in ("lower", "upper", "log_s")})
    names.update(extra)
    nll, grads = step_yardstick(sp, x, noise, k, lu)
    return nll, {names[path]: g for path, g in grads.items()}


def dev_spec_top(spec, dev):
    """image_grad_oracle.dev_spec and, next to it, learn_top on the device: (dev spec, {"w", "b", "logs"} | None)."""
    ds = igo.dev_spec(spec, dev)
    top = spec["learn_top"]
    if top is None:
        return ds, None
    t = lambda a: torch.from_numpy(np.ascontiguousarray(np.asarray(a, dtype=np.float32))).to(dev)
    return ds, {"w": t(top["w"]), "b": t(top["b"]), "logs": t(top["logs"])}


# ---- the closed forms of csrc/gbnf_image_opt.hip, in numpy (float64) ------------------------------------------------------------
def np_lu_chain(G, f, k, hw):
    """G = dLoss/dW of the composed matrix (data path) -> (g_lower, g_upper, g_log_s), the log-det term -k hw of log_s included."""
    p, sign_s, lower, upper, log_s = (np.asarray(f[key], dtype=np.float64) for key in ("p", "sign_s", "lower", "upper", "log_s"))
    n = lower.shape[0]
    m = np.tril(np.ones((n, n)), -1)
    Lp, Up = lower * m + np.eye(n), upper * m.T + np.diag(sign_s * np.exp(log_s))
    A = p.T @ G
    T = Lp.T @ A
    return (A @ Up.T) * m, T * m.T, np.diag(T) * sign_s * np.exp(log_s) - k * hw


def np_plain_logdet_grad(W, k, hw):
    """Gradient of -k hw log|det W|."""
    return -k * hw * np.linalg.inv(np.asarray(W, dtype=np.float64)).T


def np_top_grads(z, bias, logs, k):
    """Gradients of k * mean_i(-log_normal_diag(z, mu, lv)) with h = bias exp(3 logs), mu = h[:Cz], lv = h[Cz:] -> (g_bias, g_logs)."""
    z, bias, logs = (np.asarray(a, dtype=np.float64) for a in (z, bias, logs))
    n, Cz = z.shape[:2]
    h = bias * np.exp(3.0 * logs)
    mu, lv = h[:Cz].reshape(1, -1, 1, 1), h[Cz:].reshape(1, -1, 1, 1)
    d2e = (z - mu) ** 2 * np.exp(-lv)
    g_z = k * (z - mu) * np.exp(-lv) / n
    g_h = np.concatenate([-g_z.sum(axis=(0, 2, 3)), (k / n * 0.5 * (1.0 - d2e)).sum(axis=(0, 2, 3))])
    return g_h * np.exp(3.0 * logs), 3.0 * g_h * h
