"""Yardstick of the class-conditional image path (gbnf_image_flow_forward_y / gbnf_image_trainer_nll_step_y): float64 autograd of the
WHOLE loss ``k * mean_i(nll_i) + y_weight * mean_i CE(y_logits_i, argmax y_i)`` on ``image_grad_oracle.forward`` (imported unchanged)
plus the per-image prior, the class head and the cross-entropy of models/glow.py:62-84, 105-106 and image_experiment.py:227-239, and
numpy restatements of the closed forms the kernels of csrc/gbnf_image_ycond.hip implement.  Helper, not a test.

Paths: those of ``image_grad_oracle.leaf_params`` (the ``("learn_top", key)`` leaves included) and ("ycond", key) with key one of
``YCOND_KEYS``.  The g22 fixtures (tests/golden/image_ycond/, written by tests/golden/make_golden_image_ycond.py) are loaded here."""
import json
import os

import numpy as np
import torch

import image_grad_oracle as igo

YCOND_KEYS = ("cond_w", "cond_b", "cond_logs", "class_w", "class_b", "class_logs")
# state_dict name of every ycond path in a Glow module (the reference's names)
YCOND_NAMES = {"cond_w": "project_ycond.linear.weight", "cond_b": "project_ycond.linear.bias", "cond_logs": "project_ycond.logs",
               "class_w": "project_class.linear.weight", "class_b": "project_class.linear.bias", "class_logs": "project_class.logs"}


def leaf_params(spec, dtype=torch.float64):
    """image_grad_oracle.leaf_params plus the six ("ycond", key) leaves of the spec's "ycond" entry."""
    P = igo.leaf_params(spec, dtype)
    for key in YCOND_KEYS:
        P[("ycond", key)] = torch.tensor(np.asarray(spec["ycond"][key]), dtype=dtype, requires_grad=True)
    return P


def target(y):
    """t_i: the index of the largest entry of y_i, the lowest index on a tie (numpy's and torch's argmax)."""
    return np.argmax(np.asarray(y), axis=1)


def forward(spec, P, x, noise, y):
    """-> image_grad_oracle.forward's dict with z_mu, z_var ((n, Cz), per image), ll under that prior, and y_logits, nll_i, ce_i,
    correct added.  The dtype is the leaves'."""
    out = igo.forward(spec, P, x, noise)
    z = out["z"]
    dtype = z.dtype
    y = torch.as_tensor(np.asarray(y), dtype=dtype)
    Cz = z.shape[1]
    top = out["z_mu"].new_zeros(2 * Cz)
    if spec["learn_top"] is not None:                   # Conv2dZeros of a zero input: bias * exp(3 logs)
        top = P[("learn_top", "b")] * torch.exp(3.0 * P[("learn_top", "logs")])
    u = y @ P[("ycond", "cond_w")].t() + P[("ycond", "cond_b")]
    h = top.view(1, -1) + u * torch.exp(3.0 * P[("ycond", "cond_logs")]).view(1, -1)
    mu, lv = h[:, :Cz], h[:, Cz:]
    m4, l4 = mu.view(-1, Cz, 1, 1), lv.view(-1, Cz, 1, 1)
    ll = (-0.5 * (l4 + (z - m4) ** 2 * torch.exp(-l4))).sum(dim=[1, 2, 3]) + out["ldj"]
    zbar = z.mean(dim=[2, 3])
    logits = (zbar @ P[("ycond", "class_w")].t() + P[("ycond", "class_b")]) * torch.exp(3.0 * P[("ycond", "class_logs")]).view(1, -1)
    t = torch.as_tensor(target(y.detach().numpy()), dtype=torch.long)
    ce = torch.logsumexp(logits, dim=1) - logits.gather(1, t.view(-1, 1)).view(-1)
    out.update({"z_mu": mu, "z_var": lv, "u": u, "ll": ll, "nll_i": -ll, "zbar": zbar, "y_logits": logits, "ce_i": ce,
                "correct": (logits.argmax(dim=1) == t).sum()})
    return out


def yardstick(spec, x, noise, y, k=1.0, y_weight=0.01):
    """float64: (out dict detached, with nll = mean nll_i, loss_classes = mean ce_i, total = k nll + y_weight loss_classes;
    {path: gradient of total}) with respect to every leaf."""
    P = leaf_params(spec)
    out = forward(spec, P, x, noise, y)
    nll, lc = out["nll_i"].mean(), out["ce_i"].mean()
    total = k * nll + y_weight * lc
    total.backward()
    res = {key: v.detach() for key, v in out.items()}
    res.update({"nll": float(nll.detach()), "loss_classes": float(lc.detach()), "total": float(total.detach())})
    return res, {path: (t.grad if t.grad is not None else torch.zeros_like(t)).numpy() for path, t in P.items()}


# ---- the closed forms of csrc/gbnf_image_ycond.hip, in numpy (float64) ------------------------------------------------------------
def np_prior(top, yc, y):
    """(u, h) of the per-image prior: u = y Wc^T + bc, h = top_h + u exp(3 lc).  top: (bias, logs) of learn_top or None."""
    y = np.asarray(y, dtype=np.float64)
    Wc, bc, lc = (np.asarray(yc[key], dtype=np.float64) for key in ("cond_w", "cond_b", "cond_logs"))
    top_h = np.zeros(Wc.shape[0]) if top is None else np.asarray(top[0], dtype=np.float64) * np.exp(3.0 * np.asarray(top[1], dtype=np.float64))
    u = y @ Wc.T + bc
    return u, top_h[None, :] + u * np.exp(3.0 * lc)[None, :]


def np_ycond(z, ldj, top, yc, y, k=1.0, y_weight=0.01):
    """Everything gbnf_image_trainer_nll_step_y forms behind the forward, from z (n, Cz, Hz, Wz) and ldj (n,): dict(ll, y_logits, nll,
    loss_classes, correct, g_z, g_ldj and the gradients "top_b", "top_logs" (None without learn_top) and one per YCOND_KEYS)."""
    z, ldj, y = (np.asarray(a, dtype=np.float64) for a in (z, ldj, y))
    n, Cz = z.shape[:2]
    HW = z.shape[2] * z.shape[3]
    Wk, bk, lk = (np.asarray(yc[key], dtype=np.float64) for key in ("class_w", "class_b", "class_logs"))
    lc = np.asarray(yc["cond_logs"], dtype=np.float64)
    u, h = np_prior(top, yc, y)
    mu, lv = h[:, :Cz, None, None], h[:, Cz:, None, None]
    d, e = z - mu, np.exp(-lv)
    ll = (-0.5 * (lv + d * d * e)).sum(axis=(1, 2, 3)) + ldj
    zbar = z.mean(axis=(2, 3))
    sk, sc = np.exp(3.0 * lk), np.exp(3.0 * lc)
    logits = (zbar @ Wk.T + bk) * sk
    t = target(y)
    m = logits.max(axis=1, keepdims=True)
    lse = m[:, 0] + np.log(np.exp(logits - m).sum(axis=1))
    ce = lse - logits[np.arange(n), t]
    kn = k / n
    gl = np.exp(logits - lse[:, None])
    gl[np.arange(n), t] -= 1.0
    gl *= y_weight / n
    g_z = kn * d * e + ((gl * sk) @ Wk)[:, :, None, None] / HW
    g_h = np.concatenate([-(kn * d * e).sum(axis=(2, 3)), (kn * 0.5 * (1.0 - d * d * e)).sum(axis=(2, 3))], axis=1)
    out = {"ll": ll, "y_logits": logits, "nll": float(-ll.mean()), "loss_classes": float(ce.mean()),
           "correct": int((logits.argmax(axis=1) == t).sum()), "g_z": g_z, "g_ldj": np.full(n, -kn),
           "top_b": None, "top_logs": None}
    if top is not None:
        bias, logs = (np.asarray(a, dtype=np.float64) for a in top)
        out["top_b"] = g_h.sum(axis=0) * np.exp(3.0 * logs)
        out["top_logs"] = 3.0 * g_h.sum(axis=0) * bias * np.exp(3.0 * logs)
    out["cond_w"] = (g_h * sc).T @ y
    out["cond_b"] = (g_h * sc).sum(axis=0)
    out["cond_logs"] = 3.0 * (g_h * u * sc).sum(axis=0)
    out["class_w"] = (gl * sk).T @ zbar
    out["class_b"] = (gl * sk).sum(axis=0)
    out["class_logs"] = 3.0 * (gl * logits).sum(axis=0)
    return out


# ---- cases of the GPU tests: name -> (input_size, synth keywords, batch, seed, Y) ------------------------------------------------
# g22: the fixtures' geometry (a 4x4 top map in 8-wide storage); G: (16,4,4) with one level, Cz = 64, the widest; D: three levels;
# S1 / S70: the smallest component at n = 1 and at n = 70 (more images than a wave has lanes)
YC_CASES = {
    "g22": ((1, 16, 16), dict(h=32, K=2, L=2), 3, 1, 10),
    "G": ((16, 4, 4), dict(h=16, K=1, L=1), 2, 1, 256),
    "D": ((3, 32, 32), dict(h=16, K=1, L=3), 2, 1, 3),
    "S1": ((1, 8, 8), dict(h=16, K=1, L=1), 1, 1, 1),
    "S70": ((1, 8, 8), dict(h=16, K=1, L=1), 70, 2, 3),
}


def synth_y(n, Y, seed=0, soft_row=None):
    """(n, Y) float32 one-hot rows with a class drawn per row; ``soft_row``: that row is a soft distribution without a tie."""
    rng = np.random.RandomState(500 + seed)
    y = np.zeros((n, Y), dtype=np.float32)
    y[np.arange(n), rng.randint(0, Y, size=n)] = 1.0
    if soft_row is not None:
        p = rng.uniform(0.1, 1.0, size=Y) + np.arange(Y) * 1e-2
        y[soft_row] = (p / p.sum()).astype(np.float32)
    return y


def make_case(name):
    """-> (spec with "ycond", x, noise, y) of a YC_CASES entry."""
    from gbnf_amd import synth
    size, kw, N, seed, Y = YC_CASES[name]
    x, noise = synth.synth_image_batch(N, size, seed=100 + seed)
    return synth.synth_image_glow_spec(size, seed=seed, y_classes=Y, **kw), x, noise, synth_y(N, Y, seed)


def dev_ycond(spec, dev):
    """The spec's "ycond" arrays as contiguous float32 device tensors, in YCOND_KEYS order (native.NativeImageTrainer.bind_ycond)."""
    return [torch.from_numpy(np.ascontiguousarray(np.asarray(spec["ycond"][key], dtype=np.float32))).to(dev) for key in YCOND_KEYS]


# ---- the g22 fixtures: the reference's own class-conditional component ------------------------------------------------------------
G22 = ("g22_image_ycond_invconv_affine", "g22_image_ycond_lu", "g22_image_ycond_shuffle_additive")


def g22_load(name):
    data = np.load(os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden", "image_ycond", name + ".npz"))
    return json.loads(bytes(data["config"]).decode()), data


def g22_module(cfg, data, dev):
    """BoostedFlow(args) of the fixture's geometry, class-conditional, with the reference's state_dict and permutations loaded."""
    import argparse
    from gbnf_amd import BoostedFlow, image_glow
    args = argparse.Namespace(
        num_flows=cfg["K"], z_size=int(np.prod(cfg["input_size"])), density_evaluation=True, device=dev, cuda=dev.type == "cuda",
        component_type="glow", num_components=1, rho_init="decreasing", learn_top=cfg["learn_top"], y_classes=cfg["Y"], y_condition=True,
        sample_size=4, input_size=list(cfg["input_size"]), h_size=cfg["h"], num_blocks=cfg["L"], actnorm_scale=1.0,
        flow_permutation=cfg["permutation"], flow_coupling=cfg["coupling"], LU_decomposed=cfg["LU"], num_dequant_blocks=0,
        coupling_network="tanh", coupling_network_depth=cfg["depth"], batch_norm=False)
    m = BoostedFlow(args)
    glow = m.flows[0]
    glow.load_state_dict({k[len("param."):]: torch.from_numpy(data[k]) for k in data.files if k.startswith("param.")})
    k = 0
    for layer in glow.flow.layers:
        if isinstance(layer, image_glow.FlowStep):
            if not hasattr(layer, "invconv"):
                (layer.shuffle if hasattr(layer, "shuffle") else layer.reverse).set_indices(data[f"perm.{k}"])
            k += 1
    glow.set_actnorm_init()
    return m


def module_yardstick(glow, x, noise, y, k=1.0, y_weight=0.01):
    """``yardstick`` on a class-conditional ImageGlow's parameters -> (out, {state_dict name: gradient}); the LU factors through
    image_step_oracle's float64 restatement of get_weight."""
    import image_step_oracle as iso
    from gbnf_amd import image_glow
    sp = image_glow.image_spec_from_glow_module(glow)
    names = igo.state_names(glow)
    names.update({("ycond", key): nm for key, nm in YCOND_NAMES.items()})
    P = leaf_params(sp)
    leaves = dict(P)
    for i, layer in enumerate(glow.flow.layers):
        inv = getattr(layer, "invconv", None)
        if inv is not None and inv.LU_decomposed:
            path = next(p for p, nm in names.items() if nm == f"flow.layers.{i}.invconv.weight")
            t = {key: getattr(inv, key).detach().double().cpu().clone() for key in ("p", "sign_s", "lower", "upper", "log_s")}
            for key in ("lower", "upper", "log_s"):
                t[key].requires_grad_(True)
                leaves[path[:-1] + (key,)] = t[key]
                names[path[:-1] + (key,)] = f"flow.layers.{i}.invconv.{key}"
            P[path] = iso.lu_compose(t["p"], t["sign_s"], t["lower"], t["upper"], t["log_s"])
            del leaves[path], names[path]
    out = forward(sp, P, x, noise, y)
    nll, lc = out["nll_i"].mean(), out["ce_i"].mean()
    total = k * nll + y_weight * lc
    total.backward()
    res = {key: v.detach() for key, v in out.items()}
    res.update({"nll": float(nll.detach()), "loss_classes": float(lc.detach()), "total": float(total.detach())})
    return res, {names[path]: (t.grad if t.grad is not None else torch.zeros_like(t)).numpy() for path, t in leaves.items()}
