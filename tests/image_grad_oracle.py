"""Yardstick of the image training path: a float64 torch-autograd restatement of ``oracle.image_component_forward``.

The oracle's own forward is not differentiable with respect to the parameters (its ``_t()`` goes through numpy), so the
same arithmetic is restated here on leaf tensors.  ``relu`` is replaceable so that a test can look at every ReLU
pre-activation (the kink margin).  Parameter paths are those of ``native.NativeImageTrainer.backward``:

    ("levels", l, "steps", k, "an_bias" | "an_logs" | "perm_w")
    ("levels", l, "steps", k, "convs", q, "w" | "b" | "an_bias" | "an_logs" | "logs")
    ("levels", l, "split", key)        ("learn_top", key)
"""
import math

import numpy as np
import torch

CONV_KEYS = ("w", "b", "an_bias", "an_logs", "logs")


def leaf_params(spec, dtype=torch.float64):
    """{path: leaf tensor with requires_grad} of every float array of an image flow spec, in gradient-buffer order."""
    out = {}

    def leaf(path, a):
        out[path] = torch.tensor(np.asarray(a), dtype=dtype, requires_grad=True)

    def conv(path, c):
        for key in CONV_KEYS:
            if c[key] is not None:
                leaf(path + (key,), c[key])

    for l, lv in enumerate(spec["levels"]):
        for k, st in enumerate(lv["steps"]):
            p = ("levels", l, "steps", k)
            leaf(p + ("an_bias",), st["an_bias"])
            leaf(p + ("an_logs",), st["an_logs"])
            if st["perm_w"] is not None:
                leaf(p + ("perm_w",), st["perm_w"])
            for q, c in enumerate(st["convs"]):
                conv(p + ("convs", q), c)
        if lv["split"] is not None:
            conv(("levels", l, "split"), lv["split"])
    if spec["learn_top"] is not None:
        conv(("learn_top",), spec["learn_top"])
    return out


def _conv(P, path, x):
    """Conv2d (+ActNorm2d) or Conv2dZeros, models/layers.py:577-630."""
    w = P[path + ("w",)]
    y = torch.nn.functional.conv2d(x, w, P.get(path + ("b",)), padding=w.shape[-1] // 2)
    if path + ("an_bias",) in P:
        y = (y + P[path + ("an_bias",)].view(1, -1, 1, 1)) * torch.exp(P[path + ("an_logs",)].view(1, -1, 1, 1))
    if path + ("logs",) in P:
        y = y * torch.exp(P[path + ("logs",)].view(1, -1, 1, 1) * 3.0)
    return y


def _squeeze(x):
    B, C, H, W = x.shape
    x = x.view(B, C, H // 2, 2, W // 2, 2).permute(0, 1, 3, 5, 2, 4).contiguous()
    return x.view(B, C * 4, H // 2, W // 2)


def forward(spec, P, x, noise, relu=torch.relu):
    """-> dict(z, z_mu, z_var, ldj, ldj_noperm, ll).  ``ldj_noperm`` leaves out the log-determinants of the 1x1 ``perm_w``
    matrices (what gbnf_image_trainer_forward returns); ``ldj`` and ``ll`` are the oracle's.  The dtype is the leaves'."""
    first = next(iter(P.values()))
    dtype, dev = first.dtype, first.device             # (float64 on the host for the tests; tools/bench_image_train.py: f32 on the card)

    def t(a):
        return a.to(dev, dtype) if isinstance(a, torch.Tensor) else torch.as_tensor(np.asarray(a), dtype=dtype).to(dev)

    x = t(x)
    B, C, H, W = x.shape
    x = (255.0 * x + t(noise)) / 256.0
    ld = torch.full((B,), -math.log(256.0) * C * H * W, dtype=dtype, device=dev)
    bounds = torch.tensor(spec["bounds"], dtype=dtype, device=dev)
    x = ((x * 2.0 - 1.0) * bounds + 1.0) / 2.0
    logit = torch.log(x) - torch.log(1.0 - x)
    sp = torch.nn.functional.softplus
    ld = ld + (sp(logit) + sp(-logit) - sp((1.0 - bounds).log() - bounds.log())).flatten(1).sum(-1)
    ld_perm = torch.zeros((), dtype=dtype, device=dev)
    z = logit
    for l, lv in enumerate(spec["levels"]):
        z = _squeeze(z)
        for k, st in enumerate(lv["steps"]):
            p = ("levels", l, "steps", k)
            Bz, Cz, Hz, Wz = z.shape
            logs = P[p + ("an_logs",)].view(1, -1, 1, 1)
            z = (z + P[p + ("an_bias",)].view(1, -1, 1, 1)) * torch.exp(logs)
            ld = ld + logs.sum() * Hz * Wz
            if st["perm_w"] is not None:
                w = P[p + ("perm_w",)]
                z = torch.nn.functional.conv2d(z, w.view(Cz, Cz, 1, 1))
                ld_perm = ld_perm + torch.slogdet(w.double())[1].to(dtype) * Hz * Wz
            else:
                z = z[:, torch.as_tensor(np.asarray(st["perm"]), dtype=torch.long).to(dev)]
            z1, z2 = z[:, : Cz // 2], z[:, Cz // 2:]
            h = z1
            nc = len(st["convs"])
            for q in range(nc):
                h = _conv(P, p + ("convs", q), h)
                if q < nc - 1:
                    h = relu(h)
            if spec["coupling"] == "additive":
                z2 = z2 + h
            else:
                shift, raw = h[:, 0::2], h[:, 1::2]
                scale = torch.sigmoid(raw + 2.0)
                z2 = (z2 + shift) * scale
                ld = ld + torch.log(scale).sum(dim=[1, 2, 3])
            z = torch.cat([z1, z2], dim=1)
        if lv["split"] is not None:
            Cz = z.shape[1]
            z1, z2 = z[:, : Cz // 2], z[:, Cz // 2:]
            hh = _conv(P, ("levels", l, "split"), z1)
            mu, lvar = hh[:, 0::2], hh[:, 1::2]
            ld = ld + (-0.5 * (lvar + (z2 - mu) ** 2 * torch.exp(-lvar))).sum(dim=[1, 2, 3])
            z = z1
    Cz = z.shape[1]
    hprior = torch.zeros((B, 2 * Cz) + tuple(z.shape[2:]), dtype=dtype, device=dev)
    if spec["learn_top"] is not None:
        hprior = _conv(P, ("learn_top",), hprior)
    z_mu, z_var = hprior[:, :Cz], hprior[:, Cz:]
    ldj = ld + ld_perm
    ll = (-0.5 * (z_var + (z - z_mu) ** 2 * torch.exp(-z_var))).sum(dim=[1, 2, 3]) + ldj
    return {"z": z, "z_mu": z_mu, "z_var": z_var, "ldj": ldj, "ldj_noperm": ld, "ll": ll}


def kink_report(spec, x, noise):
    """[(units within 1e-5 * max|y| of zero, units)] per ReLU pre-activation tensor y of the float64 forward."""
    rows = []

    def relu(y):
        m = float(y.detach().abs().max())
        rows.append((int((y.detach().abs() < 1e-5 * m).sum()), y.numel()))
        return torch.relu(y)

    with torch.no_grad():
        forward(spec, leaf_params(spec), x, noise, relu=relu)
    return rows


def grads(spec, x, noise, g_z, g_ldj, dtype=torch.float64):
    """Gradients of  sum(g_z * z) + sum(g_ldj * ldj_noperm)  with respect to every parameter the trainer binds
    (g_z / g_ldj None = zero) -> (out dict detached, {path: gradient as numpy})."""
    P = leaf_params(spec, dtype)
    out = forward(spec, P, x, noise)
    loss = torch.zeros((), dtype=dtype)
    if g_z is not None:
        loss = loss + (torch.as_tensor(np.asarray(g_z), dtype=dtype) * out["z"]).sum()
    if g_ldj is not None:
        loss = loss + (torch.as_tensor(np.asarray(g_ldj), dtype=dtype) * out["ldj_noperm"]).sum()
    loss.backward()
    g = {path: (t.grad if t.grad is not None else torch.zeros_like(t)).numpy() for path, t in P.items() if path[0] != "learn_top"}
    return {k: v.detach() for k, v in out.items()}, g


# The cases of the image training tests: name -> (input_size, synth_image_glow_spec keywords, batch, seeds).  Every (case, seed) was
# checked to have NO ReLU pre-activation within the kink margin in float64 (tests/test_image_train_host.py re-asserts it), with
# synth.synth_image_glow_spec(size, seed=s, ...) and synth.synth_image_batch(N, size, seed=100 + s).
CASES = {
    "A": ((2, 8, 12), dict(h=16, K=1, L=1), 3, (1, 2, 3, 4, 5, 6)),
    "B": ((1, 16, 16), dict(h=32, K=2, L=2), 3, (1, 5)),
    "C": ((3, 16, 32), dict(h=48, K=1, L=2, depth=2, coupling="additive", permutation="shuffle"), 2, (5, 8, 12, 13, 14, 18, 21)),
    "C2": ((3, 32, 32), dict(h=48, K=1, L=2, depth=2, coupling="additive", permutation="shuffle"), 1, (7,)),
    "D": ((3, 32, 32), dict(h=32, K=1, L=3, depth=0), 2, (1, 2, 3, 6)),
    "E": ((1, 12, 32), dict(h=272, K=1, L=1), 1, (5, 15, 19)),
    # beyond the listed cases: 384 hidden channels, where the data gradient of the first 3x3 (a 3x3 FROM 384 channels, 166 KB of
    # strip) is staged in two halves by img_conv_kernel -- case E's 272 channels (117 KB) still fit one pass
    "E2": ((1, 12, 32), dict(h=384, K=1, L=1), 1, (3,)),
    "F": ((1, 28, 20), dict(h=32, K=2, L=2, learn_top=False, permutation="reverse"), 1, (1, 2, 4, 6)),
}
CASE_SEEDS = [(name, s) for name, (_, _, _, seeds) in CASES.items() for s in seeds]


def dev_spec(spec, dev):
    """The spec with every float array as a contiguous float32 tensor on ``dev`` (perm stays host; no learn_top): what
    native.NativeImageTrainer binds."""
    def t(a):
        return None if a is None else torch.from_numpy(np.ascontiguousarray(np.asarray(a, dtype=np.float32))).to(dev)

    def conv(c):
        return None if c is None else {k: t(c[k]) for k in CONV_KEYS}

    levels = [{"steps": [{"an_bias": t(st["an_bias"]), "an_logs": t(st["an_logs"]), "perm_w": t(st["perm_w"]), "perm": st["perm"],
                          "convs": [conv(c) for c in st["convs"]]} for st in lv["steps"]], "split": conv(lv["split"])}
              for lv in spec["levels"]]
    return {**spec, "levels": levels, "learn_top": None}


def make_case(name, seed):
    """-> (spec, x, noise) of a listed (case, seed)."""
    from gbnf_amd import synth
    size, kw, N, _ = CASES[name]
    return synth.synth_image_glow_spec(size, seed=seed, **kw), *synth.synth_image_batch(N, size, seed=100 + seed)


# ---- the g21 fixtures (tests/golden/image_grads/, written by tests/golden/make_golden_image_grads.py): the reference's own gradients of one component ----------------
G21 = ("g21_image_grads_invconv_affine", "g21_image_grads_lu", "g21_image_grads_shuffle_additive")


def g21_load(name):
    import json
    import os
    data = np.load(os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden", "image_grads", name + ".npz"))
    return json.loads(bytes(data["config"]).decode()), data


def g21_module(cfg, data, dev):
    """BoostedFlow(args) of the fixture's geometry with the reference's state_dict and permutations loaded into component 0."""
    import argparse
    from gbnf_amd import BoostedFlow, image_glow
    args = argparse.Namespace(
        num_flows=cfg["K"], z_size=int(np.prod(cfg["input_size"])), density_evaluation=True, device=dev, cuda=dev.type == "cuda",
        component_type="glow", num_components=1, rho_init="decreasing", learn_top=cfg["learn_top"], y_classes=0, y_condition=False,
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


def state_names(glow):
    """{gradient path: state_dict name} of an ImageGlow (a 1x1's path maps to 'invconv.weight'; LU factors have no path)."""
    from gbnf_amd import image_glow
    names = {}

    def conv(path, prefix, m):
        zeros = isinstance(m, image_glow.Conv2dZeros)
        names[path + ("w",)] = prefix + ".conv.weight"
        if m.conv.bias is not None:
            names[path + ("b",)] = prefix + ".conv.bias"
        if zeros:
            names[path + ("logs",)] = prefix + ".logs"
        else:
            names[path + ("an_bias",)], names[path + ("an_logs",)] = prefix + ".actnorm.bias", prefix + ".actnorm.logs"

    l = k = 0
    for i, layer in enumerate(glow.flow.layers):
        if isinstance(layer, image_glow.FlowStep):
            p, pre = ("levels", l, "steps", k), f"flow.layers.{i}"
            names[p + ("an_bias",)], names[p + ("an_logs",)] = pre + ".actnorm.bias", pre + ".actnorm.logs"
            if hasattr(layer, "invconv"):
                names[p + ("perm_w",)] = pre + ".invconv.weight"
            q = 0
            for j, mod in enumerate(layer.block.network):
                if not isinstance(mod, torch.nn.ReLU):
                    conv(p + ("convs", q), f"{pre}.block.network.{j}", mod)
                    q += 1
            k += 1
        elif isinstance(layer, image_glow.Split2d):
            conv(("levels", l, "split"), f"flow.layers.{i}.conv", layer.conv)
            l, k = l + 1, 0
    if glow.learn_top:
        conv(("learn_top",), "learn_top_fn", glow.learn_top_fn)
    return names


def g21_yardstick(glow, x, noise):
    """float64: (nll, {state_dict name: gradient}) of nll = -mean(ll) on the module's parameters, the LU factors through a float64
    restatement of get_weight (models/layers.py:757-768)."""
    from gbnf_amd import image_glow
    sp = image_glow.image_spec_from_glow_module(glow)
    P = leaf_params(sp)
    names = state_names(glow)
    leaves = {names[path]: t for path, t in P.items()}
    for i, layer in enumerate(glow.flow.layers):
        inv = getattr(layer, "invconv", None)
        if inv is not None and inv.LU_decomposed:
            path = next(p for p, nm in names.items() if nm == f"flow.layers.{i}.invconv.weight")
            lower, upper, log_s = (t.detach().double().cpu().requires_grad_(True) for t in (inv.lower, inv.upper, inv.log_s))
            n = lower.shape[0]
            mask = torch.tril(torch.ones(n, n, dtype=torch.float64), -1)
            P[path] = inv.p.double().cpu() @ ((lower * mask + torch.eye(n, dtype=torch.float64)) @
                                              (upper * mask.t() + torch.diag(inv.sign_s.double().cpu() * torch.exp(log_s))))
            del leaves[names[path]]
            leaves.update({f"flow.layers.{i}.invconv.lower": lower, f"flow.layers.{i}.invconv.upper": upper,
                           f"flow.layers.{i}.invconv.log_s": log_s})
    nll = -forward(sp, P, x, noise)["ll"].mean()
    nll.backward()
    return float(nll.detach()), {nm: (t.grad if t.grad is not None else torch.zeros_like(t)).numpy() for nm, t in leaves.items()}
