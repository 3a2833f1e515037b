"""GPU: the image training path (gbnf_image_trainer_*, native.NativeImageTrainer, BoostedImageFlow in train mode) against the
float64 yardstick (tests/image_grad_oracle.py).  Tolerances are those of tests/test_hip_train.py: forward z within 2e-5 of its
largest entry and ldj within 1e-5 relative; gradients within G_RTOL = 2e-4 of each tensor's largest entry (floor 1e-3)."""
import numpy as np
import pytest

import image_grad_oracle as igo
from conftest import rel_err

pytestmark = pytest.mark.gpu
G_RTOL = 2e-4
Z_RTOL = 2e-5
LL_RTOL = 1e-5


_dev_spec = igo.dev_spec


def _spec_from_dev(spec, dspec):
    """numpy spec with the values the device tensors hold now."""
    def a(t):
        return None if t is None else t.detach().cpu().numpy()

    def conv(c):
        return None if c is None else {k: a(c[k]) for k in igo.CONV_KEYS}

    levels = []
    for lv in dspec["levels"]:
        steps = [{"an_bias": a(st["an_bias"]), "an_logs": a(st["an_logs"]), "perm_w": a(st["perm_w"]), "perm": st["perm"],
                  "convs": [conv(c) for c in st["convs"]]} for st in lv["steps"]]
        levels.append({"steps": steps, "split": conv(lv["split"])})
    return {**spec, "levels": levels}


def _check_forward(z, ldj, out, what):
    zr, lr = out["z"].numpy(), out["ldj_noperm"].numpy()
    ez = float(np.abs(z.cpu().numpy() - zr).max()) / float(np.abs(zr).max())
    el = rel_err(ldj.cpu().numpy(), lr)
    print(f"{what}: forward z {ez:.3e} of {Z_RTOL}, ldj {el:.3e} of {LL_RTOL}")
    assert ez <= Z_RTOL, what
    assert el < LL_RTOL, what


def _check_grads(views, ref, what, scale_by=1.0):
    assert set(views) == set(ref)
    worst, where = 0.0, None
    for path, b in ref.items():
        a = views[path].cpu().numpy().astype(np.float64) / scale_by
        assert a.shape == b.shape, path
        scale = max(float(np.abs(b).max()), 1e-3)
        if float(np.abs(a - b).max()) / scale >= worst:
            worst, where = float(np.abs(a - b).max()) / scale, path
    print(f"{what}: worst gradient error {worst:.3e} of {G_RTOL} ({where})")
    for path, b in ref.items():
        a = views[path].cpu().numpy().astype(np.float64) / scale_by
        scale = max(float(np.abs(b).max()), 1e-3)
        assert np.abs(a - b).max() <= G_RTOL * scale, f"{what}: gradient {path} shape {b.shape}: {np.abs(a - b).max()} vs scale {scale}"


@pytest.mark.parametrize("name,seed", igo.CASE_SEEDS)
def test_trainer_matches_yardstick(name, seed):
    import torch
    from gbnf_amd import native
    sp, x, noise = igo.make_case(name, seed)
    dev = torch.device("cuda:0")
    tr = native.NativeImageTrainer(_dev_spec(sp, dev))
    xd, nd = torch.from_numpy(x).to(dev), torch.from_numpy(noise).to(dev)
    z, ldj, trace = tr.forward(xd, nd)
    rng = np.random.RandomState(1000 + seed)
    g_z = rng.standard_normal(tuple(z.shape)).astype(np.float32)
    g_ldj = rng.standard_normal(x.shape[0]).astype(np.float32)
    out, ref = igo.grads(sp, x, noise, g_z, g_ldj)
    _check_forward(z, ldj, out, f"{name}/{seed}")
    _, views = tr.backward(trace, torch.from_numpy(g_z).to(dev), torch.from_numpy(g_ldj).to(dev))
    _check_grads(views, ref, f"{name}/{seed}")
    if seed == igo.CASES[name][3][0] and name in ("A", "C"):          # g_z = None: the log-det path alone
        _, ref0 = igo.grads(sp, x, noise, None, g_ldj)
        _, views0 = tr.backward(trace, None, torch.from_numpy(g_ldj).to(dev))
        _check_grads(views0, ref0, f"{name}/{seed} g_z=None")
    tr.close()


@pytest.mark.parametrize("name", ["B", "F", "D"])
def test_trainer_forward_equals_f32_evaluation_handle(name):
    """z and ldj + sum H W log|det W| against a math="f32" NativeImageFlow on the same parameters."""
    import torch
    from gbnf_amd import native
    seed = igo.CASES[name][3][0]
    sp, x, noise = igo.make_case(name, seed)
    dev = torch.device("cuda:0")
    xd, nd = torch.from_numpy(x).to(dev), torch.from_numpy(noise).to(dev)
    tr = native.NativeImageTrainer(_dev_spec(sp, dev))
    z, ldj, _ = tr.forward(xd, nd)
    ze, ldje, _ = native.NativeImageFlow(sp, math="f32").forward(xd, nd)
    extra = 0.0
    for lv, hw in zip(sp["levels"], tr.level_pixels):
        for st in lv["steps"]:
            if st["perm_w"] is not None:
                extra += hw * float(np.linalg.slogdet(st["perm_w"].astype(np.float64))[1])
    assert float((z - ze).abs().max()) <= Z_RTOL * float(ze.abs().max())
    assert rel_err((ldj.double() + extra).cpu().numpy(), ldje.double().cpu().numpy()) < LL_RTOL


def test_live_parameters_and_accumulation():
    """One SGD update applied in place, then a second forward / backward WITHOUT re-creating the trainer, against the yardstick on
    the updated parameters; and two backward calls accumulate into one buffer."""
    import torch
    from gbnf_amd import native
    sp, x, noise = igo.make_case("B", 1)
    dev = torch.device("cuda:0")
    ds = _dev_spec(sp, dev)
    tr = native.NativeImageTrainer(ds)
    xd, nd = torch.from_numpy(x).to(dev), torch.from_numpy(noise).to(dev)
    rng = np.random.RandomState(7)
    z, ldj, trace = tr.forward(xd, nd)
    g_z = torch.from_numpy(rng.standard_normal(tuple(z.shape)).astype(np.float32)).to(dev)
    g_ldj = torch.from_numpy(rng.standard_normal(x.shape[0]).astype(np.float32)).to(dev)
    flat, views = tr.backward(trace, g_z, g_ldj)
    tensors = {}
    for l, lv in enumerate(ds["levels"]):
        for k, st in enumerate(lv["steps"]):
            for key in ("an_bias", "an_logs", "perm_w"):
                if st[key] is not None:
                    tensors[("levels", l, "steps", k, key)] = st[key]
            for q, c in enumerate(st["convs"]):
                tensors.update({("levels", l, "steps", k, "convs", q, key): c[key] for key in igo.CONV_KEYS if c[key] is not None})
        if lv["split"] is not None:
            tensors.update({("levels", l, "split", key): lv["split"][key] for key in igo.CONV_KEYS if lv["split"][key] is not None})
    assert set(tensors) == set(views)
    key_before = tr.key()
    for path, t in tensors.items():
        t.sub_(1e-3 * views[path] / max(float(views[path].abs().max()), 1e-6))         # in place: same storage
    assert tr.key() == key_before
    sp2 = _spec_from_dev(sp, ds)
    assert igo.kink_report(sp2, x, noise) and all(inside == 0 for inside, _ in igo.kink_report(sp2, x, noise))
    z2, ldj2, trace2 = tr.forward(xd, nd)
    out2, ref2 = igo.grads(sp2, x, noise, g_z.cpu().numpy(), g_ldj.cpu().numpy())
    _check_forward(z2, ldj2, out2, "after the update")
    assert float((z2 - z).abs().max()) > 0.0
    flat2, views2 = tr.backward(trace2, g_z, g_ldj)
    _check_grads(views2, ref2, "after the update")
    _, views3 = tr.backward(trace2, g_z, g_ldj, out=flat2)                           # accumulates: twice the gradient
    _check_grads(views3, ref2, "accumulated", scale_by=2.0)


# ---------------------------------------------------------------------------------------------------------------------
# the module: BoostedFlow(args) in train mode
# ---------------------------------------------------------------------------------------------------------------------
def _module(input_size, h, K, L, dev, depth=1, coupling="affine", permutation="invconv", learn_top=True, LU=False, C=1):
    import argparse
    from gbnf_amd import BoostedFlow
    args = argparse.Namespace(
        num_flows=K, z_size=int(np.prod(input_size)), density_evaluation=True, device=dev, cuda=True, component_type="glow",
        num_components=C, rho_init="decreasing", learn_top=learn_top, y_classes=0, y_condition=False, sample_size=4,
        input_size=list(input_size), h_size=h, num_blocks=L, actnorm_scale=1.0, flow_permutation=permutation, flow_coupling=coupling,
        LU_decomposed=LU, num_dequant_blocks=0, coupling_network="tanh", coupling_network_depth=depth, batch_norm=False)
    return BoostedFlow(args)


def _nll(z, z_mu, z_var, ldj):
    """-mean(log_normal_diag(z, z_mu, z_var) + logdet): image_experiment.py:227, utils/distributions.py:13-21."""
    return -((-0.5 * (z_var + (z - z_mu) ** 2 * (-z_var).exp())).sum(dim=[1, 2, 3]) + ldj).mean()


def test_module_train_mode_matches_yardstick():
    """model(x=x, components=0) in train mode, nll.backward(): every parameter's .grad (the 1x1 matrices' log-det term and the
    learned top prior included) against float64 autograd of the yardstick."""
    import torch
    from gbnf_amd import image_glow
    sp, x, noise = igo.make_case("B", 5)
    dev = torch.device("cuda:0")
    m = _module((1, 16, 16), 32, 2, 2, dev)
    image_glow.load_image_spec(m.flows[0], sp)
    m.train()
    xd, nd = torch.from_numpy(x).to(dev), torch.from_numpy(noise).to(dev)
    z, z_mu, z_var, ldj, y = m.component_forward(xd, 0, nd)
    assert y is None and z.requires_grad and ldj.requires_grad
    nll = _nll(z, z_mu, z_var, ldj)
    nll.backward()
    P = igo.leaf_params(sp)
    out = igo.forward(sp, P, x, noise)
    nll64 = -out["ll"].mean()
    nll64.backward()
    assert abs(float(nll.detach()) - float(nll64.detach())) <= LL_RTOL * abs(float(nll64.detach()))
    _, bind = m.native_trainer(0)
    views = {path: (obj.weight if isinstance(obj, image_glow.InvertibleConv1x1) else obj).grad.reshape(P[path].shape) for path, obj, _ in bind}
    top = m.flows[0].learn_top_fn
    views[("learn_top", "b")], views[("learn_top", "logs")] = top.conv.bias.grad, top.logs.grad.reshape(-1)
    views[("learn_top", "w")] = top.conv.weight.grad
    assert float(top.conv.weight.grad.abs().max()) == 0.0
    _check_grads(views, {path: t.grad.numpy() for path, t in P.items()}, "module B/5")
    with pytest.raises(NotImplementedError):
        m.component_forward(xd.clone().requires_grad_(True), 0, nd)
    # forward(x=..., components=...) takes the same path (fresh noise: shapes and differentiability only)
    z2, mu2, var2, ldj2, _ = m(x=xd, components="c")
    assert z2.shape == z.shape and mu2.shape == z.shape and var2.shape == z.shape and ldj2.requires_grad


def test_module_lu_gradients_reach_the_factors():
    """LU_decomposed: the chain from g_perm_weight to lower / upper / log_s, against float64 autograd of the yardstick composed with a
    float64 restatement of get_weight (models/layers.py:757-768)."""
    import torch
    from gbnf_amd import image_glow
    sp, x, noise = igo.make_case("A", 1)
    dev = torch.device("cuda:0")
    torch.manual_seed(11)
    m = _module((2, 8, 12), 16, 1, 1, dev, LU=True)
    inv = m.flows[0].flow.layers[1].invconv
    sp["levels"][0]["steps"][0]["perm_w"] = inv.composed_weight().astype(np.float32)
    for mod in m.flows[0].modules():               # everything but the 1x1 from the spec
        if isinstance(mod, image_glow.FlowStep):
            st = sp["levels"][0]["steps"][0]
            image_glow._put(mod.actnorm.bias, st["an_bias"]); image_glow._put(mod.actnorm.logs, st["an_logs"])
            for cm, c in zip([q for q in mod.block.network if not isinstance(q, torch.nn.ReLU)], st["convs"]):
                image_glow._load_conv(cm, c)
    image_glow._load_conv(m.flows[0].learn_top_fn, sp["learn_top"])
    m.flows[0].set_actnorm_init()
    assert all(inside == 0 for inside, _ in igo.kink_report(sp, x, noise))
    m.train()
    xd, nd = torch.from_numpy(x).to(dev), torch.from_numpy(noise).to(dev)
    nll = _nll(*m.component_forward(xd, 0, nd)[:4])
    nll.backward()
    P = igo.leaf_params(sp)
    lower, upper, log_s = (t.detach().double().cpu().requires_grad_(True) for t in (inv.lower, inv.upper, inv.log_s))
    n = lower.shape[0]
    mask = torch.tril(torch.ones(n, n, dtype=torch.float64), -1)
    P[("levels", 0, "steps", 0, "perm_w")] = inv.p.double().cpu() @ ((lower * mask + torch.eye(n, dtype=torch.float64)) @
                                                                      (upper * mask.t() + torch.diag(inv.sign_s.double().cpu() * torch.exp(log_s))))
    nll64 = -igo.forward(sp, P, x, noise)["ll"].mean()
    nll64.backward()
    assert abs(float(nll.detach()) - float(nll64.detach())) <= LL_RTOL * abs(float(nll64.detach()))
    _check_grads({"lower": inv.lower.grad, "upper": inv.upper.grad, "log_s": inv.log_s.grad},
                 {"lower": lower.grad.numpy(), "upper": upper.grad.numpy(), "log_s": log_s.grad.numpy()}, "LU factors")


def test_eval_and_no_grad_keep_the_evaluation_path():
    """eval() / no_grad() keep the evaluation path: the 3-tuple of the evaluation handle, the same handle class, no trainer created,
    and its values.  z is written once per element and must agree BIT FOR BIT with a fresh evaluation handle.  ldj and ll cannot be
    held to that: the evaluation kernels add their per-wave log-det partials to ldj[n] with float atomics, in no fixed order, so the
    evaluation handle does not reproduce its own last bit (measured on the unchanged handle, g12 component 0: 21 of 40 identical
    calls differ from the first by one ulp, 9.8e-4 at |ldj| = 1.5e4; z never).  Two orders of the same m additions differ by at most m
    roundings of the running sum; a g12 image receives fewer than 128 partials (4 steps x at most 16 waves, one Split2d x 16), hence
    the bar of 128 ulp-halves, 128 * 2^-24 relative, on ldj and ll."""
    import torch
    from conftest import load_image_case
    from gbnf_amd import image_glow, native
    cfg, specs, x, noise, data = load_image_case("g12_image_glow_invconv_affine")
    dev = torch.device("cuda:0")
    m = _module((3, 32, 32), cfg["h"], cfg["K"], cfg["L"], dev, depth=cfg["depth"], coupling=cfg["coupling"],
                permutation=cfg["permutation"], learn_top=cfg["learn_top"], C=cfg["C"])
    for c, sp in enumerate(specs):
        image_glow.load_image_spec(m.flows[c], sp)
    xd, nd = torch.from_numpy(x).to(dev), torch.from_numpy(noise).to(dev)
    ref = [native.NativeImageFlow(sp).forward(xd, nd) for sp in specs]
    m.train()
    with torch.no_grad():
        got_train = [m.component_forward(xd, c, nd) for c in range(cfg["C"])]
    m.eval()
    got_eval = [m.component_forward(xd, c, nd) for c in range(cfg["C"])]
    for c in range(cfg["C"]):
        assert isinstance(m.native_flow(c), native.NativeImageFlow)
        for got in (got_train[c], got_eval[c]):
            assert len(got) == 3 and torch.equal(got[0], ref[c][0])
            for a, b in zip(got[1:], ref[c][1:]):
                assert bool(((a - b).abs() <= 128 * 2.0 ** -24 * b.abs()).all()), float((a - b).abs().max())
        assert rel_err(got_eval[c][2].cpu().numpy(), data["ll"][c]) < LL_RTOL
    assert m._trainers == {}


def test_adam_loop_lowers_the_nll():
    """Ten torch.optim.Adam steps on case B (fixed batch and noise, seeded): the NLL ends below its start."""
    import torch
    from gbnf_amd import image_glow
    sp, x, noise = igo.make_case("B", 1)
    dev = torch.device("cuda:0")
    m = _module((1, 16, 16), 32, 2, 2, dev)
    image_glow.load_image_spec(m.flows[0], sp)
    m.train()
    xd, nd = torch.from_numpy(x).to(dev), torch.from_numpy(noise).to(dev)
    opt = torch.optim.Adam(m.parameters(), lr=1e-3)
    losses = []
    for _ in range(10):
        opt.zero_grad()
        loss = _nll(*m.component_forward(xd, 0, nd)[:4])
        loss.backward()
        torch.nn.utils.clip_grad_norm_(m.parameters(), 100.0)
        opt.step()
        losses.append(float(loss.detach()))
    assert np.isfinite(losses).all() and losses[-1] < losses[0], losses
    assert len(m._trainers) == 1            # the optimiser's in-place updates needed no new trainer


@pytest.mark.parametrize("name", igo.G21)
def test_module_matches_the_reference_gradients(name):
    """The g21 fixtures through BoostedFlow(args) in train mode: nll and every parameter's .grad (lower / upper / log_s included)
    against the reference's own."""
    import torch
    cfg, data = igo.g21_load(name)
    dev = torch.device("cuda:0")
    m = igo.g21_module(cfg, data, dev)
    m.train()
    z, z_mu, z_var, ldj, _ = m.component_forward(torch.from_numpy(data["x"]).to(dev), 0, torch.from_numpy(data["noise"]).to(dev))
    nll = _nll(z, z_mu, z_var, ldj)
    nll.backward()
    ez = float((z.detach().cpu() - torch.from_numpy(data["z"])).abs().max()) / float(np.abs(data["z"]).max())
    print(f"{name}: forward z {ez:.3e} of {Z_RTOL} against the reference's f32 z")
    assert ez <= Z_RTOL
    assert rel_err(ldj.detach().cpu().numpy(), data["ldj"]) < LL_RTOL
    assert abs(float(nll) - float(data["nll"])) <= LL_RTOL * abs(float(data["nll"]))
    ref = {k[len("grad."):]: data[k].astype(np.float64) for k in data.files if k.startswith("grad.")}
    got = {k: p.grad.reshape(ref[k].shape) for k, p in m.flows[0].named_parameters()}
    _check_grads(got, ref, name)
