"""GPU: label-free evaluation of class-conditional image models -- gbnf_image_flow_forward_classes (img_ycond_table_kernel,
csrc/gbnf_image_ycond.hip), gbnf_class_posterior, gbnf_image_mixture_rho_step_y and the module's class_log_prob / marginal_log_prob /
class_posterior / predict / update_rho(labels=True) / graphed_log_prob(labels=True) -- against the float64 yardstick
(tests/image_class_table_cases.py), the kernel's closed form on the device's own z and ldj, gbnf_image_flow_forward_y, and the
reference's own component under every class (fixture g23).

Tolerances: the project's own (tests/test_hip_image_train.py): z within Z_RTOL of its largest entry, ldj / table within LL_RTOL relative
of float64.  ULP2 = 2.4e-7 relative is 2 float32 ulps: the table and what it is compared with at that bar are both double-precision sums
rounded once to float32, so at most 1 ulp apart, plus one ulp of margin.  The posterior: |delta| <= 2 LL_RTOL max_k |G_k| per image,
a difference of two numbers each good to LL_RTOL."""
import ctypes as C
import functools

import numpy as np
import pytest

import image_class_table_cases as ict
import image_ycond_oracle as iyo
import test_image_boost_host as host
from conftest import rel_err
from test_hip_image_train import LL_RTOL, Z_RTOL

pytestmark = pytest.mark.gpu
SENTINEL = -12345.0
ULP2 = 2.4e-7
NAMES = sorted(ict.CASES)


def _dev(a, dev):
    import torch
    return torch.from_numpy(np.ascontiguousarray(a)).to(dev)


def _cuda():
    import torch
    return torch.device("cuda:0")


def _classes_to_check(Y):
    return list(range(Y)) if Y <= 10 else sorted({0, 63, 64, Y - 1})


@functools.lru_cache(maxsize=None)
def _run(name, math):
    """One forward_classes call of a fresh handle on the case -> numpy (z, ldj, table, logits)."""
    import torch
    from gbnf_amd import native
    sp, x, noise, _ = ict.yardstick(name)
    dev = _cuda()
    flow = native.NativeImageFlow(sp, math=math)
    z, ldj, table, lg = flow.forward_classes(_dev(x, dev), _dev(noise, dev), want_z=True, want_logits=True)
    torch.cuda.synchronize()
    return tuple(t.cpu().numpy() for t in (z, ldj, table, lg))


# ---- 1. the table against float64 ----------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("math", ["f32", "default"])
@pytest.mark.parametrize("name", NAMES)
def test_table_matches_the_yardstick(name, math):
    sp, x, noise, out = ict.yardstick(name)
    z, ldj, table, lg = _run(name, math)
    n, Y, Cz, HW = ict.geometry(name)
    assert table.shape == (n, Y) and z.shape[:2] == (n, Cz) and z.shape[2] * z.shape[3] == HW
    ez = float(np.abs(z - out["z"]).max()) / float(np.abs(out["z"]).max())
    et, ed = rel_err(table, out["table"]), rel_err(ldj, out["ldj"])
    print(f"{name} {math}: z {ez:.3e} ldj {ed:.3e} table {et:.3e}")
    assert ez <= Z_RTOL and ed < LL_RTOL
    assert et < LL_RTOL
    if Y > 1:
        assert np.abs(table[:, 0] - table[:, 1]).min() > 0.0
    if math == "f32":
        assert float(np.abs(lg - out["y_logits"]).max()) <= 1e-5 * float(np.abs(out["y_logits"]).max())


# ---- 2. the kernel alone ---------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("math", ["f32", "default"])
@pytest.mark.parametrize("name", NAMES)
def test_table_kernel_against_its_closed_form(name, math):
    """The same call's z and ldj, read back, through the numpy float64 closed form with the prior the handle holds (its y-free part
    is float32(bias e^{3 logs}), gbnf_image_flow_create): whatever the flow did, the table kernel adds nothing beyond one rounding."""
    sp = ict.yardstick(name)[0]
    z, ldj, table, _ = _run(name, math)
    closed = ict.np_table(z, ldj, ict.class_priors(sp, ict.handle_top_h(sp)))
    err = float((np.abs(table - closed) / np.abs(closed)).max())
    print(f"{name} {math}: table against the closed form {err:.3e} (bar {ULP2:.1e})")
    assert np.isfinite(closed).all() and err <= ULP2


# ---- 3. consistency with forward_y -----------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("name", NAMES)
def test_table_agrees_with_forward_y(name):
    import torch
    from gbnf_amd import native
    sp, x, noise, _ = ict.yardstick(name)
    dev = _cuda()
    n, Y = x.shape[0], ict.geometry(name)[1]
    flow = native.NativeImageFlow(sp)
    flow.deterministic = True
    xd, nd = _dev(x, dev), _dev(noise, dev)
    z, ldj, table, lg = flow.forward_classes(xd, nd, want_z=True, want_logits=True)
    worst, equal = 0.0, 0
    for k in _classes_to_check(Y):
        y = torch.zeros((n, Y), device=dev)
        y[:, k] = 1.0
        z2, ldj2, ll, lg2 = flow.forward(xd, nd, y=y)
        assert torch.equal(z2, z) and torch.equal(ldj2, ldj) and torch.equal(lg2, lg), k
        a, b = table[:, k].double(), ll.double()
        worst = max(worst, float(((a - b).abs() / b.abs()).max()))
        equal += int(torch.equal(table[:, k], ll))
    print(f"{name}: table against forward_y {worst:.3e} (bar {ULP2:.1e}); bit-equal columns {equal} of {len(_classes_to_check(Y))}")
    assert worst <= ULP2


# ---- 4. determinism -------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("name", ["S70", "W", "g22"])
def test_table_is_deterministic(name):
    import torch
    from gbnf_amd import native
    sp, x, noise, _ = ict.yardstick(name)
    dev = _cuda()
    n = x.shape[0]
    flow = native.NativeImageFlow(sp)
    xd, nd = _dev(x, dev), _dev(noise, dev)
    z0 = flow.forward_classes(xd, nd, want_z=True)[0]
    z1 = flow.forward_classes(xd, nd, want_z=True)[0]
    assert torch.equal(z0, z1)                                # mode off: z is still bit-equal
    flow.deterministic = True
    a = flow.forward_classes(xd, nd, want_z=True, want_logits=True)
    b = flow.forward_classes(xd, nd, want_z=True, want_logits=True)
    for s, t in zip(a, b):
        assert torch.equal(s, t)
    rev = flow.forward_classes(xd.flip(0).contiguous(), nd.flip(0).contiguous())[2]
    assert torch.equal(rev.flip(0), a[2])
    for i in sorted({0, n // 2, n - 1}):
        alone = flow.forward_classes(xd[i:i + 1].contiguous(), nd[i:i + 1].contiguous())[2]
        assert torch.equal(alone[0], a[2][i]), i


# ---- 5. range repair -------------------------------------------------------------------------------------------------------------------
def test_forward_classes_repairs_an_out_of_range_image(monkeypatch):
    """The recipe of tests/test_hip_image_ycond.py::test_forward_y_repairs_an_out_of_range_image: the image is marked, the same call's
    repair launch re-evaluates it, and the table launch behind it reads the repaired z / ldj."""
    import copy
    import torch
    from gbnf_amd import native
    sp, x, noise, _ = ict.yardstick("g22")
    sp = copy.deepcopy(sp)
    net = sp["levels"][0]["steps"][1]["convs"]
    net[0]["an_logs"] = net[0]["an_logs"] + np.float32(12.0)
    net[-1]["w"] = (net[-1]["w"] * np.float32(np.exp(-12.0))).astype(np.float32)
    dev = _cuda()
    xd, nd = _dev(x[:1], dev), _dev(noise[:1], dev)
    exact = native.NativeImageFlow(sp, math="f32")
    t3 = exact.forward_classes(xd, nd)[2]
    monkeypatch.setenv("GBNF_IMAGE_NO_PROBE", "1")
    flow = native.NativeImageFlow(sp)
    assert native.MATH_NAME[int(flow.numerics().math_mode)] == "f16x3"
    before = flow.repair_counts()
    table = flow.forward_classes(xd, nd)[2]
    torch.cuda.synchronize()
    after = flow.repair_counts()
    assert after["marked_calls"] == before["marked_calls"] + 1 and after["repaired_images"] == before["repaired_images"] + 1
    assert bool(torch.isfinite(table).all()) and rel_err(table.cpu().numpy(), t3.cpu().numpy()) < LL_RTOL


# ---- 6. class_posterior ----------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("with_prior", [False, True])
@pytest.mark.parametrize("n,Y", [(1, 1), (3, 10), (70, 70), (2, 256)])
def test_class_posterior(n, Y, with_prior):
    import torch
    from gbnf_amd import native
    dev = _cuda()
    rng = np.random.RandomState(n * 1000 + Y)
    t = (rng.randn(n, Y) * 1e3).astype(np.float32)
    if Y > 1:
        t[0, Y // 2] = -np.inf                                # one impossible class
    if n > 1:
        t[n - 1] = -np.inf                                    # an impossible row
    lp = np.log(rng.dirichlet(np.ones(Y))).astype(np.float32) if with_prior else None
    lpx, post, pred = native.class_posterior(_dev(t, dev), None if lp is None else _dev(lp, dev), want_post=True, want_pred=True)
    torch.cuda.synchronize()
    lpx, post, pred = lpx.cpu().numpy(), post.cpu().numpy(), pred.cpu().numpy()
    rx, rp = ict.np_posterior(t, lp)
    np.testing.assert_allclose(lpx, rx, rtol=ULP2, atol=ULP2, equal_nan=True)
    np.testing.assert_allclose(post, rp, rtol=ULP2, atol=ULP2, equal_nan=True)
    assert pred.dtype == np.int32 and np.array_equal(pred, np.argmax(post, axis=1))
    finite = np.isfinite(rx)
    assert finite.sum() == (n - 1 if n > 1 else n)
    assert np.abs(np.exp(post[finite].astype(np.float64)).sum(axis=1) - 1.0).max() <= 1e-6
    if n > 1:
        assert lpx[n - 1] == -np.inf and np.isnan(post[n - 1]).all() and pred[n - 1] == 0
    # the outputs are optional, and log_px does not depend on which were asked for
    only = native.class_posterior(_dev(t, dev), None if lp is None else _dev(lp, dev), want_post=False, want_pred=True)
    assert only[1] is None and np.array_equal(only[0].cpu().numpy(), lpx, equal_nan=True) and np.array_equal(only[2].cpu().numpy(), pred)


# ---- 7. the module ---------------------------------------------------------------------------------------------------------------------
MODULE_SEEDS = (None, 5, 2)          # component 0: the reference's (fixture g22); the later ones synthetic


def _module(dev, C_=3, rho_lr=1e-5):
    """BoostedFlow of the g22 fixture's geometry with C_ class-conditional components, built like image_ycond_oracle.g22_module:
    component 0 carries the reference's state_dict, the later ones synthetic parameters."""
    import argparse
    import torch
    from gbnf_amd import BoostedFlow, image_glow, synth
    cfg, data = iyo.g22_load(iyo.G22[0])
    args = argparse.Namespace(
        num_flows=cfg["K"], z_size=int(np.prod(cfg["input_size"])), density_evaluation=True, device=dev, cuda=dev.type == "cuda",
        component_type="glow", num_components=C_, rho_init="decreasing", learn_top=cfg["learn_top"], y_classes=cfg["Y"], y_condition=True,
        sample_size=4, input_size=list(cfg["input_size"]), h_size=cfg["h"], num_blocks=cfg["L"], actnorm_scale=1.0,
        flow_permutation=cfg["permutation"], flow_coupling=cfg["coupling"], LU_decomposed=cfg["LU"], num_dequant_blocks=0,
        coupling_network="tanh", coupling_network_depth=cfg["depth"], batch_norm=False, boosted=True, rho_iters=12, rho_lr=rho_lr)
    torch.manual_seed(0)
    m = BoostedFlow(args)
    m.flows[0].load_state_dict({k[len("param."):]: torch.from_numpy(data[k]) for k in data.files if k.startswith("param.")})
    m.flows[0].set_actnorm_init()
    for c in range(1, C_):
        image_glow.load_image_spec(m.flows[c], synth.synth_image_glow_spec(tuple(cfg["input_size"]), h=cfg["h"], K=cfg["K"], L=cfg["L"],
                                                                          seed=MODULE_SEEDS[c], y_classes=cfg["Y"]))
    m.eval()
    return m, data


@functools.lru_cache(maxsize=None)
def _module_tables64():
    """(3, n, Y) float64 tables of the module's components on the fixture's x and noise: computed once on CPU copies of the parameters."""
    import torch
    from gbnf_amd import image_glow
    m, data = _module(torch.device("cpu"))
    Y, n = m.flows[0].y_classes, data["x"].shape[0]
    eye = np.eye(Y, dtype=np.float32)
    out = []
    with torch.no_grad():
        for c in range(3):
            sp = image_glow.image_spec_from_glow_module(m.flows[c])
            P = iyo.leaf_params(sp)
            out.append(np.stack([iyo.forward(sp, P, data["x"], data["noise"], np.repeat(eye[k:k + 1], n, axis=0))["ll"].numpy()
                                 for k in range(Y)], axis=1))
    return np.stack(out)


def test_module_class_log_prob():
    import torch
    from gbnf_amd import native
    dev = _cuda()
    m, data = _module(dev)
    m.image_eval_deterministic = True
    xd, nd, yd = _dev(data["x"], dev), _dev(data["noise"], dev), _dev(data["y"], dev)
    n, Y = yd.shape
    comp = m.component_class_log_prob(xd, noise=nd)
    assert tuple(comp.shape) == (n, 3, Y)
    G = m.class_log_prob(xd, noise=nd)
    assert tuple(G.shape) == (n, Y)
    for k in range(Y):                                       # column k: the recursion on that column alone, to the bit
        assert torch.equal(G[:, k], native.mixture_lse(comp[:, :, k].t().contiguous(), m.rho)), k
    # the row's own class: log_prob with the label
    ll = m.log_prob(xd, noise=nd, y_onehot=yd)
    own = G[torch.arange(n, device=dev), torch.argmax(yd, dim=1)]
    err = float(((own.double() - ll.double()).abs() / ll.double().abs()).max())
    print(f"class_log_prob at the labels against log_prob: {err:.3e} (bar {ULP2:.1e}), bit-equal: {bool(torch.equal(own, ll))}")
    assert err <= ULP2
    per = m.component_log_prob(xd, noise=nd, y_onehot=yd)
    own_c = comp[torch.arange(n, device=dev), :, torch.argmax(yd, dim=1)]
    assert float(((own_c.double() - per.double()).abs() / per.double().abs()).max()) <= ULP2
    # n_used
    G2 = m.class_log_prob(xd, n_used=2, noise=nd)
    assert torch.equal(G2[:, 0], native.mixture_lse(comp[:, :2, 0].t().contiguous(), m.rho)) and not torch.equal(G2, G)
    assert tuple(m.component_class_log_prob(xd, n_used=1, noise=nd).shape) == (n, 1, Y)
    assert torch.equal(m.class_log_prob(xd, n_used=1, noise=nd), comp[:, 0, :])


@pytest.mark.parametrize("with_prior", [False, True])
def test_module_marginal_and_posterior(with_prior):
    import torch
    dev = _cuda()
    m, data = _module(dev)
    xd, nd = _dev(data["x"], dev), _dev(data["noise"], dev)
    t64 = _module_tables64()
    n, Y = t64.shape[1:]
    prior = np.random.RandomState(3).dirichlet(np.ones(Y)).astype(np.float32) if with_prior else None
    kw = dict(noise=nd, class_prior=None if prior is None else _dev(prior, dev))
    G64 = ict.np_mixture(t64, m.rho.cpu().numpy())
    assert rel_err(m.class_log_prob(xd, noise=nd).cpu().numpy(), G64) < LL_RTOL
    lpx64, post64 = ict.np_posterior(G64, None if prior is None else np.log(prior.astype(np.float64)))
    bar = 2 * LL_RTOL * np.abs(G64).max(axis=1)
    lpx = m.marginal_log_prob(xd, **kw).cpu().numpy()
    post = m.class_posterior(xd, **kw)
    pred = m.predict(xd, **kw)
    print(f"marginal: worst {np.abs(lpx - lpx64).max():.3e}, posterior: worst {np.abs(post.cpu().numpy() - post64).max():.3e}, bar {bar.min():.3e}")
    assert lpx.shape == (n,) and (np.abs(lpx - lpx64) <= bar).all()
    assert tuple(post.shape) == (n, Y) and (np.abs(post.cpu().numpy() - post64) <= bar[:, None]).all()
    assert pred.dtype == torch.int64 and torch.equal(pred, torch.argmax(post, dim=1))
    lpx2 = m.marginal_log_prob(xd, n_used=2, **kw).cpu().numpy()
    lpx64_2 = ict.np_posterior(ict.np_mixture(t64[:2], m.rho.cpu().numpy()), None if prior is None else np.log(prior.astype(np.float64)))[0]
    assert (np.abs(lpx2 - lpx64_2) <= bar).all() and np.abs(lpx2 - lpx).max() > 0.0


# ---- 8. the rho update with y ----------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("component", [1, 2])
def test_rho_step_y_against_float64(component):
    """rho_step(y=) on 2 and 3 conditioned components against float64 arithmetic on the device's own table (the bounds of
    tests/test_hip_image_boost.py::test_rho_step_against_float64) and the table against forward_y."""
    import torch
    from gbnf_amd import native
    from test_hip_image_boost import RHO0, _expect_rho
    dev = _cuda()
    m, data = _module(dev)
    xd, nd, yd = _dev(data["x"], dev), _dev(data["noise"], dev), _dev(data["y"], dev)
    flows = [m.native_flow(c) for c in range(3)]
    n = xd.shape[0]
    t64 = _module_tables64()
    t = iyo.target(data["y"])
    ll64 = t64[:, np.arange(n), t][:component + 1]
    g64 = host.grad64(ll64, RHO0, component)
    step = 0.05 / abs(g64)
    rho = _dev(RHO0.copy(), dev)
    stats = native.NativeImageFlow.rho_step(flows, xd, nd, component, rho, step, y=yd).cpu().numpy()
    ll = flows[component].rho_ll.cpu().double().numpy()
    rho = rho.cpu().numpy()
    assert ll.shape == (component + 1, n) and (np.abs(ll - ll64) <= LL_RTOL * np.abs(ll64)).all()
    for c in range(component + 1):
        want = flows[c].forward(xd, nd, want_z=False, y=yd, want_logits=False)[2].cpu().double().numpy()
        assert (np.abs(ll[c] - want) <= LL_RTOL * np.abs(want)).all()
    fixed = host.fixed_ll64(ll, RHO0, component)
    g_dev = float(np.mean(fixed - ll[component]))
    bound = 1e-5 * max(np.abs(fixed).max(), np.abs(ll[component]).max())
    bound64 = 2e-5 * max(np.abs(host.fixed_ll64(ll64, RHO0, component)).max(), np.abs(ll64[component]).max())
    print(f"component {component}: grad {stats[0]} vs {g_dev} on the device table (bound {bound:.3e}), vs {g64} in float64 (bound {bound64:.3e})")
    assert abs(float(stats[0]) - g_dev) <= bound and abs(float(stats[0]) - g64) <= bound64
    want = _expect_rho(RHO0[component], step, stats[0])
    assert stats[1] == RHO0[component] and stats[2] == rho[component] and stats[3] == np.abs(stats[2] - stats[1])
    assert abs(float(rho[component]) - float(want)) <= float(np.spacing(want))
    assert 0.01 < rho[component] < 100.0 and rho[component] != RHO0[component], "the step was meant to move rho inside the clamp"
    others = [c for c in range(3) if c != component]
    assert (rho[others] == RHO0[others]).all()                # only rho[component] is written


def test_module_update_rho_with_labels():
    """update_rho(loader, labels=True) over 12 iterations against the float64 replay of the schedule on the yardstick's log-likelihoods
    of the same batches, noise and labels (the pattern and bound of test_module_update_rho_against_the_replay)."""
    import torch
    from gbnf_amd import image_glow, synth
    from test_hip_image_boost import RHO0, _Loader
    dev = _cuda()
    rho_lr = 1e-3
    m, data = _module(dev, rho_lr=rho_lr)
    m.component = 2
    size, Y = tuple(m.flows[0].input_size), int(m.flows[0].y_classes)
    xs = [synth.synth_image_batch(4, size, seed=s)[0] for s in (104, 105)]
    ys = [iyo.synth_y(4, Y, seed=s) for s in (4, 5)]
    loader = _Loader([(_dev(x, dev), _dev(y, dev)) for x, y in zip(xs, ys)])
    version = m.rho._version
    m.train()
    m.update_rho(loader, noise_generator=torch.Generator(device=dev).manual_seed(7), labels=True)
    assert not m.training
    g = torch.Generator(device=dev).manual_seed(7)
    noises = [torch.rand(xs[k % 2].shape, generator=g, device=dev).cpu().numpy() for k in range(12)]
    cpu, _ = _module(torch.device("cpu"))
    specs = [image_glow.image_spec_from_glow_module(cpu.flows[c]) for c in range(3)]
    leaves = [iyo.leaf_params(sp) for sp in specs]
    with torch.no_grad():
        tables = [np.stack([iyo.forward(sp, P, xs[k % 2], noises[k], ys[k % 2])["ll"].numpy() for sp, P in zip(specs, leaves)])
                  for k in range(12)]
    r = host.replay_update_rho(tables, RHO0, 2, rho_lr, 12)
    print(f"replay: rho {r['rho']} after {r['iters']} iterations, grads {r['grads'][:3]}, difs {r['difs'][-1]}")
    assert r["difs"][11] >= 2 * host.TOLERANCE or r["difs"][11] <= 0.5 * host.TOLERANCE, "the stop rule could flip on rounding"
    assert 0.01 < r["rho"] < 100.0 and all(0.01 < v < 100.0 for v in r["rhos"]), "the replay was meant to stay inside the clamp"
    assert loader.served == r["iters"] == 12
    rho = m.rho.cpu().numpy()
    worst = max(np.abs(t).max() for t in tables)
    moved = abs(r["rho"] - float(RHO0[2]))
    bound = sum(r["steps"]) * 2e-5 * worst + r["iters"] * float(np.spacing(np.float32(max(r["rhos"] + [float(RHO0[2])]))))
    print(f"module: rho[2] {rho[2]} vs {r['rho']} (bound {bound:.3e}, moved {moved:.3e})")
    assert moved > 10 * bound, "the replay was meant to move rho by much more than the bound"
    assert abs(float(rho[2]) - r["rho"]) <= bound
    assert (rho[:2] == RHO0[:2]).all() and m.rho._version > version
    with pytest.raises(ValueError, match="y_onehot"):         # a loader without labels
        m.update_rho([(_dev(xs[0], dev), None)], labels=True)


# ---- 9. the graph -------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("det", [True, False])
def test_graphed_log_prob_with_labels(det):
    import torch
    from gbnf_amd import native, synth
    dev = _cuda()
    m, data = _module(dev, C_=2)
    m.image_eval_deterministic = det
    size, Y = tuple(m.flows[0].input_size), int(m.flows[0].y_classes)
    x, noise = synth.synth_image_batch(4, size, seed=104)
    xd, nd = _dev(x, dev), _dev(noise, dev)
    y1, y2 = _dev(iyo.synth_y(4, Y, seed=4), dev), _dev(np.roll(iyo.synth_y(4, Y, seed=4), 1, axis=1), dev)
    f = m.graphed_log_prob(4, labels=True)

    def same(a, b):
        return torch.equal(a, b) if det else rel_err(a.cpu().numpy(), b.cpu().numpy()) < LL_RTOL

    g1 = f(xd, nd, y1).clone()
    assert tuple(g1.shape) == (4,) and same(g1, m.log_prob(xd, noise=nd, y_onehot=y1))
    g2 = f(xd, nd, y2).clone()                                # another y, the same graph
    assert same(g2, m.log_prob(xd, noise=nd, y_onehot=y2)) and float((g2 - g1).abs().min()) > 0.0
    assert same(f(xd, nd, y1), g1)
    with torch.no_grad():                                     # a parameter changes: f re-captures by itself
        m.flows[1].project_ycond.linear.bias.mul_(1.5)
    g3 = f(xd, nd, y1).clone()
    assert same(g3, m.log_prob(xd, noise=nd, y_onehot=y1)) and float((g3 - g1).abs().max()) > 0.0
    with pytest.raises(ValueError, match="y_onehot"):
        f(xd, nd)
    with pytest.raises(native.GbnfError):
        f(xd[:2], nd[:2], y1[:2])


# ---- 10. refusals at the C boundary -----------------------------------------------------------------------------------------------------
def test_refusals():
    """Each refused with nothing launched: sentinel-filled outputs stay untouched."""
    import torch
    from gbnf_amd import native, synth
    sp, x, noise, _ = ict.yardstick("g22")
    dev = _cuda()
    L = native.lib()
    n, Y = x.shape[0], 10
    xd, nd = _dev(x, dev), _dev(noise, dev)
    yd = _dev(iyo.synth_y(n, Y, 1), dev)
    ptr = lambda t: C.c_void_p(t.data_ptr()) if t is not None else C.c_void_p(0)
    plain_spec = {k_: v for k_, v in sp.items() if k_ != "ycond"}
    flow, plain = native.NativeImageFlow(sp, math="f32"), native.NativeImageFlow(plain_spec, math="f32")
    bare = native.NativeImageFlow({**sp, "ycond": {**sp["ycond"], "class_w": None}}, math="f32")
    other = native.NativeImageFlow(synth.synth_image_glow_spec((1, 16, 16), h=32, K=2, L=2, seed=5, y_classes=Y + 1), math="f32")
    nb, nbp = C.c_int64(), C.c_int64()
    assert L.gbnf_image_flow_workspace_bytes(flow.handle, n, C.byref(nb)) == 0 and L.gbnf_image_flow_workspace_bytes(plain.handle, n, C.byref(nbp)) == 0
    ws = torch.empty(nb.value // 4 + 1, dtype=torch.float32, device=dev)
    outs = {"z": torch.full((n,) + flow.z_shape, SENTINEL, device=dev), "ldj": torch.full((n,), SENTINEL, device=dev),
            "table": torch.full((n, Y), SENTINEL, device=dev), "lg": torch.full((n, Y), SENTINEL, device=dev)}

    def fc(h, x_=xd, ldj=outs["ldj"], table=outs["table"], lg=None, w=ws, bytes_=None):
        return L.gbnf_image_flow_forward_classes(h, ptr(x_), ptr(nd), n, ptr(outs["z"]), ptr(ldj), ptr(table), ptr(lg), ptr(w),
                                                 nb.value if bytes_ is None else bytes_, None)

    assert fc(plain.handle) == -1 and b"conditioning" in L.gbnf_last_error()               # a plain handle
    assert fc(flow.handle, x_=None) == -1 and fc(flow.handle, ldj=None) == -1 and fc(flow.handle, table=None) == -1
    assert fc(flow.handle, w=None) == -1 and b"null" in L.gbnf_last_error()
    assert fc(flow.handle, bytes_=nbp.value) == -1 and b"workspace" in L.gbnf_last_error()  # a workspace sized for the plain call
    assert fc(bare.handle, lg=outs["lg"]) == -1 and b"class head" in L.gbnf_last_error()    # logits without a head
    assert L.gbnf_image_flow_forward_classes(flow.handle, None, None, 0, None, None, None, None, None, 0, None) == 0     # n = 0
    # the rho update with y
    rb = C.c_int64()
    trio = lambda a, b: (C.c_void_p * 2)(a.handle.value, b.handle.value)
    assert L.gbnf_image_rho_step_workspace_bytes(trio(flow, other), 2, n, C.byref(rb)) == 0
    rws = torch.empty(rb.value // 4 + 1, dtype=torch.float32, device=dev)
    rho, table, rstats = (torch.full(sh, SENTINEL, device=dev) for sh in ((2,), (2, n), (4,)))

    def ry(handles, y_=yd):
        return L.gbnf_image_mixture_rho_step_y(handles, 1, ptr(xd), ptr(nd), ptr(y_), n, ptr(rho), 0.1, ptr(table), ptr(rstats), ptr(rws),
                                               rb.value, None)

    assert ry(trio(flow, plain)) == -1 and b"conditioning" in L.gbnf_last_error()           # a plain handle among the flows
    assert ry(trio(plain, flow)) == -1
    assert ry(trio(flow, other)) == -1 and b"classes" in L.gbnf_last_error()                # two class counts
    assert ry(trio(flow, flow), y_=None) == -1 and b"null" in L.gbnf_last_error()           # a null y
    assert L.gbnf_image_mixture_rho_step(trio(flow, flow), 1, ptr(xd), ptr(nd), n, ptr(rho), 0.1, ptr(table), ptr(rstats), ptr(rws), rb.value,
                                         None) == -1 and b"needs y" in L.gbnf_last_error()  # the plain call keeps refusing
    # class_posterior
    cl = torch.full((n, Y), 1.0, device=dev)
    px, post = torch.full((n,), SENTINEL, device=dev), torch.full((n, Y), SENTINEL, device=dev)
    pred = torch.full((n,), -7, dtype=torch.int32, device=dev)
    cp = lambda Y_, a=cl, b=px: L.gbnf_class_posterior(ptr(a), None, n, Y_, ptr(b), ptr(post), ptr(pred), None)
    assert cp(0) == -1 and cp(257) == -2 and cp(Y, a=None) == -1 and cp(Y, b=None) == -1
    assert L.gbnf_class_posterior(None, None, 0, Y, None, None, None, None) == 0
    torch.cuda.synchronize()
    for t in list(outs.values()) + [rho, table, rstats, px, post]:
        assert bool((t == SENTINEL).all())
    assert bool((pred == -7).all())
    # ... and the same calls with nothing wrong go through
    assert fc(flow.handle, lg=outs["lg"]) == 0 and cp(Y) == 0
    rho.fill_(0.5)
    assert ry(trio(flow, flow)) == 0
    torch.cuda.synchronize()
    for t in (outs["table"], outs["lg"], table, rstats, px, post):
        assert not bool((t == SENTINEL).any())
    assert float(px[0]) == 1.0 and bool((pred == 0).all())    # Y equal classes under the uniform prior: log_px = the common value


# ---- 11. the reference anchor ---------------------------------------------------------------------------------------------------------------
def test_component_class_log_prob_matches_the_reference():
    """Fixture g23: the reference's own class-conditional component run once per class on g22's parameters, x and noise."""
    dev = _cuda()
    cfg, data = iyo.g22_load(iyo.G22[0])
    m = iyo.g22_module(cfg, data, dev)
    m.eval()
    ref = ict.g23_load()
    got = m.component_class_log_prob(_dev(data["x"], dev), noise=_dev(data["noise"], dev))
    assert tuple(got.shape) == (ref.shape[0], 1, ref.shape[1])
    err = rel_err(got[:, 0, :].cpu().numpy(), ref)
    print(f"component_class_log_prob against the reference: {err:.3e}")
    assert err < LL_RTOL
