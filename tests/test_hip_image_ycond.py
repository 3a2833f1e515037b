"""GPU: class-conditional image Glow -- gbnf_image_flow_set_ycond / _forward_y / _prior_y, gbnf_image_trainer_bind_ycond /
_nll_step_y, gbnf_image_boosted_nll_step_y (csrc/gbnf_image_ycond.hip) and the module's y_onehot paths -- against the float64
yardstick (tests/image_ycond_oracle.py) and the reference's own class-conditional component (fixtures g22).

Tolerances are the project's own (tests/test_hip_image_train.py, tests/test_hip_fused_step.py): z within Z_RTOL of its largest entry,
ldj / ll / nll within LL_RTOL relative, gradients within G_RTOL of each tensor's largest entry (floor 1e-3) after dividing by
loss_scale, parameters within PARAM_TOL.  The logits of an exact-f32 handle: 1e-5 of the yardstick's largest logit; of a default
(split-f16) handle: within exp(3 lk_j) sum_c |Wk[j,c]| Z_RTOL max|z| of the f32 handle's -- what the z bar allows a mean of z to move."""
import ctypes as C
import functools
import math

import numpy as np
import pytest

import image_step_oracle as iso
import image_ycond_oracle as iyo
from conftest import rel_err
from test_hip_fused_step import LR, PARAM_TOL, _assert_close
from test_hip_inverse import X_BAR
from test_hip_image_train import G_RTOL, LL_RTOL, Z_RTOL, _check_grads, _nll

pytestmark = pytest.mark.gpu
SENTINEL = -12345.0


@functools.lru_cache(maxsize=None)
def _yardstick(name):
    """(spec, x, noise, y, out, gradients at loss_scale 1 and y_weight 1): computed once, shared, left unchanged."""
    sp, x, noise, y = iyo.make_case(name)
    out, g = iyo.yardstick(sp, x, noise, y, k=1.0, y_weight=1.0)
    return sp, x, noise, y, out, g


@functools.lru_cache(maxsize=None)
def _yardstick_at(name, k, yw):
    sp, x, noise, y = iyo.make_case(name)
    return iyo.yardstick(sp, x, noise, y, k=k, y_weight=yw)


def _per_dim(sp):
    return 1.0 / (math.log(2.0) * float(np.prod(sp["input_size"])))


def _dev(a, dev):
    import torch
    return torch.from_numpy(np.ascontiguousarray(a)).to(dev)


def _trainer(sp, dev, deterministic=False, ycond=None):
    """NativeImageTrainer on device copies of the spec's arrays with learn_top and the conditioning bound -> (trainer, {path: tensor})."""
    from gbnf_amd import native
    ds, top = iso.dev_spec_top(sp, dev)
    tr = native.NativeImageTrainer(ds, deterministic=deterministic)
    if top is not None:
        tr.bind_top(top["w"], top["b"], top["logs"])
    tr.bind_ycond(*(ycond if ycond is not None else iyo.dev_ycond(sp, dev)))
    return tr, {path: t for (path, _, _), t in zip(tr._step_regions, tr.params) if t is not None}


def _logit_bound(sp, z):
    yc = sp["ycond"]
    return np.exp(3.0 * yc["class_logs"].astype(np.float64)) * np.abs(yc["class_w"].astype(np.float64)).sum(axis=1) * Z_RTOL * float(np.abs(z).max())


# ---- 1. forward_y ---------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("name", sorted(iyo.YC_CASES))
def test_forward_y_matches_the_yardstick(name):
    import torch
    from gbnf_amd import native
    sp, x, noise, y, out, _ = _yardstick(name)
    dev = torch.device("cuda:0")
    xd, nd, yd = _dev(x, dev), _dev(noise, dev), _dev(y, dev)
    exact = native.NativeImageFlow(sp, math="f32")
    assert exact.y_classes == y.shape[1] and exact.has_class_head
    z, ldj, ll, lg = exact.forward(xd, nd, y=yd)
    zr, lgr = out["z"].numpy(), out["y_logits"].numpy()
    ez = float(np.abs(z.cpu().numpy() - zr).max()) / float(np.abs(zr).max())
    el, ed = rel_err(ll.cpu().numpy(), out["ll"].numpy()), rel_err(ldj.cpu().numpy(), out["ldj"].numpy())
    eg = float(np.abs(lg.cpu().numpy() - lgr).max()) / float(np.abs(lgr).max())
    print(f"{name}: f32 z {ez:.3e} ll {el:.3e} ldj {ed:.3e} logits {eg:.3e}")
    assert ez <= Z_RTOL and el < LL_RTOL and ed < LL_RTOL and eg <= 1e-5
    flow = native.NativeImageFlow(sp)
    z2, ldj2, ll2, lg2 = flow.forward(xd, nd, y=yd)
    assert float((z2 - z).abs().max()) <= Z_RTOL * float(z.abs().max())
    assert rel_err(ll2.cpu().numpy(), out["ll"].numpy()) < LL_RTOL and rel_err(ldj2.cpu().numpy(), out["ldj"].numpy()) < LL_RTOL
    diff = np.abs(lg2.double().cpu().numpy() - lg.double().cpu().numpy()).max(axis=0)
    bound = _logit_bound(sp, zr)
    print(f"{name}: default-handle logits {float((diff / bound).max()):.3e} of the bound")
    assert (diff <= bound).all()
    # ll moves with y as the yardstick says
    if y.shape[1] > 1:
        y2 = np.roll(y, 1, axis=1)
        with torch.no_grad():
            ref2 = iyo.forward(sp, iyo.leaf_params(sp), x, noise, y2)["ll"].numpy()
        ll3 = flow.forward(xd, nd, y=_dev(y2, dev), want_z=False)[2]
        assert rel_err(ll3.cpu().numpy(), ref2) < LL_RTOL and np.abs(ref2 - out["ll"].numpy()).min() > 0.0
        assert float((ll3 - ll2).abs().min()) > 0.0
    # a NULL class head: no logits, the same ll
    bare = native.NativeImageFlow({**sp, "ycond": {**sp["ycond"], "class_w": None}}, math="f32")
    assert not bare.has_class_head
    z4, ldj4, ll4, lg4 = bare.forward(xd, nd, y=yd)
    assert lg4 is None and rel_err(ll4.cpu().numpy(), ll.cpu().numpy()) < 1e-6 and torch.equal(z4, z)
    with pytest.raises(native.GbnfError, match="class head"):
        bare.forward(xd, nd, y=yd, want_logits=True)


@pytest.mark.parametrize("name", iyo.G22)
def test_module_forward_matches_the_reference(name):
    """The g22 fixtures through BoostedFlow(args) in eval mode: (z, z_mu, z_var, ldj, y_logits) and component_log_prob."""
    import torch
    cfg, data = iyo.g22_load(name)
    dev = torch.device("cuda:0")
    m = iyo.g22_module(cfg, data, dev)
    m.eval()
    xd, nd, yd = _dev(data["x"], dev), _dev(data["noise"], dev), _dev(data["y"], dev)
    z, mu, var, ldj, lg = m.component_forward(xd, 0, nd, y_onehot=yd)
    assert len(m(x=xd, y_onehot=yd, components=0)) == 5          # (the drop-in signature; it draws its own noise)
    assert tuple(mu.shape) == tuple(z.shape) == data["z"].shape and mu.stride()[2:] == (0, 0)
    assert float(np.abs(z.cpu().numpy() - data["z"]).max()) <= Z_RTOL * float(np.abs(data["z"]).max())
    assert rel_err(ldj.cpu().numpy(), data["ldj"]) < LL_RTOL
    for got, key in ((mu, "z_mu"), (var, "z_var")):
        assert float(np.abs(got.cpu().numpy() - data[key]).max()) <= 1e-6 * max(1.0, float(np.abs(data[key]).max())), key
    sp_lg = np.abs(data["y_logits"]).max()
    glow = m.flows[0]
    bound = (np.exp(3.0 * data["param.project_class.logs"].astype(np.float64)) * np.abs(data["param.project_class.linear.weight"]).sum(axis=1)
             * Z_RTOL * float(np.abs(data["z"]).max()) + 1e-5 * sp_lg)
    assert (np.abs(lg.cpu().numpy() - data["y_logits"]).max(axis=0) <= bound).all()
    ll = m.component_log_prob(xd, 1, nd, y_onehot=yd)[:, 0]
    assert abs(float(-ll.double().mean()) - float(data["nll"])) <= LL_RTOL * abs(float(data["nll"]))
    with pytest.raises(ValueError, match="y_onehot"):
        m.component_forward(xd, 0, nd)
    assert glow.y_condition


# ---- 2. range repair -------------------------------------------------------------------------------------------------------------
def test_forward_y_repairs_an_out_of_range_image(monkeypatch):
    """tools/stress_image.py's recipe (the first convolution's ActNorm2d scales the hidden activation by e^12, the last convolution's
    weights shrink by the same factor) with the create-time probe off: the image is marked, the repair launch of the same call
    re-evaluates it, and the launch behind it computes ll and the logits from the repaired z / ldj."""
    import copy
    import torch
    from gbnf_amd import native
    sp, x, noise, y, _, _ = _yardstick("g22")
    sp = copy.deepcopy(sp)
    net = sp["levels"][0]["steps"][1]["convs"]
    net[0]["an_logs"] = net[0]["an_logs"] + np.float32(12.0)
    net[-1]["w"] = (net[-1]["w"] * np.float32(np.exp(-12.0))).astype(np.float32)
    dev = torch.device("cuda:0")
    xd, nd, yd = _dev(x[:1], dev), _dev(noise[:1], dev), _dev(y[:1], dev)
    exact = native.NativeImageFlow(sp, math="f32")
    z3, ldj3, ll3, lg3 = exact.forward(xd, nd, y=yd)
    monkeypatch.setenv("GBNF_IMAGE_NO_PROBE", "1")
    flow = native.NativeImageFlow(sp)
    assert native.MATH_NAME[int(flow.numerics().math_mode)] == "f16x3"
    before = flow.repair_counts()
    z, ldj, ll, lg = flow.forward(xd, nd, y=yd)
    torch.cuda.synchronize()
    after = flow.repair_counts()
    assert after["marked_calls"] == before["marked_calls"] + 1 and after["repaired_images"] == before["repaired_images"] + 1
    assert torch.isfinite(ll).all() and rel_err(ll.cpu().numpy(), ll3.cpu().numpy()) < LL_RTOL
    diff = np.abs(lg.double().cpu().numpy() - lg3.double().cpu().numpy()).max(axis=0)
    bound = _logit_bound(sp, z3.cpu().numpy())
    print(f"repaired image: logits {float((diff / bound).max()):.3e} of the bound")
    assert (diff <= bound).all()


# ---- 3. nll_step_y at lr = 0 -----------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("bits", [False, True])
@pytest.mark.parametrize("name", sorted(iyo.YC_CASES))
def test_nll_step_y_with_zero_lr_matches_the_yardstick(name, bits):
    import torch
    from gbnf_amd import native
    sp, x, noise, y, _, _ = _yardstick(name)
    k = _per_dim(sp) if bits else 1.0
    yw = 0.01 if bits else 0.5
    out, ref = _yardstick_at(name, k, yw)
    dev = torch.device("cuda:0")
    tr, tensors = _trainer(sp, dev)
    assert tr.y_classes == y.shape[1]
    before = {p: t.clone() for p, t in tensors.items()}
    stats, flat = tr.nll_step(_dev(x, dev), _dev(noise, dev), native.OptState(tr, "adamw"), loss_scale=k, y=_dev(y, dev), y_weight=yw,
                              lr=0.0, weight_decay=1e-5, max_grad_norm=50.0)
    stats = stats.cpu()
    assert stats.numel() == 8
    print(f"{name} k={k:.3e}: nll {float(stats[0])} vs {out['nll']}, ce {float(stats[4])} vs {out['loss_classes']}, correct {float(stats[5])}")
    assert abs(float(stats[0]) - out["nll"]) <= LL_RTOL * abs(out["nll"])
    assert abs(float(stats[4]) - out["loss_classes"]) <= 1e-5 * max(abs(out["loss_classes"]), 1e-30) or (out["loss_classes"] == 0.0 and float(stats[4]) == 0.0)
    assert float(stats[5]) == float(out["correct"])
    assert float(stats[3]) == 0.0 and float(stats[6]) == 0.0 and float(stats[7]) == 0.0
    # the class regions scale with y_weight, everything else with loss_scale: compare each at its own scale
    views = tr.step_views(flat)
    head = {p for p in ref if p[0] == "ycond" and p[1].startswith("class")}
    _check_grads({p: v for p, v in views.items() if p not in head}, {p: g / k for p, g in ref.items() if p not in head}, f"{name} k={k:.3e}",
                 scale_by=k)
    _check_grads({p: views[p] for p in head}, {p: ref[p] / yw for p in head}, f"{name} head", scale_by=yw)
    for p, t in tensors.items():
        assert torch.equal(t, before[p]), p
    norm = float(np.sqrt(sum(float((g ** 2).sum()) for g in ref.values())))
    assert abs(float(stats[1]) - norm) <= 1e-5 * norm


# ---- 4. y_weight = 0 ---------------------------------------------------------------------------------------------------------------
def test_zero_y_weight_leaves_the_class_head_out():
    import torch
    from gbnf_amd import native
    sp, x, noise, y, _, _ = _yardstick("g22")
    dev = torch.device("cuda:0")
    xd, nd, yd = _dev(x, dev), _dev(noise, dev), _dev(y, dev)
    flats = []
    for change in (False, True):
        yc = iyo.dev_ycond(sp, dev)
        if change:
            for t in yc[3:]:
                t.mul_(-1.7).add_(0.05)
        tr, _ = _trainer(sp, dev, deterministic=True, ycond=yc)
        _, flat = tr.nll_step(xd, nd, native.OptState(tr, "sgd"), y=yd, y_weight=0.0, lr=0.0)
        flats.append(tr.step_views(flat))
    for key in ("class_w", "class_b", "class_logs"):
        assert float(flats[0][("ycond", key)].abs().max()) == 0.0 and float(flats[1][("ycond", key)].abs().max()) == 0.0
    for p in flats[0]:
        if not (p[0] == "ycond" and p[1].startswith("class")):
            assert torch.equal(flats[0][p], flats[1][p]), p
    assert float(flats[0][("ycond", "cond_w")].abs().max()) > 0.0


# ---- 5. determinism ------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("det", [True, False])
def test_step_y_is_reproducible(det):
    import torch
    from gbnf_amd import native
    sp, x, noise, y, _, _ = _yardstick("S70")
    dev = torch.device("cuda:0")
    xd, nd, yd = _dev(x, dev), _dev(noise, dev), _dev(y, dev)
    runs = []
    for _ in range(2):
        tr, tensors = _trainer(sp, dev, deterministic=det)
        st = native.OptState(tr, "adamw")
        stats, flat = tr.nll_step(xd, nd, st, loss_scale=_per_dim(sp), y=yd, y_weight=0.01, lr=1e-3, weight_decay=1e-5, max_grad_norm=5.0)
        runs.append((stats.clone(), flat.clone(), tr.step_views(flat), [t.clone() for t in tensors.values()], st.exp_avg.clone(), st.exp_avg_sq.clone()))
    a, b = runs
    for key in iyo.YCOND_KEYS:                              # the new regions: ordered sums in and out of deterministic mode
        assert torch.equal(a[2][("ycond", key)], b[2][("ycond", key)]), key
    assert torch.equal(a[0][4:6], b[0][4:6])
    if det:
        assert torch.equal(a[0], b[0]) and torch.equal(a[1], b[1]) and torch.equal(a[4], b[4]) and torch.equal(a[5], b[5])
        assert all(torch.equal(p, q) for p, q in zip(a[3], b[3]))


# ---- 6. the module's step against autograd ---------------------------------------------------------------------------------------
@pytest.mark.parametrize("name", iyo.G22)
def test_module_step_matches_the_reference(name):
    """training_step(lr = 0) of the g22 fixtures: nll, class loss and every gradient by state_dict name (the reference's f32 autograd of
    bpd + 0.01 cross_entropy)."""
    import torch
    cfg, data = iyo.g22_load(name)
    dev = torch.device("cuda:0")
    m = iyo.g22_module(cfg, data, dev)
    m.train()
    out = m.training_step(_dev(data["x"], dev), noise=_dev(data["noise"], dev), y_onehot=_dev(data["y"], dev), y_weight=cfg["y_weight"], lr=0.0,
                          want_grads=True)
    assert abs(float(out["nll"]) - float(data["nll"])) <= LL_RTOL * abs(float(data["nll"]))
    print(f"{name}: nll {float(out['nll'])} vs {float(data['nll'])}, class loss {float(out['loss_classes'])} vs {float(data['loss_classes'])}")
    assert abs(float(out["loss_classes"]) - float(data["loss_classes"])) <= 1e-5 * abs(float(data["loss_classes"]))
    t = np.argmax(data["y"], axis=1)
    assert float(out["class_correct"]) == float((np.argmax(data["y_logits"], axis=1) == t).sum())
    k, yw = _per_dim(cfg), cfg["y_weight"]
    ref = {n[len("grad."):]: data[n].astype(np.float64) for n in data.files if n.startswith("grad.")}
    head = {n for n in ref if n.startswith("project_class")}
    got = {n: v.reshape(ref[n].shape) for n, v in out["grads"].items()}
    _check_grads({n: v for n, v in got.items() if n not in head}, {n: g / k for n, g in ref.items() if n not in head}, name, scale_by=k)
    _check_grads({n: got[n] for n in head}, {n: ref[n] / yw for n in head}, name + " head", scale_by=yw)


@pytest.mark.parametrize("name", [iyo.G22[0], iyo.G22[1]])
def test_fused_step_y_against_the_eager_path(name):
    """One SGD step with clipping: component_forward in train mode + the reference's loss + clip_grad_norm_ + optim.SGD.step() on one
    copy of the module, training_step on the other (the pattern and bound of tests/test_hip_image_fused_step.py)."""
    import torch
    cfg, data = iyo.g22_load(name)
    dev = torch.device("cuda:0")
    eager, fused = iyo.g22_module(cfg, data, dev), iyo.g22_module(cfg, data, dev)
    eager.train(); fused.train()
    xd, nd, yd = _dev(data["x"], dev), _dev(data["noise"], dev), _dev(data["y"], dev)
    lr, yw = 1e-2, 0.3
    z, mu, var, ldj, lg = eager.component_forward(xd, 0, nd, y_onehot=yd)
    assert lg.requires_grad and mu.requires_grad
    ce = torch.nn.functional.cross_entropy(lg, torch.argmax(yd, dim=1))
    loss = _nll(z, mu, var, ldj) * _per_dim(cfg) + yw * ce
    loss.backward()
    params = list(eager.flows[0].parameters())
    assert all(p.grad is not None for n, p in eager.flows[0].named_parameters() if n.startswith("project_"))
    max_norm = 0.5 * float(torch.linalg.vector_norm(torch.stack([torch.linalg.vector_norm(p.grad) for p in params])))
    torch.nn.utils.clip_grad_norm_(params, max_norm)
    torch.optim.SGD(params, lr=lr).step()
    out = fused.training_step(xd, noise=nd, y_onehot=yd, y_weight=yw, lr=lr, optimizer="sgd", max_grad_norm=max_norm)
    assert abs(float(out["clip_coef"]) - 0.5) <= 1e-4
    assert abs(float(out["loss_classes"]) - float(ce)) <= 1e-5 * abs(float(ce))
    moved = 0
    for (nm, pe), (_, pf) in zip(eager.flows[0].named_parameters(), fused.flows[0].named_parameters()):
        g = float(pe.grad.abs().max())
        bound = 2 * G_RTOL * lr * g + PARAM_TOL * float(pe.detach().abs().max())
        assert float((pe.detach() - pf.detach()).abs().max()) <= bound, nm
        moved += int(not np.array_equal(pf.detach().cpu().numpy().reshape(-1), data["param." + nm].reshape(-1)))
    assert moved > len(params) // 2
    for nm in iyo.YCOND_NAMES.values():                      # all six new tensors stepped
        assert not np.array_equal(dict(fused.flows[0].named_parameters())[nm].detach().cpu().numpy(), data["param." + nm]), nm


@pytest.mark.parametrize("name", iyo.G22)
def test_module_adamw_step_against_torch(name):
    """The pattern and bound of test_module_behaviour in tests/test_hip_image_fused_step.py on a class-conditional module: two eager
    steps of torch.optim.AdamW on the module's own autograd path (component_forward in train mode, nll + y_weight cross_entropy),
    then training_step(y_onehot=) takes the third from the optimiser's state.  Fed the fused call's gradient, torch's third step gives
    the same parameters, exp_avg and exp_avg_sq within PARAM_TOL of each tensor's largest entry -- all six project_* tensors among
    them, so moments, weight decay, bias correction and the offsets of the new regions behind the top prior's are all in it."""
    import torch
    cfg, data = iyo.g22_load(name)
    dev = torch.device("cuda:0")
    m = iyo.g22_module(cfg, data, dev)
    m.train()
    xd, nd, yd = _dev(data["x"], dev), _dev(data["noise"], dev), _dev(data["y"], dev)
    yw, wd = 0.3, 1e-5
    glow = m.flows[0]
    params = list(glow.parameters())
    opt = torch.optim.AdamW(params, lr=LR, weight_decay=wd, foreach=False)
    for _ in range(2):
        opt.zero_grad()
        z, mu, var, ldj, lg = m.component_forward(xd, 0, nd, y_onehot=yd)
        (_nll(z, mu, var, ldj) + yw * torch.nn.functional.cross_entropy(lg, torch.argmax(yd, dim=1))).backward()
        opt.step()
    new = set(iyo.YCOND_NAMES.values())
    for nm, p in glow.named_parameters():
        if nm in new:                                        # the eager path reached all six: their moments are not zero
            assert float(opt.state[p]["exp_avg"].abs().max()) > 0.0 and float(opt.state[p]["exp_avg_sq"].max()) > 0.0, nm
    twins = [p.detach().cpu().clone().requires_grad_(True) for p in params]
    opt2 = torch.optim.AdamW(twins, lr=LR, weight_decay=wd, foreach=False)
    for p, q in zip(params, twins):
        opt2.state[q] = {k: (v.detach().cpu().clone() if isinstance(v, torch.Tensor) else v) for k, v in opt.state[p].items()}
    m.opt_state(0, "adamw").load_from(opt, m.step_parameters(0))
    assert m.opt_state(0).step == 2
    before = {nm: p.detach().clone() for nm, p in glow.named_parameters()}
    out = m.training_step(xd, noise=nd, y_onehot=yd, y_weight=yw, lr=LR, weight_decay=wd, bits_per_dim=False, want_grads=True)
    assert m.opt_state(0).step == 3 and new <= set(out["grads"])
    for (nm, p), q in zip(glow.named_parameters(), twins):
        q.grad = out["grads"][nm].detach().cpu().reshape(q.shape).clone()
    opt2.step()
    twin_of = {id(p): q for p, q in zip(params, twins)}
    name_of = {id(p): nm for nm, p in glow.named_parameters()}
    for (nm, p), q in zip(glow.named_parameters(), twins):
        _assert_close(p, q, nm)
    seen = set()
    for p, ea, eas in zip(m.step_parameters(0), *m.opt_state(0).views()):
        if p is None:
            continue
        nm, q = name_of[id(p)], twin_of[id(p)]
        _assert_close(ea, opt2.state[q]["exp_avg"], nm + " exp_avg")
        _assert_close(eas, opt2.state[q]["exp_avg_sq"], nm + " exp_avg_sq")
        seen.add(nm)
    assert new <= seen
    for nm in new:                                           # ... and the step moved each of them
        assert not torch.equal(dict(glow.named_parameters())[nm].detach(), before[nm]), nm


# ---- 7. the boosted step --------------------------------------------------------------------------------------------------------------
def test_boosted_step_y():
    import torch
    from gbnf_amd import native
    sp, x, noise, y, _, _ = _yardstick("g22")
    dev = torch.device("cuda:0")
    xd, nd, yd = _dev(x, dev), _dev(noise, dev), _dev(y, dev)
    from gbnf_amd import synth
    fixed = native.NativeImageFlow(synth.synth_image_glow_spec((1, 16, 16), h=32, K=2, L=2, seed=5, y_classes=y.shape[1]), math="f32")
    ll_fixed = fixed.forward(xd, nd, y=yd, want_z=False)[2]
    floor = float(ll_fixed.sort().values[1]) + 1e-3          # one row above the floor, two below it
    tr, tensors = _trainer(sp, dev, deterministic=True)
    tr2, tensors2 = _trainer(sp, dev, deterministic=True)
    start = {p: t.clone() for p, t in tensors.items()}
    st, st2 = native.OptState(tr, "adamw"), native.OptState(tr2, "adamw")
    hyper = dict(loss_scale=_per_dim(sp), y=yd, y_weight=0.01, lr=1e-3, weight_decay=1e-5, max_grad_norm=5.0)
    stats, flat = tr.boosted_nll_step(fixed, xd, nd, st, g_floor=floor, **hyper)
    stats2, flat2 = tr2.nll_step(xd, nd, st2, **hyper)
    assert stats.numel() == 12
    G = float(-(torch.clamp(ll_fixed.double(), min=floor)).mean())
    assert abs(float(stats[8]) - G) <= LL_RTOL * abs(G)
    assert float(stats[9]) == float(np.float32(stats[0].item()) - np.float32(stats[8].item()))
    assert float(stats[10]) == float((ll_fixed < np.float32(floor)).sum()) == 2.0 and float(stats[11]) == 0.0
    assert torch.equal(stats[:8], stats2) and torch.equal(flat, flat2)
    # ... and so do the update and the optimiser state (both trainers are in deterministic mode: bit for bit)
    assert tensors.keys() == tensors2.keys() and st.step == st2.step == 1
    for p, t in tensors.items():
        assert torch.equal(t, tensors2[p]), p
    assert torch.equal(st.exp_avg, st2.exp_avg) and torch.equal(st.exp_avg_sq, st2.exp_avg_sq)
    assert float(st.exp_avg.abs().max()) > 0.0 and sum(int(not torch.equal(t, start[p])) for p, t in tensors.items()) > len(tensors) // 2
    # a plain call on conditioned handles, and a conditioned call on a plain fixed component: refused
    with pytest.raises(native.GbnfError):
        tr.boosted_nll_step(fixed, xd, nd, native.OptState(tr, "adamw"), lr=0.0)
    plain = native.NativeImageFlow({k_: v for k_, v in sp.items() if k_ != "ycond"}, math="f32")
    with pytest.raises(native.GbnfError):
        tr.boosted_nll_step(plain, xd, nd, native.OptState(tr, "adamw"), y=yd, lr=0.0)


# ---- 8. sampling -------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("name", ["g22", "G", "S1"])
def test_prior_y(name):
    import torch
    from gbnf_amd import native
    sp, x, noise, y, out, _ = _yardstick(name)
    dev = torch.device("cuda:0")
    flow = native.NativeImageFlow(sp, math="f32")
    yd = _dev(y, dev)
    e = torch.randn((y.shape[0],) + flow.z_shape, device=dev, generator=torch.Generator(dev).manual_seed(3))
    mu, lv, z = flow.prior_y(yd, e, 0.7)
    for got, ref in ((mu, out["z_mu"].numpy()), (lv, out["z_var"].numpy())):
        scale = max(float(np.abs(out["z_mu"].numpy()).max()), float(np.abs(out["z_var"].numpy()).max()))
        assert float(np.abs(got.cpu().numpy() - ref).max()) <= 1e-6 * scale
    cz = flow.z_shape[0]
    want = mu.view(-1, cz, 1, 1) + torch.exp(lv.view(-1, cz, 1, 1)) * 0.7 * e
    assert float((z - want).abs().max()) <= 4 * 2.0 ** -23 * float(want.abs().max())
    mu2, lv2, none = flow.prior_y(yd)
    assert none is None and torch.equal(mu2, mu) and torch.equal(lv2, lv)


def test_module_decode_and_round_trip():
    """decode(z=None, y_onehot=eye(Y)): Y finite images in [0,1], and z comes back when a decoded image is encoded with the same y.

    The model is one for which [0,1] FOLLOWS: the reference's decode ends in x = ((2 sigmoid(v) - 1) / 0.9 + 1) / 2 (models/glow.py:
    154-161), which lies in [0,1] exactly when |v| <= log(19) = 2.94 and in (-0.056, 1.056) otherwise (its comments assume the former).
    An ADDITIVE-coupling model fresh from the constructor is, after set_actnorm_init, squeezes and ORTHOGONAL 1x1 matrices (the QR
    factor) around identity couplings (Conv2dZeros starts at zero) and zero-mean unit Split2d priors, so a pixel's channel vector keeps its 2-norm through every step: |v| <= sqrt(8) times the
    largest latent entry (8 = the widest level).  With project_ycond at a quarter of the fixture's values (|mu|, |lv| < 0.4),
    temperature 0.1 and draws cut at 3 sigma, every latent entry is below 0.4 + 0.3 e^0.4 = 0.85 in the worst case of every sign at
    once: |v| < 2.4."""
    import argparse
    import torch
    from gbnf_amd import BoostedFlow
    cfg, data = iyo.g22_load(iyo.G22[0])
    dev = torch.device("cuda:0")
    Y, T = cfg["Y"], 0.1
    m = BoostedFlow(argparse.Namespace(
        num_flows=cfg["K"], z_size=256, density_evaluation=True, device=dev, cuda=True, component_type="glow", num_components=1,
        rho_init="decreasing", learn_top=True, y_classes=Y, y_condition=True, sample_size=4, input_size=[1, 16, 16], h_size=cfg["h"],
        num_blocks=cfg["L"], actnorm_scale=1.0, flow_permutation="invconv", flow_coupling="additive", LU_decomposed=False,
        num_dequant_blocks=0, coupling_network="tanh", coupling_network_depth=1, batch_norm=False))
    glow = m.flows[0]
    with torch.no_grad():
        for nm in ("project_ycond.linear.weight", "project_ycond.linear.bias", "project_ycond.logs"):
            dict(glow.named_parameters())[nm].copy_(0.25 * _dev(data["param." + nm], dev))
    glow.set_actnorm_init()
    m.eval()
    eye = torch.eye(Y, device=dev)
    handle = m.native_flow(0)
    mu, lv, _ = handle.prior_y(eye)
    assert float(mu.abs().max()) < 0.4 and float(lv.abs().max()) < 0.4 and float(mu.abs().max()) > 0.0
    gen = torch.Generator(dev).manual_seed(5)
    e = torch.randn((Y,) + handle.z_shape, device=dev, generator=gen).clamp_(-3.0, 3.0)
    eps = [torch.randn((Y,) + sh, device=dev, generator=gen).clamp_(-3.0, 3.0) for sh in handle.split_shapes()]
    xs = m.decode(None, y_onehot=eye, temperature=T, components=0, eps=eps, e=e)
    print(f"decoded images: min {float(xs.min())}, max {float(xs.max())}")
    assert tuple(xs.shape) == (Y, 1, 16, 16) and bool(torch.isfinite(xs).all())
    assert float(xs.min()) >= 0.0 and float(xs.max()) <= 1.0
    assert float((xs[0] - xs[1]).abs().max()) > 0.0                      # the class moves the image
    assert tuple(m(z=None, y_onehot=eye, temperature=T, components=0, reverse=True).shape) == (Y, 1, 16, 16)
    # encode the decoded images with the same y (noise = x: (255 x + x) / 256 == x): z comes back at the bar tests/test_hip_inverse.py
    # holds a device inverse to, X_BAR (2e-5) of max(1, max|z|) -- also Z_RTOL, the bar of the image forward.  Attainable here: every
    # pixel lies in (0.035, 0.965) (|v| < 2.4), where the forward direction's v = logit(s), s = 0.05 + 0.9 x, multiplies the f32 rounding
    # of x (2^-24) by at most 0.9 / (s (1 - s)) = 12, i.e. 7e-7 in v; the orthogonal steps keep a pixel's 2-norm, so at most
    # sqrt(8) * 7e-7 = 2e-6 reaches an entry of z, beside the two directions' own f32 error.
    z0 = handle.prior_y(eye, e, T, want_prior=False)[2]
    assert bool(((xs > 0.035) & (xs < 0.965)).all())
    zb = m.component_forward(xs, 0, xs.clone(), y_onehot=eye)[0]
    err, scale = float((zb - z0).abs().max()), max(1.0, float(z0.abs().max()))
    print(f"round trip: max|z_back - z| {err:.3e}, bar {X_BAR * scale:.3e}")
    assert err <= X_BAR * scale


def test_module_sample_equals_decode():
    """sample(y_onehot=) equals per-component decode on the same draws; both stay inside the range of the reference's decode."""
    import torch
    cfg, data = iyo.g22_load(iyo.G22[0])
    dev = torch.device("cuda:0")
    m = iyo.g22_module(cfg, data, dev)
    m.eval()
    Y = cfg["Y"]
    eye = torch.eye(Y, device=dev)
    handle = m.native_flow(0)
    gen = torch.Generator(dev).manual_seed(5)
    e = torch.randn((Y,) + handle.z_shape, device=dev, generator=gen)
    eps = [torch.randn((Y,) + sh, device=dev, generator=gen) for sh in handle.split_shapes()]
    xs = m.decode(None, y_onehot=eye, temperature=0.7, components=0, eps=eps, e=e)
    half = 0.5 / 0.9
    assert bool(torch.isfinite(xs).all()) and float(xs.min()) > 0.5 - half - 1e-6 and float(xs.max()) < 0.5 + half + 1e-6
    # (one component: every row is component 0's)
    got, comp = m.sample(temperature=0.7, e=e, eps=eps, uniforms=torch.rand(Y, device=dev, generator=gen), y_onehot=eye, return_components=True)
    assert int(comp.abs().max()) == 0 and torch.equal(got, xs)
    with pytest.raises(ValueError, match="y_onehot"):
        m.sample(4)
    with pytest.raises(ValueError, match="y_onehot"):
        m.decode(None, components=0)


# ---- 9. refusals --------------------------------------------------------------------------------------------------------------------------
def test_refusals():
    """Each refused with nothing launched: sentinel-filled outputs stay untouched."""
    import torch
    from gbnf_amd import native
    sp, x, noise, y, _, _ = _yardstick("g22")
    dev = torch.device("cuda:0")
    L = native.lib()
    n, Y = x.shape[0], y.shape[1]
    xd, nd, yd = _dev(x, dev), _dev(noise, dev), _dev(y, dev)
    ptr = lambda t: C.c_void_p(t.data_ptr()) if t is not None else C.c_void_p(0)
    plain_spec = {k_: v for k_, v in sp.items() if k_ != "ycond"}
    flow, plain = native.NativeImageFlow(sp, math="f32"), native.NativeImageFlow(plain_spec, math="f32")
    nb, nbp = C.c_int64(), C.c_int64()
    assert L.gbnf_image_flow_workspace_bytes(flow.handle, n, C.byref(nb)) == 0 and L.gbnf_image_flow_workspace_bytes(plain.handle, n, C.byref(nbp)) == 0
    assert nb.value > nbp.value
    ws = torch.empty(nb.value // 4 + 1, dtype=torch.float32, device=dev)
    outs = {"z": torch.full((n,) + flow.z_shape, SENTINEL, device=dev), "ldj": torch.full((n,), SENTINEL, device=dev),
            "ll": torch.full((n,), SENTINEL, device=dev), "lg": torch.full((n, Y), SENTINEL, device=dev)}
    fy = lambda h, yy, bytes_=None: L.gbnf_image_flow_forward_y(h, ptr(xd), ptr(nd), ptr(yy), n, ptr(outs["z"]), ptr(outs["ldj"]), ptr(outs["ll"]),
                                                                ptr(outs["lg"]), ptr(ws), nb.value if bytes_ is None else bytes_, None)
    assert fy(flow.handle, None) == -1 and b"y" in L.gbnf_last_error()                       # a null y
    assert fy(plain.handle, yd) == -1 and b"conditioning" in L.gbnf_last_error()            # forward_y on an unconditioned handle
    assert fy(flow.handle, yd, nbp.value) == -1 and b"workspace" in L.gbnf_last_error()     # a workspace sized for the plain call
    assert L.gbnf_image_flow_forward(flow.handle, ptr(xd), ptr(nd), n, ptr(outs["z"]), ptr(outs["ldj"]), ptr(outs["ll"]), ptr(ws), nb.value,
                                     None) == -1 and b"needs y" in L.gbnf_last_error()      # the plain forward on a conditioned handle
    host = (C.c_float * 64)()
    assert L.gbnf_image_flow_prior(flow.handle, host) == -1 and b"needs y" in L.gbnf_last_error()
    assert L.gbnf_image_flow_prior_y(flow.handle, None, n, None, 1.0, ptr(outs["lg"]), None, None) == -1
    yc = [np.ascontiguousarray(sp["ycond"][key]) for key in iyo.YCOND_KEYS]
    hp = [a.ctypes.data_as(C.c_void_p) for a in yc]
    for bad in (0, 257):                                                                        # Y of 0 or 257
        assert L.gbnf_image_flow_set_ycond(plain.handle, bad, *hp) in (-1, -2)
    assert L.gbnf_image_flow_set_ycond(plain.handle, 257, *hp) == -2
    yv = C.c_int32(-1)
    assert L.gbnf_image_flow_y_classes(plain.handle, C.byref(yv)) == 0 and yv.value == 0
    # the trainer
    ds, top = iso.dev_spec_top(sp, dev)
    tr = native.NativeImageTrainer(ds)
    tr.bind_top(top["w"], top["b"], top["logs"])
    sb = C.c_int64()
    assert L.gbnf_image_trainer_step_workspace_bytes(tr.handle, n, C.byref(sb)) == 0
    before_bytes = sb.value
    dyc = iyo.dev_ycond(sp, dev)
    for bad in (0, 257):
        assert L.gbnf_image_trainer_bind_ycond(tr.handle, bad, *[ptr(t) for t in dyc]) in (-1, -2)
    assert tr.step_grad_floats == tr._off + 2 * 16 + 16 * 16 * 9          # (nothing was bound by the refused calls)
    sgd = native._OptHyper(kind=native.OPT_KIND["sgd"], step=1, lr=0.0)
    flat = torch.full((tr.step_grad_floats + 4096,), SENTINEL, device=dev)
    stats = torch.full((8,), SENTINEL, device=dev)
    wst = torch.empty(before_bytes // 4 + 64, dtype=torch.float32, device=dev)
    step_y = lambda yy, bytes_: L.gbnf_image_trainer_nll_step_y(tr.handle, ptr(xd), ptr(nd), ptr(yy), n, 1.0, 0.01, ptr(flat), None, None,
                                                                 C.byref(sgd), ptr(stats), ptr(wst), bytes_, None)
    assert step_y(yd, before_bytes) == -1 and b"conditioning" in L.gbnf_last_error()        # nll_step_y on an unconditioned trainer
    tr.bind_ycond(*dyc)
    assert L.gbnf_image_trainer_step_workspace_bytes(tr.handle, n, C.byref(sb)) == 0 and sb.value > before_bytes
    assert step_y(yd, before_bytes) == -1 and b"workspace" in L.gbnf_last_error()           # a workspace sized before binding
    wst = torch.empty(sb.value // 4 + 64, dtype=torch.float32, device=dev)
    assert step_y(None, sb.value) == -1 and b"y is null" in L.gbnf_last_error()              # a null y
    assert L.gbnf_image_trainer_nll_step(tr.handle, ptr(xd), ptr(nd), n, 1.0, ptr(flat), None, None, C.byref(sgd), ptr(stats), ptr(wst),
                                         sb.value, None) == -1 and b"needs y" in L.gbnf_last_error()
    # the rho update over a mixture whose SECOND handle is conditioned: refused before the first component's launches
    handles = (C.c_void_p * 2)(plain.handle.value, flow.handle.value)
    rb = C.c_int64()
    assert L.gbnf_image_rho_step_workspace_bytes(handles, 2, n, C.byref(rb)) == 0
    rws = torch.empty(rb.value // 4 + 1, dtype=torch.float32, device=dev)
    rho, table, rstats = (torch.full(sh, SENTINEL, device=dev) for sh in ((2,), (2, n), (4,)))
    assert L.gbnf_image_mixture_rho_step(handles, 1, ptr(xd), ptr(nd), n, ptr(rho), 0.1, ptr(table), ptr(rstats), ptr(rws), rb.value,
                                         None) == -1 and b"needs y" in L.gbnf_last_error()
    torch.cuda.synchronize()
    for t in list(outs.values()) + [flat, stats, rho, table, rstats]:
        assert bool((t == SENTINEL).all())
    # ... and the same calls with nothing wrong go through
    assert fy(flow.handle, yd) == 0 and step_y(yd, sb.value) == 0
    torch.cuda.synchronize()
    assert not bool((outs["ll"] == SENTINEL).any()) and not bool((stats == SENTINEL).any())
