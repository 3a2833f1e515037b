"""GPU: one image training step in one call -- gbnf_image_trainer_nll_step / _apply_update / _bind_lu / _bind_top
(csrc/gbnf_image_opt.hip), native.NativeImageTrainer's step methods and BoostedImageFlow.training_step -- against the float64
yardstick of the whole loss (tests/image_step_oracle.py), torch's own clip_grad_norm_ + torch.optim and the reference's gradients.

Tolerances are the project's own (tests/test_hip_image_train.py, tests/test_hip_fused_step.py): nll within 1e-5 relative; gradients
within G_RTOL = 2e-4 of each tensor's largest entry (floor 1e-3) AFTER dividing by loss_scale (a bits-per-dimension gradient is 1e-4 of
the nats one: the floor would swamp it); parameters and moments against torch.optim fed the same gradient within
PARAM_TOL = 1e-6 x max|tensor| (the update kernel is the tabular one: its derivation applies)."""
import ctypes as C
import functools
import math

import numpy as np
import pytest

import image_grad_oracle as igo
import image_step_oracle as iso
from test_hip_fused_step import LR, OPT_CASES, PARAM_TOL, STEP_SCALES, _assert_close, _regions, _torch_optimizer, _torch_step
from test_hip_image_train import G_RTOL, LL_RTOL, Z_RTOL, _check_grads, _module, _nll

pytestmark = pytest.mark.gpu


@functools.lru_cache(maxsize=None)
def _yardstick(name):
    """(spec, x, noise, nll, gradients at loss_scale 1) of a step case: computed once, shared, left unchanged."""
    sp, x, noise = iso.make_case(name)
    nll, g = iso.step_yardstick(sp, x, noise)
    return sp, x, noise, nll, g


def _per_dim(sp):
    return 1.0 / (math.log(2.0) * float(np.prod(sp["input_size"])))


def _trainer(sp, dev, lu=None):
    """NativeImageTrainer on device copies of the spec's arrays, learn_top and the LU factors of ``lu`` bound -> (trainer, {path: tensor})."""
    import torch
    from gbnf_amd import native
    ds, top = iso.dev_spec_top(sp, dev)
    tr = native.NativeImageTrainer(ds)
    for (l, k), f in (lu or {}).items():
        t = {key: torch.from_numpy(np.ascontiguousarray(f[key])).to(dev) for key in f}
        tr.bind_lu(l, k, t["p"], t["sign_s"], t["lower"], t["upper"], t["log_s"])
    if top is not None:
        tr.bind_top(top["w"], top["b"], top["logs"])
    tensors = {path: t for (path, _, _), t in zip(tr._step_regions, tr.params) if t is not None}
    return tr, tensors


def _dev(a, dev):
    import torch
    return torch.from_numpy(a).to(dev)


@pytest.mark.parametrize("bits", [False, True])
@pytest.mark.parametrize("name", sorted(iso.STEP_CASES))
def test_nll_step_with_zero_lr_matches_the_yardstick(name, bits):
    """1. loss and every gradient (perm_w with its log-det term, the top prior) at lr = 0; parameters bit-identical."""
    import torch
    from gbnf_amd import native
    sp, x, noise, nll, ref = _yardstick(name)
    dev = torch.device("cuda:0")
    tr, tensors = _trainer(sp, dev)
    k = _per_dim(sp) if bits else 1.0
    before = {p: t.clone() for p, t in tensors.items()}
    stats, flat = tr.nll_step(_dev(x, dev), _dev(noise, dev), native.OptState(tr, "adamw"), loss_scale=k, lr=0.0, weight_decay=1e-5,
                              max_grad_norm=50.0)
    stats = stats.cpu()
    print(f"{name} k={k:.3e}: nll {float(stats[0])} vs {nll}")
    assert abs(float(stats[0]) - nll) <= LL_RTOL * abs(nll)
    assert flat.numel() == tr.step_grad_floats
    _check_grads(tr.step_views(flat), ref, f"{name} k={k:.3e}", scale_by=k)
    for p, t in tensors.items():
        assert torch.equal(t, before[p]), p
    norm = float(flat.double().norm())
    assert abs(float(stats[1]) - norm) <= 1e-5 * norm
    assert float(stats[3]) == 0.0


def _lu_case(name):
    """Case ``name`` with every perm_w replaced by its float32 LU parameterisation -> (spec with the matrices the factors compose to, lu)."""
    import torch
    sp, x, noise, _, _ = _yardstick(name)
    sp = {**sp, "levels": [{**lv, "steps": [dict(st) for st in lv["steps"]]} for lv in sp["levels"]]}
    lu = {}
    for l, lv in enumerate(sp["levels"]):
        for k, st in enumerate(lv["steps"]):
            f = lu[(l, k)] = iso.lu_factor(st["perm_w"])
            st["perm_w"] = iso.lu_compose(*(torch.tensor(f[key], dtype=torch.float64) for key in ("p", "sign_s", "lower", "upper", "log_s"))
                                          ).numpy().astype(np.float32)
    return sp, x, noise, lu


@pytest.mark.parametrize("name", ["B", "D"])
def test_lu_factors_at_library_level(name):
    """2. bind_lu: gradients of lower / upper / log_s, the composed region zero, the forward that of the plain-weight trainer."""
    import torch
    from gbnf_amd import native
    sp, x, noise, lu = _lu_case(name)
    dev = torch.device("cuda:0")
    nll, ref = iso.step_yardstick(sp, x, noise, 1.0, lu)
    plain, _ = _trainer(sp, dev)
    tr, _ = _trainer({**sp, "levels": [{**lv, "steps": [{**st, "perm_w": np.zeros_like(st["perm_w"])} for st in lv["steps"]]}
                                       for lv in sp["levels"]]}, dev, lu)
    xd, nd = _dev(x, dev), _dev(noise, dev)
    stats, flat = tr.nll_step(xd, nd, native.OptState(tr, "sgd"), lr=0.0)
    stats_p, _ = plain.nll_step(xd, nd, native.OptState(plain, "sgd"), lr=0.0)
    views = tr.step_views(flat)
    composed = {p: v for p, v in views.items() if p[-1] == "perm_w"}
    assert len(composed) == len(lu) and all(float(v.abs().max()) == 0.0 for v in composed.values())
    _check_grads({p: v for p, v in views.items() if p[-1] != "perm_w"}, ref, f"LU {name}")
    assert abs(float(stats[0]) - nll) <= LL_RTOL * abs(nll)
    assert abs(float(stats[0]) - float(stats_p[0])) <= LL_RTOL * abs(float(stats_p[0]))
    z, zp = tr.forward(xd, nd)[0], plain.forward(xd, nd)[0]          # (the composed matrices are in the bound tensors now)
    assert float((z - zp).abs().max()) <= Z_RTOL * float(zp.abs().max())


@pytest.mark.parametrize("name", igo.G21)
def test_module_step_matches_the_reference_gradients(name):
    """3. The g21 fixtures through BoostedFlow(args).training_step at lr = 0: nll and every gradient by state_dict name."""
    import torch
    cfg, data = igo.g21_load(name)
    dev = torch.device("cuda:0")
    m = igo.g21_module(cfg, data, dev)
    m.train()
    before = {k: p.detach().clone() for k, p in m.flows[0].named_parameters()}
    out = m.training_step(_dev(data["x"], dev), noise=_dev(data["noise"], dev), lr=0.0, bits_per_dim=False, want_grads=True)
    assert abs(float(out["nll"]) - float(data["nll"])) <= LL_RTOL * abs(float(data["nll"]))
    assert abs(float(out["bpd"]) - float(data["nll"]) * _per_dim(cfg)) <= LL_RTOL * abs(float(data["nll"]) * _per_dim(cfg))
    ref = {k[len("grad."):]: data[k].astype(np.float64) for k in data.files if k.startswith("grad.")}
    _check_grads({k: v.reshape(ref[k].shape) for k, v in out["grads"].items()}, ref, name)
    assert all(p.grad is None and torch.equal(p, before[k]) for k, p in m.flows[0].named_parameters())


@pytest.mark.parametrize("case,with_lu", [(c, False) for c in sorted(OPT_CASES)] + [("adamw_wd_clip", True)])
def test_a_step_is_its_parts(case, with_lu):
    """4. Five consecutive nll_step calls on case B against a CPU torch.optim twin fed the gradients the calls returned."""
    import torch
    from gbnf_amd import native
    cfg = OPT_CASES[case]
    dev = torch.device("cuda:0")
    if with_lu:
        sp, x, noise, lu = _lu_case("B")
    else:
        (sp, x, noise, _, _), lu = _yardstick("B"), None
    tr, _ = _trainer(sp, dev, lu)
    xd, nd = _dev(x, dev), _dev(noise, dev)
    probe, _ = tr.nll_step(xd, nd, native.OptState(tr, "sgd"), lr=0.0)
    max_norm = 0.5 * float(probe[1]) if cfg["clip"] else 0.0          # the gradient scales with loss_scale: 1 and 2 clip, 0.3 and 0.1 do not
    regions = _regions(tr)
    live = [r for r in regions if r[2] is not None]
    clones = [t.detach().cpu().clone().requires_grad_(True) for _, _, t in live]
    opt = _torch_optimizer(clones, cfg["kind"], LR, cfg["weight_decay"])
    state = native.OptState(tr, cfg["kind"])
    coefs = []
    for it, k in enumerate(STEP_SCALES):
        stats, flat = tr.nll_step(xd, nd, state, loss_scale=k, lr=LR, weight_decay=cfg["weight_decay"], max_grad_norm=max_norm)
        stats = stats.cpu()
        norm, coef = _torch_step(opt, clones, regions, flat.cpu(), max_norm)
        assert abs(float(stats[1]) - norm) <= 1e-5 * norm, f"step {it}: norm {float(stats[1])} vs {norm}"
        assert abs(float(stats[2]) - coef) <= 1e-5, f"step {it}: coefficient {float(stats[2])} vs {coef}"
        coefs.append(coef)
    assert state.step == 5
    if cfg["clip"]:
        assert min(coefs) < 1.0 and max(coefs) == 1.0
    m_views, v_views = state.views()
    k = 0
    for idx, (off, size, t) in enumerate(regions):
        if t is None:
            assert with_lu and m_views[idx] is None
            continue
        _assert_close(t, clones[k], f"parameter {idx}")
        if cfg["kind"] == "adamw":
            _assert_close(m_views[idx], opt.state[clones[k]]["exp_avg"], f"exp_avg {idx}")
            _assert_close(v_views[idx], opt.state[clones[k]]["exp_avg_sq"], f"exp_avg_sq {idx}")
        k += 1
    assert with_lu == any(t is None for _, _, t in regions)


@pytest.mark.parametrize("name", ["g21_image_grads_lu", "g21_image_grads_invconv_affine"])
def test_fused_step_against_the_eager_path(name):
    """5. One SGD step with clipping: component_forward in train mode + the reference's loss + clip_grad_norm_ + optim.SGD.step() on
    one copy of the module, training_step on the other, same noise.  Per tensor |dp| <= 2 G_RTOL lr max|g| + PARAM_TOL max|p|: both
    gradients are within G_RTOL max|g| of the exact one."""
    import torch
    cfg, data = igo.g21_load(name)
    dev = torch.device("cuda:0")
    eager, fused = igo.g21_module(cfg, data, dev), igo.g21_module(cfg, data, dev)
    eager.train(); fused.train()
    xd, nd = _dev(data["x"], dev), _dev(data["noise"], dev)
    lr = 1e-2
    loss = _nll(*eager.component_forward(xd, 0, nd)[:4]) * _per_dim(cfg)
    loss.backward()
    params = list(eager.flows[0].parameters())
    max_norm = 0.5 * float(torch.linalg.vector_norm(torch.stack([torch.linalg.vector_norm(p.grad) for p in params])))
    torch.nn.utils.clip_grad_norm_(params, max_norm)
    torch.optim.SGD(params, lr=lr).step()
    out = fused.training_step(xd, noise=nd, lr=lr, optimizer="sgd", max_grad_norm=max_norm)
    assert abs(float(out["clip_coef"]) - 0.5) <= 1e-4
    loss = float(loss.detach())
    assert abs(float(out["nll"]) * _per_dim(cfg) - loss) <= LL_RTOL * abs(loss)
    state0 = {k[len("param."):]: data[k] for k in data.files if k.startswith("param.")}
    moved = 0
    for (nm, pe), (_, pf) in zip(eager.flows[0].named_parameters(), fused.flows[0].named_parameters()):
        g = float(pe.grad.abs().max())
        bound = 2 * G_RTOL * lr * g + PARAM_TOL * float(pe.detach().abs().max())
        assert float((pe.detach() - pf.detach()).abs().max()) <= bound, nm
        moved += int(not np.array_equal(pf.detach().cpu().numpy().reshape(-1), state0[nm].reshape(-1)))
    assert moved > len(state0) // 2          # the fused copy did step


def test_zero_lr_freezes_and_the_update_is_bit_identical():
    """6. lr = 0: parameters bit for bit, moments move.  Two runs of two apply_update calls on the same gradient buffer agree bit for
    bit (the backward's float atomics are not part of this: include/gbnf.h)."""
    import torch
    from gbnf_amd import native
    sp, x, noise, _, _ = _yardstick("B")
    dev = torch.device("cuda:0")
    tr, tensors = _trainer(sp, dev)
    before = {p: t.clone() for p, t in tensors.items()}
    state = native.OptState(tr, "adamw")
    _, flat = tr.nll_step(_dev(x, dev), _dev(noise, dev), state, lr=0.0, weight_decay=1e-5, max_grad_norm=0.5)
    assert all(torch.equal(t, before[p]) for p, t in tensors.items())
    assert float(state.exp_avg.abs().max()) > 0 and float(state.exp_avg_sq.max()) > 0
    runs = []
    for _ in range(2):
        tr2, tensors2 = _trainer(sp, dev)
        st2 = native.OptState(tr2, "adamw")
        stats = [tr2.apply_update(flat * s, st2, lr=LR, weight_decay=1e-5, max_grad_norm=0.5).clone() for s in (1.0, 0.5)]
        runs.append(([t.clone() for t in tensors2.values()], st2.exp_avg.clone(), st2.exp_avg_sq.clone(), stats))
    (pa, ma, va, sa), (pb, mb, vb, sb) = runs
    assert all(torch.equal(a, b) for a, b in zip(pa, pb)) and torch.equal(ma, mb) and torch.equal(va, vb)
    assert all(torch.equal(a, b) for a, b in zip(sa, sb))
    assert not all(torch.equal(a, before[p]) for a, p in zip(pa, tensors))


def test_module_behaviour():
    """7. Twenty steps lower the nll on one trainer object; the packed evaluation copy follows the update; n = 1; resuming from a
    torch.optim.AdamW gives torch's third step."""
    import torch
    from gbnf_amd import image_glow
    sp, x, noise, _, _ = _yardstick("B")
    dev = torch.device("cuda:0")
    m = _module((1, 16, 16), 32, 2, 2, dev)
    image_glow.load_image_spec(m.flows[0], sp)
    m.train()
    xd, nd = _dev(x, dev), _dev(noise, dev)
    # two eager AdamW steps, then the fused third from the optimiser's state
    params = list(m.flows[0].parameters())
    opt = torch.optim.AdamW(params, lr=LR, weight_decay=1e-5, foreach=False)
    for _ in range(2):
        opt.zero_grad()
        _nll(*m.component_forward(xd, 0, nd)[:4]).backward()
        opt.step()
    twins = [p.detach().cpu().clone().requires_grad_(True) for p in params]
    opt2 = torch.optim.AdamW(twins, lr=LR, weight_decay=1e-5, foreach=False)
    for p, q in zip(params, twins):
        opt2.state[q] = {k: (v.detach().cpu().clone() if isinstance(v, torch.Tensor) else v) for k, v in opt.state[p].items()}
    m.opt_state(0, "adamw").load_from(opt, m.step_parameters(0))
    assert m.opt_state(0).step == 2
    out = m.training_step(xd, noise=nd, lr=LR, weight_decay=1e-5, bits_per_dim=False, want_grads=True)
    for (nm, p), q in zip(m.flows[0].named_parameters(), twins):
        q.grad = out["grads"][nm].detach().cpu().reshape(q.shape).clone()
    opt2.step()
    for (nm, p), q in zip(m.flows[0].named_parameters(), twins):
        _assert_close(p, q, nm)
    assert m.opt_state(0).step == 3
    # a packed evaluation copy keyed on the parameters' versions as they are now: the steps below must invalidate it
    m.eval()
    lp_before = m.log_prob(xd, noise=nd).clone()
    packed = m.native_flow(0)
    m.train()
    # twenty steps
    trainer = m._trainers[0][1]
    nlls = [float(m.training_step(xd, noise=nd, lr=LR, max_grad_norm=50.0)["nll"]) for _ in range(20)]
    assert np.isfinite(nlls).all() and nlls[-1] < nlls[0], nlls
    assert m._trainers[0][1] is trainer and len(m._trainers) == 1
    one = m.training_step(xd[:1], noise=nd[:1], lr=LR)
    assert np.isfinite([float(one["nll"]), float(one["bpd"]), float(one["grad_norm"])]).all()
    # the packed evaluation copy was invalidated: log_prob is that of a fresh module with the same state_dict
    m.eval()
    fresh = _module((1, 16, 16), 32, 2, 2, dev)
    fresh.load_state_dict(m.state_dict())
    fresh.flows[0].set_actnorm_init()
    fresh.eval()
    a, b = m.log_prob(xd, noise=nd), fresh.log_prob(xd, noise=nd)
    assert m.native_flow(0) is not packed and float((a - lp_before).abs().max()) > 0.0
    assert bool(((a - b).abs() <= 128 * 2.0 ** -24 * b.abs()).all()), float((a - b).abs().max())      # (ldj: float atomics, test_hip_image_train)


def test_refusals():
    """8. GBNF_ERR_INVALID or a Python error with a reason."""
    import torch
    from gbnf_amd import native
    sp, x, noise, _, _ = _yardstick("C")
    dev = torch.device("cuda:0")
    tr, _ = _trainer(sp, dev)
    L = native.lib()
    xd = _dev(x, dev)
    n = x.shape[0]
    nb = C.c_int64()
    assert L.gbnf_image_trainer_step_workspace_bytes(tr.handle, n, C.byref(nb)) == 0
    ws = torch.empty(nb.value // 4 + 1, dtype=torch.float32, device=dev)
    flat = torch.zeros(tr.step_grad_floats, dtype=torch.float32, device=dev)
    stats = torch.zeros(4, dtype=torch.float32, device=dev)
    ptr = lambda t: C.c_void_p(t.data_ptr())
    sgd = native._OptHyper(kind=native.OPT_KIND["sgd"], step=1, lr=0.0)
    adamw = native._OptHyper(kind=native.OPT_KIND["adamw"], step=1, lr=0.0, beta1=0.9, beta2=0.999, eps=1e-8)
    args = lambda h, nbytes, n_=n: (tr.handle, ptr(xd), None, n_, 1.0, ptr(flat), None, None, C.byref(h), ptr(stats), ptr(ws), nbytes, None)
    assert L.gbnf_image_trainer_nll_step(*args(sgd, nb.value - 256)) == -1 and b"workspace" in L.gbnf_last_error()
    assert L.gbnf_image_trainer_nll_step(*args(adamw, nb.value)) == -1 and b"AdamW" in L.gbnf_last_error()
    assert L.gbnf_image_trainer_nll_step(*args(sgd, nb.value, 0)) == -1
    assert L.gbnf_image_trainer_apply_update(tr.handle, ptr(flat), None, None, C.byref(adamw), ptr(stats), None) == -1
    torch.cuda.synchronize()
    assert float(stats.abs().max()) == 0.0 and float(flat.abs().max()) == 0.0           # nothing was launched
    c = sp["levels"][0]["steps"][0]["an_bias"].shape[0]
    eye, ones = torch.eye(c, device=dev), torch.ones(c, device=dev)
    with pytest.raises(native.GbnfError, match="permutation"):                            # case C shuffles: no matrix to compose into
        tr.bind_lu(0, 0, eye, ones, eye.clone(), eye.clone(), ones.clone())
    with pytest.raises(native.GbnfError, match="outside"):
        L_ = native.lib()
        native._check(L_.gbnf_image_trainer_bind_lu(tr.handle, 5, 0, ptr(eye), ptr(ones), ptr(eye), ptr(eye), ptr(ones)))
    m = _module((1, 16, 16), 32, 2, 2, dev)
    m.train()
    xm = torch.rand(2, 1, 16, 16, device=dev)
    with pytest.raises(ValueError, match="ActNorm"):
        m.training_step(xm, lr=LR)
    m.flows[0].set_actnorm_init()
    with pytest.raises(NotImplementedError):
        m.training_step(xm.clone().requires_grad_(True), lr=LR)
