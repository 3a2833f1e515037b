"""GPU: the fused training step -- gbnf_trainer_apply_update / gbnf_trainer_nll_step (csrc/gbnf_opt.hip), native.OptState and
BoostedFlow.training_step -- against torch's own clip_grad_norm_ + torch.optim.AdamW / SGD and the reference's gradients.

The parameter bound PARAM_TOL = 1e-6 x max|tensor|: the straight f32 AdamW formula with an f64 gradient norm differs from
torch.optim.AdamW by 7.5e-8 of max|p| after 5 steps (CPU torch); 1e-6 leaves ~13x for the order of operations."""
import ctypes as C

import numpy as np
import pytest

from conftest import GRADS_CASES, load_grads_case, load_train_bn_case
from test_hip_train import G_RTOL, _args, _dev_spec

pytestmark = pytest.mark.gpu
PARAM_TOL = 1e-6

GEOMETRIES = {
    "glow_d6_h30_K2": ("glow", 6, 30, 2, {}),
    "glow_d43_h215_K5": ("glow", 43, 215, 5, {}),                      # 3e5 entries: multi-workgroup reductions
    "realnvp_d21_h32_K3_bn": ("realnvp", 21, 32, 3, {}),               # BatchNorm on every step but the last
    "realnvp_d6_h30_K2_nobn": ("realnvp", 6, 30, 2, {"batch_norm": False}),      # reserved regions
}
OPT_CASES = {
    "adamw_wd_clip": dict(kind="adamw", weight_decay=1e-5, clip=True),
    "adamw_noclip": dict(kind="adamw", weight_decay=0.0, clip=False),
    "sgd_wd_clip": dict(kind="sgd", weight_decay=1e-3, clip=True),
}
LR = 1e-3
STEP_SCALES = (1.0, 0.3, 2.0, 0.1, 1.0)      # overall scale of the 5 gradients: with the median norm as the limit some steps clip


def _trainer(geometry, dev, seed=3, math="f16x3"):
    from gbnf_amd import native, synth
    kind, d, h, K, kw = GEOMETRIES[geometry] if isinstance(geometry, str) else geometry
    spec = synth.synth_boosted_specs(kind, 1, d, h, K, seed=seed, **kw)[0]
    return native.NativeTrainer(_dev_spec(spec, dev), math=math)


def _regions(tr):
    """(offset, size, tensor | None) per region of the flat layout."""
    out, off = [], 0
    for t, size in zip(tr.params, tr._sizes):
        out.append((off, size, t))
        off += size
    return out


def _random_grads(tr, dev, seed):
    """5 flat gradients: every region with its own scale in 1e-4 .. 1, reserved regions zero."""
    import torch
    g = torch.Generator().manual_seed(seed)
    base = torch.zeros(tr.grad_floats)
    for off, size, t in _regions(tr):
        if t is not None:
            base[off:off + size] = torch.randn(size, generator=g) * 10.0 ** (-4.0 * float(torch.rand((), generator=g)))
    flats = [(base * s * (1.0 + 0.1 * torch.randn(tr.grad_floats, generator=g)) * (base != 0)).contiguous() for s in STEP_SCALES]
    return flats


def _torch_optimizer(clones, kind, lr, weight_decay):
    import torch
    if kind == "adamw":
        return torch.optim.AdamW(clones, lr=lr, weight_decay=weight_decay, foreach=False)
    return torch.optim.SGD(clones, lr=lr, weight_decay=weight_decay, foreach=False)


def _torch_step(opt, clones, regions, flat_cpu, max_norm):
    """clip_grad_norm_ + opt.step() on CPU clones fed views of the flat gradient -> (norm, coefficient)."""
    import torch
    live = [r for r in regions if r[2] is not None]
    for p, (off, size, t) in zip(clones, live):
        p.grad = flat_cpu[off:off + size].view(p.shape).clone()
    if max_norm > 0:
        norm = float(torch.nn.utils.clip_grad_norm_(clones, max_norm, foreach=False))
        coef = min(1.0, max_norm / (norm + 1e-6))
    else:
        norm = float(torch.linalg.vector_norm(torch.stack([torch.linalg.vector_norm(p.grad) for p in clones])))
        coef = 1.0
    opt.step()
    return norm, coef


def _assert_close(mine, ref, what, tol=PARAM_TOL):
    mine, ref = mine.detach().cpu().double().reshape(-1), ref.detach().cpu().double().reshape(-1)
    scale = float(ref.abs().max())
    err = float((mine - ref).abs().max())
    assert err <= tol * scale, f"{what}: {err:.3e} > {tol} x {scale:.3e}"


def _check_flat_grads(flat, ref_flat, tr, what, floor=1e-3):
    """The rule of test_hip_train._check_grads on a flat buffer: G_RTOL of each tensor's largest entry, same floor."""
    flat = flat.detach().cpu().numpy()
    for k, (off, size, t) in enumerate(_regions(tr)):
        a, b = flat[off:off + size], np.asarray(ref_flat[off:off + size])
        if t is None:
            assert not a.any(), f"{what}: reserved region {k} is not zero"
            continue
        scale = max(float(np.abs(b).max()), floor)
        assert np.abs(a - b).max() <= G_RTOL * scale, f"{what}: gradient {k} ({size}): {np.abs(a - b).max()} vs scale {scale}"


@pytest.mark.parametrize("case", sorted(OPT_CASES))
@pytest.mark.parametrize("geometry", sorted(GEOMETRIES))
def test_update_matches_torch_optimizer(geometry, case):
    """1. Five consecutive apply_update calls against clip_grad_norm_ + torch.optim on a clone, same gradients."""
    import torch
    from gbnf_amd import native
    dev = torch.device("cuda:0")
    cfg = OPT_CASES[case]
    tr = _trainer(geometry, dev)
    regions = _regions(tr)
    live = [r for r in regions if r[2] is not None]
    flats = _random_grads(tr, dev, seed=11)
    norms = sorted(float(f.double().norm()) for f in flats)
    max_norm = norms[2] if cfg["clip"] else 0.0
    clones = [t.detach().cpu().clone().requires_grad_(True) for _, _, t in live]
    opt = _torch_optimizer(clones, cfg["kind"], LR, cfg["weight_decay"])
    state = native.OptState(tr, cfg["kind"])
    coefs = []
    for it, flat in enumerate(flats):
        stats = tr.apply_update(flat.to(dev), state, lr=LR, weight_decay=cfg["weight_decay"], max_grad_norm=max_norm).cpu()
        norm, coef = _torch_step(opt, clones, regions, flat, max_norm)
        assert abs(float(stats[1]) - norm) <= 1e-5 * norm, f"step {it}: norm {float(stats[1])} vs {norm}"
        assert abs(float(stats[2]) - coef) <= 1e-5, f"step {it}: coefficient {float(stats[2])} vs {coef}"
        assert float(stats[3]) == 0.0
        coefs.append(coef)
    assert state.step == 5
    if cfg["clip"]:
        assert min(coefs) < 1.0 and max(coefs) == 1.0         # the limit clips on some steps and not on others
    m_views, v_views = state.views()
    k = 0
    for idx, (off, size, t) in enumerate(regions):
        if t is None:
            assert m_views[idx] is None
            continue
        _assert_close(t, clones[k], f"parameter {idx}")
        if cfg["kind"] == "adamw":
            st = opt.state[clones[k]]
            _assert_close(m_views[idx], st["exp_avg"], f"exp_avg {idx}")
            _assert_close(v_views[idx], st["exp_avg_sq"], f"exp_avg_sq {idx}")
        k += 1
    if cfg["kind"] == "adamw":            # nothing is written where no tensor lives
        for (off, size, t) in regions:
            if t is None:
                assert not state.exp_avg[off:off + size].any() and not state.exp_avg_sq[off:off + size].any()


def test_zero_learning_rate_freezes_the_parameters_but_not_the_moments():
    """2. update_learning_rates (density_experiment.py:511-513): lr = 0 for a component that is not being trained."""
    import torch
    from gbnf_amd import native
    dev = torch.device("cuda:0")
    tr = _trainer("realnvp_d21_h32_K3_bn", dev)
    before = [None if t is None else t.clone() for t in tr.params]
    state = native.OptState(tr, "adamw")
    flat = _random_grads(tr, dev, seed=5)[0].to(dev)
    tr.apply_update(flat, state, lr=0.0, weight_decay=1e-5, max_grad_norm=0.5)
    for t, b in zip(tr.params, before):
        if t is not None:
            assert torch.equal(t, b)
    assert float(state.exp_avg.abs().max()) > 0 and float(state.exp_avg_sq.max()) > 0


def test_update_is_bit_identical_from_run_to_run():
    """3. Same inputs, two runs: parameters, state and stats agree bit for bit."""
    import torch
    from gbnf_amd import native
    dev = torch.device("cuda:0")
    results = []
    for run in range(2):
        tr = _trainer("glow_d43_h215_K5", dev)
        state = native.OptState(tr, "adamw")
        flats = _random_grads(tr, dev, seed=7)
        stats = [tr.apply_update(f.to(dev), state, lr=LR, weight_decay=1e-5, max_grad_norm=0.5).clone() for f in flats[:2]]
        results.append(([t.clone() for t in tr.params], state.exp_avg.clone(), state.exp_avg_sq.clone(), stats))
    (pa, ma, va, sa), (pb, mb, vb, sb) = results
    assert all(torch.equal(a, b) for a, b in zip(pa, pb))
    assert torch.equal(ma, mb) and torch.equal(va, vb)
    assert all(torch.equal(a, b) for a, b in zip(sa, sb))


@pytest.mark.parametrize("name", GRADS_CASES)
def test_whole_step_matches_reference_backward(name):
    """4. nll_step with lr = 0 on the g10 fixtures (the reference's own nll.backward()): the loss and the flat gradient."""
    import torch
    from gbnf_amd import native
    dev = torch.device("cuda:0")
    cfg, spec, x, nll, flat, g_x = load_grads_case(name)
    tr = native.NativeTrainer(_dev_spec(spec, dev))            # RealNVP: BatchNorm on running statistics, as in the fixture
    before = [None if t is None else t.clone() for t in tr.params]
    stats, grads = tr.nll_step(torch.from_numpy(x).to(dev), native.OptState(tr, "adamw"), lr=0.0)
    my_nll = float(stats[0])
    print(f"{name}: nll {my_nll} vs {nll}")
    assert abs(my_nll - nll) <= 1e-5 * abs(nll)
    _check_flat_grads(grads, flat, tr, name)
    for t, b in zip(tr.params, before):
        if t is not None:
            assert torch.equal(t, b)


def test_whole_step_in_batch_statistics_mode_matches_reference():
    """4. (g10_realnvp_grads_train_bn) BatchNorm in train() form: loss, gradients through the statistics, and bn_momentum = 0.9 moves
    the running statistics like models/layers.py:339-344."""
    import torch
    from gbnf_amd import native
    dev = torch.device("cuda:0")
    cfg, spec, x, data = load_train_bn_case()
    ds = _dev_spec(spec, dev)
    bns = [st["bn"] for st in ds["steps"] if st["bn"] is not None]
    for bn in bns:
        bn["batch_mean"] = torch.zeros(cfg["d"], device=dev)
        bn["batch_var"] = torch.zeros(cfg["d"], device=dev)
    tr = native.NativeTrainer(ds)
    assert tr.has_batch_stats
    tr.set_batch_stats(True)
    stats, grads = tr.nll_step(torch.from_numpy(x).to(dev), native.OptState(tr, "adamw"), lr=0.0, bn_momentum=0.9)
    nll = float(data["nll"])
    print(f"train_bn: nll {float(stats[0])} vs {nll}")
    assert abs(float(stats[0]) - nll) <= 1e-5 * abs(nll)
    _check_flat_grads(grads, data["grads"], tr, "train_bn")
    for k, bn in enumerate(bns):
        np.testing.assert_allclose(bn["running_mean"].cpu().numpy(), data["running_mean"][k], rtol=0, atol=2e-6)
        np.testing.assert_allclose(bn["running_var"].cpu().numpy(), data["running_var"][k], rtol=0, atol=2e-6)
    # bn_momentum < 0: the running statistics stay where they are
    kept = [bn["running_mean"].clone() for bn in bns]
    tr.nll_step(torch.from_numpy(x).to(dev), native.OptState(tr, "adamw"), lr=0.0)
    assert all(torch.equal(bn["running_mean"], k) for bn, k in zip(bns, kept))


@pytest.mark.parametrize("geometry,n", [(("glow", 8, 32, 3, {}), 77), (("realnvp", 21, 32, 3, {}), 33)])
def test_whole_step_is_its_parts(geometry, n):
    """5. One nll_step = the update of test 1 applied to the gradient it returns; rows = a gather in front; n = 1 runs."""
    import torch
    from gbnf_amd import native, synth
    dev = torch.device("cuda:0")
    d = geometry[1]
    hyper = dict(lr=LR, weight_decay=1e-5, max_grad_norm=1e-3)

    tr = _trainer(geometry, dev)
    regions = _regions(tr)
    live = [r for r in regions if r[2] is not None]
    clones = [t.detach().cpu().clone().requires_grad_(True) for _, _, t in live]
    x = torch.from_numpy(synth.synth_batch(n, d, seed=2)).to(dev)
    stats, grads = tr.nll_step(x, native.OptState(tr, "adamw"), **hyper)
    assert float(stats[2]) < 1.0, "the limit was meant to clip"
    opt = _torch_optimizer(clones, "adamw", LR, 1e-5)
    norm, coef = _torch_step(opt, clones, regions, grads.cpu(), hyper["max_grad_norm"])
    assert abs(float(stats[1]) - norm) <= 1e-5 * norm and abs(float(stats[2]) - coef) <= 1e-5
    for k, (off, size, t) in enumerate(live):
        _assert_close(t, clones[k], f"parameter at {off}")

    # rows with repeats, n != n_x: the same step as on the gathered batch
    xs = torch.from_numpy(synth.synth_batch(50, d, seed=4)).to(dev)
    rows = torch.randint(0, 50, (77,), generator=torch.Generator().manual_seed(1)).to(dev)
    assert rows.unique().numel() < 77
    tr_a, tr_b = _trainer(geometry, dev), _trainer(geometry, dev)
    sa, ga = tr_a.nll_step(xs, native.OptState(tr_a, "adamw"), rows=rows, lr=0.0)
    sb, gb = tr_b.nll_step(xs[rows].contiguous(), native.OptState(tr_b, "adamw"), lr=0.0)
    assert abs(float(sa[0]) - float(sb[0])) <= 1e-5 * abs(float(sb[0]))
    _check_flat_grads(ga, gb.cpu().numpy(), tr_a, "rows")

    s1, g1 = tr_a.nll_step(xs[:1].contiguous(), native.OptState(tr_a, "adamw"), **hyper)
    assert torch.isfinite(s1).all() and torch.isfinite(g1).all()


def test_resume_from_a_torch_optimizer():
    """6. Two AdamW steps through the module path, OptState.load_from, a third step fused: equals torch's third step on a clone fed the
    gradient the fused step returned (a wrong `step` / bias correction shows here); store_to hands the state back."""
    import torch
    from gbnf_amd import BoostedFlow, native
    dev = torch.device("cuda:0")
    torch.manual_seed(0)
    m = BoostedFlow(_args("glow", 8, 32, 3, 1, dev)).to(dev)
    m.train()
    x = torch.randn(256, 8, device=dev) * torch.linspace(0.5, 2.0, 8, device=dev) + 0.3
    opt = torch.optim.AdamW(m.flows[0].parameters(), lr=LR, weight_decay=1e-5)
    for it in range(2):
        opt.zero_grad()
        z, _, _, ldj, _ = m(x=x, components=0)
        torch.mean(-(torch.sum(-0.5 * np.log(2 * np.pi) - 0.5 * z.pow(2), dim=-1) + ldj)).backward()
        opt.step()
    tr = m.native_trainer(0)
    state = native.OptState(tr, "adamw").load_from(opt, tr.params)
    assert state.step == 2
    # a CPU twin of the optimiser at this point
    clones = [p.detach().cpu().clone().requires_grad_(True) for p in tr.params]
    twin = torch.optim.AdamW(clones, lr=LR, weight_decay=1e-5, foreach=False)
    for p, c in zip(tr.params, clones):
        twin.state[c] = {"step": torch.tensor(2.0), "exp_avg": opt.state[p]["exp_avg"].detach().cpu().clone(),
                         "exp_avg_sq": opt.state[p]["exp_avg_sq"].detach().cpu().clone()}
    regions = _regions(tr)
    stats, grads = tr.nll_step(x, state, lr=LR, weight_decay=1e-5)
    assert state.step == 3
    _torch_step(twin, clones, regions, grads.cpu(), 0.0)
    for k, (p, c) in enumerate(zip(tr.params, clones)):
        _assert_close(p, c, f"parameter {k} after the fused third step")
    # back to torch: a fourth step with the same gradient on both sides
    state.store_to(opt, tr.params)
    assert all(int(opt.state[p]["step"]) == 3 for p in tr.params)
    g4 = _random_grads(tr, dev, seed=9)[0]
    for (off, size, p) in regions:
        p.grad = g4[off:off + size].view(p.shape).to(dev)
    opt.step()
    _torch_step(twin, clones, regions, g4, 0.0)
    for k, (p, c) in enumerate(zip(tr.params, clones)):
        _assert_close(p, c, f"parameter {k} after store_to + a torch step")


def _nll_of(m, x, c=0):
    import torch
    with torch.no_grad():
        z, _, _, ldj, _ = m(x=x, components=c)
        return torch.mean(-(torch.sum(-0.5 * np.log(2 * np.pi) - 0.5 * z.pow(2), dim=-1) + ldj)).item()


def test_module_training_step_lowers_the_nll_and_invalidates_packed_copies():
    """7. The configuration of test_training_steps_lower_the_nll_without_rebinding through BoostedFlow.training_step."""
    import torch
    from gbnf_amd import BoostedFlow
    dev = torch.device("cuda:0")
    torch.manual_seed(0)
    m = BoostedFlow(_args("glow", 8, 32, 3, 2, dev)).to(dev)
    m.train()
    x = torch.randn(512, 8, device=dev) * torch.linspace(0.5, 2.0, 8, device=dev) + 0.3
    losses, trainer_ids = [], set()
    for it in range(30):
        out = m.training_step(x, lr=5e-3)
        assert set(out) == {"nll", "grad_norm", "clip_coef"} and all(v.dim() == 0 and v.is_cuda for v in out.values())
        losses.append(out["nll"].item())
        trainer_ids.add(id(m.native_trainer(0)))
        if it == 0:                    # a packed evaluation copy exists from here on: the later updates must reach it
            m.eval()
            _nll_of(m, x)
            m.train()
    assert len(trainer_ids) == 1
    assert losses[-1] < losses[0] - 0.2
    assert m.opt_state(0).step == 30
    m.eval()
    after = _nll_of(m, x)               # packed evaluation kernel
    assert abs(after - losses[-1]) < 0.05, f"eval {after} vs last training value {losses[-1]} (first {losses[0]})"


def test_module_training_step_of_a_boosted_component_on_a_repairing_trainer():
    """7. component = 1: resampled with the fixed component's boosting weights (the caller's RNG), train_math = "repair"."""
    import torch
    from gbnf_amd import BoostedFlow
    dev = torch.device("cuda:0")
    torch.manual_seed(0)
    args = _args("glow", 8, 32, 3, 2, dev)
    args.train_math = "repair"
    m = BoostedFlow(args).to(dev)
    m.train()
    x = torch.randn(512, 8, device=dev) * torch.linspace(0.5, 2.0, 8, device=dev) + 0.3
    m.training_step(x, lr=5e-3)        # component 0 (initialises its ActNorm)
    m.component = 1
    before = [p.clone() for p in m.flows[1].parameters()]
    fixed = [p.clone() for p in m.flows[0].parameters()]
    out = m.training_step(x, lr=5e-3, max_grad_norm=5.0, resample=True)
    assert set(out) == {"nll", "grad_norm", "clip_coef", "G_nll"}
    assert all(torch.isfinite(v).item() for v in out.values())
    assert m.native_trainer(1).math == "repair"
    assert any(not torch.equal(a, b) for a, b in zip(before, m.flows[1].parameters()))
    assert all(torch.equal(a, b) for a, b in zip(fixed, m.flows[0].parameters()))


def test_step_argument_validation():
    """8. Bad arguments: GBNF_ERR_INVALID with a message, nothing launched (parameters and stats untouched)."""
    import torch
    from gbnf_amd import native
    dev = torch.device("cuda:0")
    L = native.lib()
    tr = _trainer("glow_d6_h30_K2", dev)
    before = [t.clone() for t in tr.params]
    n, d = 16, 6
    x = torch.randn(n, d, device=dev)
    flat = torch.ones(tr.grad_floats, device=dev)
    m, v = torch.zeros_like(flat), torch.zeros_like(flat)
    stats = torch.full((4,), -7.0, device=dev)
    nb = C.c_int64()
    assert L.gbnf_trainer_step_workspace_bytes(tr.handle, n, C.byref(nb)) == 0 and nb.value > 0
    ws = torch.empty(nb.value // 4 + 1, dtype=torch.float32, device=dev)
    ptr = lambda t: C.c_void_p(t.data_ptr()) if t is not None else C.c_void_p(0)
    hyper = lambda **kw: native._OptHyper(**{**dict(kind=1, step=1, lr=1e-3, beta1=0.9, beta2=0.999, eps=1e-8, bn_momentum=-1.0), **kw})

    def update(h, m_=m, v_=v):
        return L.gbnf_trainer_apply_update(tr.handle, ptr(flat), ptr(m_), ptr(v_), C.byref(h), ptr(stats), None)

    def step(h, n_x=n, rows=None, n_=n, m_=m, v_=v, ws_bytes=None):
        return L.gbnf_trainer_nll_step(tr.handle, ptr(x), n_x, ptr(rows), n_, ptr(flat), ptr(m_), ptr(v_), C.byref(h), ptr(stats), ptr(ws),
                                       nb.value if ws_bytes is None else ws_bytes, None)

    bad = [lambda: update(hyper(kind=2)), lambda: update(hyper(kind=-1)), lambda: update(hyper(), m_=None),
           lambda: update(hyper(), v_=None), lambda: update(hyper(step=0)), lambda: update(hyper(step=-3)),
           lambda: step(hyper(kind=2)), lambda: step(hyper(), m_=None), lambda: step(hyper(step=0)),
           lambda: step(hyper(), ws_bytes=nb.value - 256), lambda: step(hyper(), n_=n - 1), lambda: step(hyper(), n_=0, n_x=0)]
    for k, call in enumerate(bad):
        assert call() == -1, f"bad call {k} was accepted"
        assert L.gbnf_last_error(), f"bad call {k} left no message"
    torch.cuda.synchronize()
    assert all(torch.equal(a, b) for a, b in zip(before, tr.params))
    assert torch.equal(stats, torch.full((4,), -7.0, device=dev)) and not m.any() and torch.equal(flat, torch.ones_like(flat))
    # SGD needs no state; and the good call goes through
    assert update(hyper(kind=0), m_=None, v_=None) == 0
    assert step(hyper()) == 0
    torch.cuda.synchronize()
    assert torch.isfinite(stats).all() and float(stats[1]) > 0
