"""GPU: the joint likelihood step of the whole tabular mixture -- gbnf_mixture_nll_step (csrc/gbnf_mixstep.hip),
native.mixture_nll_step and BoostedFlow.mixture_training_step -- against the float64 yardstick tests/mixture_step_oracle.py, torch's
clip_grad_norm_ + torch.optim on CPU clones, and gbnf_trainer_nll_step (C = 1, bit for bit).

Bars, none of them new: ll / G / nll 1e-5 relative (BASELINE); r within 1e-5 max(1, max|ll64|) (tests/test_hip_score.py); gradients
G_RTOL = 2e-4 of each tensor's largest float64 entry (tests/test_hip_train.py), the yardstick taken on the DEVICE's r; parameters and
moments PARAM_TOL = 1e-6 max|tensor| (tests/test_hip_fused_step.py).  The gradient floor is 1e-3 x the device's mean responsibility
of the component, not _check_grads' fixed 1e-3: the gradient is linear in r, and the fixed floor would judge nothing of a component
that carries 1 % of the batch."""
import ctypes as C

import numpy as np
import pytest

from conftest import rel_err
from test_hip_fused_step import LR, PARAM_TOL, _assert_close, _regions, _torch_optimizer
from test_hip_train import G_RTOL, _args, _dev_spec
import mixture_step_oracle as mso
import score_oracle

pytestmark = pytest.mark.gpu


def _dev():
    import torch
    return torch.device("cuda:0")


def _trainers(specs, math="f16x3", deterministic=False):
    from gbnf_amd import native
    return [native.NativeTrainer(_dev_spec(sp, _dev()), math=math, deterministic=deterministic) for sp in specs]


def _states(trainers, kind="adamw"):
    from gbnf_amd import native
    return [native.OptState(t, kind) for t in trainers]


def _log_w(rho, C_):
    import torch
    return torch.from_numpy(score_oracle.log_weights64(rho, C_).astype(np.float32)).to(_dev())


def _snapshot(trainers):
    return [[None if t is None else t.clone() for t in tr.params] for tr in trainers]


def _same(a, b):
    import torch
    return all((p is None and q is None) or torch.equal(p, q) for u, v in zip(a, b) for p, q in zip(u, v))


def _check_component_grads(flat, ref64, tr, rbar_c, what):
    """G_RTOL of each tensor's largest float64 entry, floor 1e-3 rbar_c; reserved regions stay zero."""
    flat = flat.detach().cpu().numpy().astype(np.float64)
    assert np.isfinite(flat).all()
    worst = 0.0
    for k, (off, size, t) in enumerate(_regions(tr)):
        a, b = flat[off:off + size], ref64[off:off + size]
        if t is None:
            assert not a.any(), f"{what}: reserved region {k} is not zero"
            continue
        scale = max(float(np.abs(b).max()), 1e-3 * rbar_c)
        err = float(np.abs(a - b).max())
        worst = max(worst, err / scale)
        assert err <= G_RTOL * scale, f"{what}: gradient {k} ({size}): {err:.3e} vs scale {scale:.3e}"
    return worst


def _check_step_against_float64(specs, rho, x_np, trainers, stats, flats, G, r, what, grads=True, forward=None):
    """What test group 1 asks of one lr = 0 call: G, r, nll, the mean responsibilities, the gradients on the device's r, the norms."""
    nc, n = len(specs), x_np.shape[0]
    fwd = score_oracle.mixture64(specs, rho, x_np) if forward is None else forward
    zs, ll64, r64, G64 = fwd
    st = stats.cpu().numpy().astype(np.float64)
    r_dev = r.cpu().numpy().astype(np.float64)
    e_G, e_nll = rel_err(G.cpu().numpy(), G64), abs(st[0] + G64.mean()) / max(abs(G64.mean()), 1.0)
    eps = 1e-5 * max(1.0, float(np.abs(ll64).max()))
    dr = float(np.abs(r_dev - r64).max())
    print(f"{what}: G rel_err {e_G:.2e}, nll rel_err {e_nll:.2e}, |dr| {dr:.2e} (eps {eps:.2e}), rbar {np.array2string(st[4:4 + nc], precision=3)}")
    assert e_G < 1e-5 and e_nll < 1e-5 and dr <= eps
    assert st[3] == 0.0
    assert np.abs(st[4:4 + nc] - r_dev.mean(axis=1)).max() <= 1e-6
    norms = np.array([float(f.double().norm()) for f in flats])
    assert np.abs(st[4 + nc:4 + 2 * nc] - norms).max() <= 1e-5 * norms.max()
    total = float(np.sqrt((norms ** 2).sum()))
    assert abs(st[1] - total) <= 1e-5 * total
    if grads:
        g64 = mso.step64(specs, rho, x_np, r=r_dev, forward=fwd)[4]
        for c in range(nc):
            worst = _check_component_grads(flats[c], mso.flat64(specs[c], g64[c]), trainers[c], float(st[4 + c]), f"{what} component {c}")
            print(f"{what}: component {c} worst gradient error {worst:.2e} of its bar's scale (bar {G_RTOL})")
    return st


# ---- 1. gradients, loss and statistics against float64 -------------------------------------------------------------------------------
FIXTURES = ["g6_glow_d43_h64_c3_rho", "g5_glow_d6_h30_c2", "g5_realnvp_d6_h30_c3", "g4_realnvp_d21_h105_c2_mixed",
            "g5_glow_d43_h64_c2_depth2", "g4_realnvp_d21_h105_c8"]
CASES_1 = [(name, "f16x3") for name in FIXTURES] + [(name, math) for name in FIXTURES[:2] for math in ("bf16x6", "repair")]


@pytest.mark.parametrize("name,math", CASES_1)
def test_step_matches_float64(name, math, golden_case):
    import torch
    from gbnf_amd import native
    g = golden_case(name)
    specs = g.specs[: g.n_used]
    trainers = _trainers(specs, math)
    before = _snapshot(trainers)
    x = torch.from_numpy(g.x).to(_dev())
    states = _states(trainers)
    stats, flats, G, r = native.mixture_nll_step(trainers, states, _log_w(g.rho, len(specs)), x, lr=0.0, want_G=True, want_r=True)
    torch.cuda.synchronize()
    assert _same(before, _snapshot(trainers)), "lr = 0 moved a parameter"
    assert all(s.step == 1 for s in states)
    st = _check_step_against_float64(specs, g.rho, g.x, trainers, stats, flats, G, r, f"{name} {math}")
    assert st[2] == 1.0          # no limit given: nothing clipped


# ---- 2. shapes where the new kernels can go wrong ------------------------------------------------------------------------------------
_SHAPE_FWD = {}


@pytest.mark.parametrize("n,misalign", [(1, 0), (77, 0), (77, 1), (1100, 0), (8192, 0)])
def test_shapes(n, misalign):
    """One row; a ragged wave (the seed's element tail, several norm workgroups); x off the 16-byte grid; two sums workgroups, the
    second ragged (n = 1100); every thread of the sums walks the grid stride (n = 8192).  nll and norms at every size, gradients
    against float64 up to n = 77."""
    import torch
    from gbnf_amd import native, synth
    specs = synth.synth_boosted_specs("glow", 2, 43, 64, 2, seed=5)
    rho = np.array([1.0, 0.6], dtype=np.float32)
    x_np = synth.synth_batch(n, 43, seed=n)
    if n not in _SHAPE_FWD:
        _SHAPE_FWD[n] = score_oracle.mixture64(specs, rho, x_np)
    trainers = _trainers(specs)
    buf = torch.zeros(n * 43 + 4, dtype=torch.float32, device=_dev())
    x = buf[misalign: misalign + n * 43].view(n, 43)
    x.copy_(torch.from_numpy(x_np))
    assert x.data_ptr() % 16 == 4 * misalign
    stats, flats, G, r = native.mixture_nll_step(trainers, _states(trainers), _log_w(rho, 2), x, lr=0.0, want_G=True, want_r=True)
    _check_step_against_float64(specs, rho, x_np, trainers, stats, flats, G, r, f"n={n} misalign={misalign}", grads=n <= 77,
                                forward=_SHAPE_FWD[n])


# ---- 3. the update -------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("kind", ["adamw", "sgd"])
def test_update_matches_torch_over_all_components(kind):
    """Three consecutive steps on three RealNVP components against CPU clones fed the returned flats: ONE clip_grad_norm_ over all
    components' parameters, then one torch.optim per component.  Component 0 starts two updates ahead (differing AdamW steps),
    component 2 runs with lr = 0."""
    import torch
    from gbnf_amd import native, synth
    dev = _dev()
    specs = synth.synth_boosted_specs("realnvp", 3, 21, 32, 3, seed=3)
    rho = np.array([1.0, 0.7, 0.4], dtype=np.float32)
    wd = 1e-5 if kind == "adamw" else 1e-3
    lrs = [LR, 2 * LR, 0.0]
    # (three batches of different spread: their total norms differ by more than a step moves them)
    xs = [torch.from_numpy(synth.synth_batch(64, 21, seed=20 + it, scale=s)).to(dev) for it, s in enumerate((1.0, 0.6, 1.4))]
    log_w = _log_w(rho, 3)

    def fresh():
        trainers = _trainers(specs)
        states = _states(trainers, kind)
        g = torch.Generator().manual_seed(1)
        pre = [(torch.randn(trainers[0].grad_floats, generator=g) * 1e-2).to(dev) for _ in range(2)]
        for f in pre:          # component 0 is two updates ahead
            trainers[0].apply_update(f, states[0], lr=LR, weight_decay=wd)
        return trainers, states

    # a first pass (no limit) finds the three total norms; the median is the limit of the judged pass
    trainers, states = fresh()
    totals = [float(native.mixture_nll_step(trainers, states, log_w, x, lr=lrs, weight_decay=wd)[0][1]) for x in xs]
    max_norm = sorted(totals)[1]

    trainers, states = fresh()
    assert [s.step for s in states] == [2, 0, 0]
    regions = [_regions(t) for t in trainers]
    clones = [[t.detach().cpu().clone().requires_grad_(True) for _, _, t in reg if t is not None] for reg in regions]
    opts = [_torch_optimizer(cl, kind, lr, wd) for cl, lr in zip(clones, lrs)]
    if kind == "adamw":        # the clones of component 0 continue on its moments and step
        m0, v0 = states[0].views()
        live = [k for k, (_, _, t) in enumerate(regions[0]) if t is not None]
        for p, k in zip(clones[0], live):
            opts[0].state[p] = {"step": torch.tensor(2.0), "exp_avg": m0[k].detach().cpu().clone(),
                                "exp_avg_sq": v0[k].detach().cpu().clone()}
    frozen = [t.clone() for t in trainers[2].params if t is not None]
    coefs = []
    for it, x in enumerate(xs):
        stats, flats, _, _ = native.mixture_nll_step(trainers, states, log_w, x, lr=lrs, weight_decay=wd, max_grad_norm=max_norm)
        st = stats.cpu().double()
        for c in range(3):
            flat = flats[c].cpu()
            live = [r for r in regions[c] if r[2] is not None]
            for p, (off, size, t) in zip(clones[c], live):
                p.grad = flat[off:off + size].view(p.shape).clone()
        norm = float(torch.nn.utils.clip_grad_norm_([p for cl in clones for p in cl], max_norm, foreach=False))
        for o in opts:
            o.step()
        want = min(1.0, max_norm / (float(torch.sqrt((st[7:10] ** 2).sum())) + 1e-6))
        assert abs(float(st[1]) - norm) <= 1e-5 * norm, f"step {it}: total norm {float(st[1])} vs {norm}"
        assert abs(float(st[2]) - want) <= 1e-5, f"step {it}: coefficient {float(st[2])} vs {want}"
        assert abs(float(st[2]) - min(1.0, max_norm / (norm + 1e-6))) <= 1e-5
        coefs.append(float(st[2]))
    assert min(coefs) < 1.0 and max(coefs) == 1.0, coefs          # the limit clips on some steps and not on others
    assert [s.step for s in states] == [5, 3, 3]
    for c in range(3):
        m_views, v_views = states[c].views()
        k = 0
        for idx, (off, size, t) in enumerate(regions[c]):
            if t is None:
                continue
            _assert_close(t, clones[c][k], f"component {c} parameter {idx}")
            if kind == "adamw":
                s = opts[c].state[clones[c][k]]
                _assert_close(m_views[idx], s["exp_avg"], f"component {c} exp_avg {idx}")
                _assert_close(v_views[idx], s["exp_avg_sq"], f"component {c} exp_avg_sq {idx}")
            k += 1
    assert all(torch.equal(a, b) for a, b in zip(frozen, [t for t in trainers[2].params if t is not None])), "lr = 0 moved component 2"
    if kind == "adamw":
        assert float(states[2].exp_avg.abs().max()) > 0 and float(states[2].exp_avg_sq.max()) > 0


# ---- 4. C = 1 is gbnf_trainer_nll_step -----------------------------------------------------------------------------------------------
def test_lone_component_is_nll_step_bit_for_bit():
    import torch
    from gbnf_amd import native, synth
    spec = synth.synth_boosted_specs("glow", 1, 43, 64, 2, seed=9)[0]
    x = torch.from_numpy(synth.synth_batch(77, 43, seed=3)).to(_dev())
    hyper = dict(lr=LR, weight_decay=1e-5, max_grad_norm=0.05)
    (ta,), (tb,) = _trainers([spec], deterministic=True), _trainers([spec], deterministic=True)
    sa, sb = native.OptState(ta, "adamw"), native.OptState(tb, "adamw")
    stats_a, flat_a = ta.nll_step(x, sa, **hyper)
    stats_b, flats_b, G, r = native.mixture_nll_step([tb], [sb], torch.zeros(1, device=_dev()), x, want_G=True, want_r=True, **hyper)
    assert float(stats_a[2]) < 1.0, "the limit was meant to clip"
    assert torch.equal(r, torch.ones_like(r))
    assert torch.equal(flat_a, flats_b[0])
    assert _same(_snapshot([ta]), _snapshot([tb]))
    assert torch.equal(sa.exp_avg, sb.exp_avg) and torch.equal(sa.exp_avg_sq, sb.exp_avg_sq)
    assert torch.equal(stats_a[1:4], stats_b[1:4])
    assert abs(float(stats_a[0]) - float(stats_b[0])) <= 1e-6 * abs(float(stats_a[0]))
    assert float(stats_b[4]) == 1.0 and float(stats_b[5]) == float(stats_b[1])


# ---- 5. determinism ------------------------------------------------------------------------------------------------------------------
def test_deterministic_trainers_repeat_bit_for_bit():
    import torch
    from gbnf_amd import native, synth
    specs = synth.synth_boosted_specs("glow", 3, 43, 64, 2, seed=5)
    rho = np.array([1.0, 0.6, 0.3], dtype=np.float32)
    x = torch.from_numpy(synth.synth_batch(300, 43, seed=8)).to(_dev())
    outs = []
    for run in range(2):
        trainers = _trainers(specs, deterministic=True)
        states = _states(trainers)
        stats, flats, G, r = native.mixture_nll_step(trainers, states, _log_w(rho, 3), x, lr=LR, max_grad_norm=0.05, want_G=True,
                                                     want_r=True)
        outs.append((_snapshot(trainers), [s.exp_avg.clone() for s in states], [s.exp_avg_sq.clone() for s in states], flats, stats, G, r))
    a, b = outs
    assert float(a[4][2]) < 1.0
    assert _same(a[0], b[0])
    for k in (1, 2, 3):
        assert all(torch.equal(u, v) for u, v in zip(a[k], b[k]))
    assert torch.equal(a[4], b[4]) and torch.equal(a[5], b[5]) and torch.equal(a[6], b[6])


def test_deterministic_refusal_launches_nothing():
    """A flow of 26 steps trains on the per-step kernels (unordered float atomics): in deterministic mode the whole call is refused
    before the first launch, although the other component could be served."""
    import torch
    from gbnf_amd import native, synth
    specs = [synth.synth_glow_spec(8, 32, 3, seed=3, gain=0.3), synth.synth_glow_spec(8, 32, 26, seed=4, gain=0.3)]
    trainers = _trainers(specs, deterministic=True)
    before = _snapshot(trainers)
    x = torch.from_numpy(synth.synth_batch(64, 8, seed=1)).to(_dev())
    states = _states(trainers)
    with pytest.raises(native.GbnfError, match="deterministic"):
        native.mixture_nll_step(trainers, states, _log_w([1.0, 1.0], 2), x, lr=LR)
    torch.cuda.synchronize()
    assert _same(before, _snapshot(trainers))
    assert all(s.step == 0 and not s.exp_avg.any() for s in states)


# ---- 6. refusals on live handles -----------------------------------------------------------------------------------------------------
def test_refusals_on_live_handles_write_nothing():
    import torch
    from gbnf_amd import native, synth
    dev = _dev()
    L = native.lib()
    specs = synth.synth_boosted_specs("realnvp", 2, 21, 32, 3, seed=3)
    ds = [_dev_spec(sp, dev) for sp in specs]
    for st in ds[1]["steps"]:          # component 1 can run on batch statistics
        if st["bn"] is not None:
            st["bn"]["batch_mean"] = torch.zeros(21, device=dev)
            st["bn"]["batch_var"] = torch.zeros(21, device=dev)
    trainers = [native.NativeTrainer(s) for s in ds]
    other_d = _trainers(synth.synth_boosted_specs("realnvp", 1, 6, 30, 2, seed=3))[0]
    assert trainers[1].has_batch_stats
    n = 16
    x = torch.randn(n, 21, device=dev)
    log_w = _log_w([1.0, 1.0], 2)
    nb = native.mixture_step_workspace_bytes(trainers, n)
    ws = torch.empty(nb // 4 + 1, dtype=torch.float32, device=dev)
    flats = [torch.ones(max(t.grad_floats, other_d.grad_floats), device=dev) for t in trainers]
    ms = [torch.zeros_like(f) for f in flats]
    vs = [torch.zeros_like(f) for f in flats]
    stats = torch.full((8,), -7.0, device=dev)
    before = _snapshot(trainers + [other_d])
    arr = lambda ts: (C.c_void_p * 2)(*[t.data_ptr() for t in ts])
    hyper = lambda **kw: native._OptHyper(**{**dict(kind=1, step=1, lr=1e-3, beta1=0.9, beta2=0.999, eps=1e-8, bn_momentum=-1.0), **kw})

    def call(handles=None, hypers=None, ws_bytes=nb):
        hs = (native._OptHyper * 2)(*(hypers or [hyper(), hyper()]))
        h = (C.c_void_p * 2)(*(handles or [t.handle for t in trainers]))
        rc = L.gbnf_mixture_nll_step(h, 2, C.c_void_p(log_w.data_ptr()), C.c_void_p(x.data_ptr()), n, arr(flats), arr(ms), arr(vs), hs,
                                     C.c_void_p(stats.data_ptr()), None, None, C.c_void_p(ws.data_ptr()), ws_bytes, None)
        return rc, L.gbnf_last_error().decode(errors="replace")

    trainers[1].set_batch_stats(True)
    rc, msg = call()
    assert rc == -2 and "gbnf_trainer_set_batch_stats(0)" in msg, msg          # GBNF_ERR_UNSUPPORTED
    trainers[1].set_batch_stats(False)
    bad = {"the same trainer twice": dict(handles=[trainers[0].handle, trainers[0].handle]),
           "different d": dict(handles=[trainers[0].handle, other_d.handle]),
           "AdamW and SGD mixed": dict(hypers=[hyper(), hyper(kind=0)]),
           "two limits": dict(hypers=[hyper(max_grad_norm=1.0), hyper(max_grad_norm=2.0)]),
           "a step of 0": dict(hypers=[hyper(), hyper(step=0)]),
           "a workspace one byte short": dict(ws_bytes=nb - 1)}
    for what, kw in bad.items():
        rc, msg = call(**kw)
        assert rc == -1 and "gbnf_mixture_nll_step" in msg, f"{what}: rc {rc}, {msg}"
    torch.cuda.synchronize()
    assert _same(before, _snapshot(trainers + [other_d]))
    assert torch.equal(stats, torch.full((8,), -7.0, device=dev))
    assert all(torch.equal(f, torch.ones_like(f)) for f in flats) and not any(m.any() for m in ms)
    rc, msg = call()          # and the good call goes through
    torch.cuda.synchronize()
    assert rc == 0, msg
    assert bool(torch.isfinite(stats).all()) and float(stats[3]) == 0.0


# ---- 7. the module -------------------------------------------------------------------------------------------------------------------
def _glow_module(C_=3, deterministic=None, seed=0):
    import torch
    from gbnf_amd import BoostedFlow, synth
    dev = _dev()
    args = _args("glow", 43, 64, 2, C_, dev)
    if deterministic is not None:
        args.deterministic = deterministic
    m = BoostedFlow(args)
    for c, sp in enumerate(synth.synth_boosted_specs("glow", C_, 43, 64, 2, seed=5 + seed)):
        m.load_spec(c, sp)
    m.component = C_ - 1
    return m.to(dev)


def test_module_steps_lower_the_mixture_nll_and_rebuild_the_packed_copies():
    import torch
    from gbnf_amd import synth
    m = _glow_module()
    m.eval()
    x = torch.from_numpy(synth.synth_batch(256, 43, seed=2)).to(_dev())
    with torch.no_grad():
        start = float(-m.log_prob(x).mean())          # (a packed evaluation copy exists from here on)
    for it in range(20):
        out = m.mixture_training_step(x, lr=2e-3, max_grad_norm=50.0)
        assert set(out) == {"nll", "grad_norm", "clip_coef", "mean_responsibilities", "component_grad_norms"}
        assert all(v.is_cuda for v in out.values()) and out["nll"].dim() == 0 and out["grad_norm"].dim() == 0 and out["clip_coef"].dim() == 0
        assert out["mean_responsibilities"].shape == (3,) and out["component_grad_norms"].shape == (3,)
        if it == 0:
            assert abs(float(out["nll"]) - start) <= 1e-5 * abs(start)
            assert abs(float(out["mean_responsibilities"].sum()) - 1.0) <= 1e-5
    assert all(m.opt_state(c).step == 20 for c in range(3))
    assert all(p.grad is None for p in m.parameters())
    with torch.no_grad():
        end = float(-m.log_prob(x).mean())
    after = float(m.mixture_training_step(x, lr=0.0)["nll"])
    print(f"mixture nll {start:.4f} -> {end:.4f} (lr = 0 step: {after:.4f})")
    assert end < start
    assert abs(end - after) <= 1e-5 * abs(after), "log_prob ran on stale packed copies"


def test_module_call_is_the_native_call_in_deterministic_mode():
    import torch
    from gbnf_amd import native, synth
    x = torch.from_numpy(synth.synth_batch(100, 43, seed=2)).to(_dev())
    ma, mb = _glow_module(deterministic=True), _glow_module(deterministic=True)
    hyper = dict(lr=LR, weight_decay=1e-5, max_grad_norm=0.05)
    out = ma.mixture_training_step(x, **hyper)
    trainers = [mb.native_trainer(c) for c in range(3)]
    assert all(t.deterministic for t in trainers)
    stats = native.mixture_nll_step(trainers, [mb.opt_state(c) for c in range(3)], mb._log_w(3), x, **hyper)[0]
    assert torch.equal(out["nll"], stats[0]) and float(out["clip_coef"]) < 1.0
    for p, q in zip(ma.parameters(), mb.parameters()):
        assert torch.equal(p, q)


def test_module_in_train_mode_runs_on_running_statistics():
    import torch
    from gbnf_amd import BoostedFlow, synth
    dev = _dev()
    m = BoostedFlow(_args("realnvp", 21, 32, 3, 2, dev))
    for c, sp in enumerate(synth.synth_boosted_specs("realnvp", 2, 21, 32, 3, seed=3)):
        m.load_spec(c, sp)
    m.component = 1
    m = m.to(dev)
    m.train()
    x = torch.from_numpy(synth.synth_batch(64, 21, seed=2)).to(dev)
    xr = x.clone().requires_grad_(True)
    z, ldj = m.component_forward(xr, 0)          # a recorded train-mode forward that awaits its backward
    tr = m.native_trainer(0)
    assert tr.batch_stats
    buffers = {k: v.clone() for k, v in m.named_buffers()}
    params = [p.clone() for p in m.parameters()]
    out = m.mixture_training_step(x, lr=LR)
    assert bool(torch.isfinite(out["nll"]))
    assert tr.batch_stats, "the trainer's batch-statistics mode was not put back"
    for k, v in m.named_buffers():
        assert torch.equal(v, buffers[k]), f"buffer {k} moved"
    assert any(not torch.equal(p, q) for p, q in zip(m.parameters(), params))
    # the pending backward is refused, not wrong: by autograd itself where the step moved a saved parameter's version counter, else by
    # _FlowFunction ("batch statistics of this call were overwritten": forward_serial moved)
    with pytest.raises(RuntimeError):
        (z.sum() + ldj.sum()).backward()


def test_module_argument_errors():
    import torch
    from gbnf_amd import BoostedFlow
    dev = _dev()
    m = _glow_module()
    x = torch.randn(32, 43, device=dev)
    with pytest.raises(ValueError, match="lr"):
        m.mixture_training_step(x, lr=[LR, LR])
    fresh = BoostedFlow(_args("glow", 8, 32, 2, 2, dev)).to(dev)          # ActNorms not initialised
    fresh.component = 1
    with pytest.raises(ValueError, match="ActNorm"):
        fresh.mixture_training_step(torch.randn(32, 8, device=dev), lr=LR)


def test_module_with_one_component_is_the_plain_step():
    """n_used = 1 on a model whose component is 0: test 4 through the module, against training_step on a twin."""
    import torch
    from gbnf_amd import synth
    x = torch.from_numpy(synth.synth_batch(77, 43, seed=3)).to(_dev())
    ma, mb = _glow_module(deterministic=True), _glow_module(deterministic=True)
    ma.component = mb.component = 0
    ma.eval(), mb.eval()
    hyper = dict(lr=LR, weight_decay=1e-5, max_grad_norm=0.05)
    a = ma.training_step(x, resample=False, **hyper)
    b = mb.mixture_training_step(x, n_used=1, **hyper)
    assert torch.equal(a["grad_norm"], b["grad_norm"]) and torch.equal(a["clip_coef"], b["clip_coef"])
    assert abs(float(a["nll"]) - float(b["nll"])) <= 1e-6 * abs(float(a["nll"]))
    assert float(b["mean_responsibilities"][0]) == 1.0
    for p, q in zip(ma.parameters(), mb.parameters()):
        assert torch.equal(p, q)
    assert mb.opt_state(0).step == 1 and torch.equal(ma.opt_state(0).exp_avg, mb.opt_state(0).exp_avg)
