"""GPU: the training path (gbnf_trainer_*) against the float64 oracle and the reference's own
nll.backward() (fixtures g10_*).  Tolerances: forward as the evaluation path (1e-5 relative on ldj); gradients 2e-4 of the
largest entry of each tensor (f32 dot products over up to N samples, atomically accumulated in no fixed order)."""
import argparse

import numpy as np
import pytest

from conftest import GRADS_CASES, load_grads_case, rel_err

pytestmark = pytest.mark.gpu
G_RTOL = 2e-4


def _dev_spec(spec, dev):
    """flow spec (numpy) -> device spec (CUDA tensors) for native.NativeTrainer."""
    import torch
    t = lambda a: torch.from_numpy(np.ascontiguousarray(a, dtype=np.float32)).to(dev)
    net = lambda n: {"act": n["act"], "layers": [(t(w), t(b)) for w, b in n["layers"]]}
    out = {"kind": spec["kind"], "d": spec["d"], "coupling": spec.get("coupling"), "steps": []}
    for st in spec["steps"]:
        if spec["kind"] == "glow":
            out["steps"].append({"an_bias": t(st["an_bias"]), "an_logs": t(st["an_logs"]), "perm": st["perm"],
                                 "net": net(st["net"])})
        else:
            bn = st["bn"]
            out["steps"].append({"flipped": st["flipped"],
                                 "bn": None if bn is None else {**{k: t(bn[k]) for k in ("log_gamma", "beta", "running_mean",
                                                                                         "running_var")}, "eps": bn["eps"]},
                                 "t_net": net(st["t_net"]), "s_net": net(st["s_net"])})
    return out


def _check_grads(dev_grads, ref_grads, what, floor=1e-3):
    """``floor``: smallest scale a tensor is judged on (a gradient that is exactly zero by symmetry -- e.g. a bias in front of
    a batch-statistics BatchNorm -- comes out as f32 summation noise of the terms that cancel)."""
    assert len(dev_grads) == len(ref_grads)
    for k, (a, b) in enumerate(zip(dev_grads, ref_grads)):
        if b is None:
            assert a is None
            continue
        a = a.detach().cpu().numpy().reshape(b.shape)
        scale = max(float(np.abs(b).max()), floor)
        assert np.abs(a - b).max() <= G_RTOL * scale, f"{what}: gradient {k} shape {b.shape}: {np.abs(a - b).max()} vs scale {scale}"


TRAIN_CASES = ["g3_glow_d43_h215_c8", "g5_glow_d43_h64_c2_additive", "g5_glow_d43_h64_c2_reverse_relu",
               "g5_glow_d43_h64_c2_depth2", "g5_glow_d43_h64_c2_depth0", "g5_glow_d6_h30_c2", "g5_glow_d63_h128_c2",
               "g4_realnvp_d21_h105_c8", "g4_realnvp_d21_h105_c2_mixed", "g4_realnvp_d21_h105_c2_relu_nobn",
               "g5_realnvp_d6_h30_c3", "g6_glow_d43_h64_n77", "g6_glow_d43_h64_n1", "g6_realnvp_d21_h64_n33",
               "g1_toy_realnvp_c2"]


@pytest.mark.parametrize("name", TRAIN_CASES)
def test_trainer_forward_and_backward_match_oracle(name, golden_case):
    import torch
    from gbnf_amd import native
    from oracle import gbnf_oracle as oracle
    dev = torch.device("cuda:0")
    g = golden_case(name)
    rng = np.random.RandomState(7)
    for c in sorted({0, len(g.specs) - 1}):
        spec = g.specs[c]
        tr = native.NativeTrainer(_dev_spec(spec, dev))
        x = torch.from_numpy(g.x).to(dev)
        z, ldj = tr.forward(x)
        z64, ldj64 = oracle.component_forward(spec, g.x, backend="numpy64")
        assert rel_err(ldj.cpu().numpy(), ldj64) < 1e-5
        assert np.abs(z.cpu().numpy() - z64).max() <= 1e-5 * max(1.0, float(np.abs(z64).max()))
        g_z = rng.standard_normal(g.x.shape).astype(np.float32)
        g_l = rng.standard_normal(g.x.shape[0]).astype(np.float32)
        gx64, grads64 = oracle.component_grads(spec, g.x, g_z, g_l)
        gx, grads = tr.backward(x, torch.from_numpy(g_z).to(dev), torch.from_numpy(g_l).to(dev), want_gx=True)
        _check_grads(grads, grads64, f"{name}[{c}]")
        assert np.abs(gx.cpu().numpy() - gx64).max() <= G_RTOL * float(np.abs(gx64).max())
        # the same with the forward call's trace (no forward sweep inside the backward kernel): the same state (since round 3
        # the traced forward runs on the register-chained kernel: same arithmetic, another summation order)
        z2, ldj2, trace = tr.forward(x, want_trace=True)
        assert rel_err(ldj2.cpu().numpy(), ldj64) < 1e-5
        assert np.abs(z2.cpu().numpy() - z64).max() <= 1e-5 * max(1.0, float(np.abs(z64).max()))
        gx_t, grads_t = tr.backward(x, torch.from_numpy(g_z).to(dev), torch.from_numpy(g_l).to(dev), want_gx=True, trace=trace)
        _check_grads(grads_t, grads64, f"{name}[{c}] traced")
        assert np.abs(gx_t.cpu().numpy() - gx64).max() <= G_RTOL * float(np.abs(gx64).max())
        # null upstream gradients are zeros
        _, only_l = tr.backward(x, None, torch.from_numpy(g_l).to(dev))
        _, l64 = oracle.component_grads(spec, g.x, np.zeros_like(g_z), g_l)
        _check_grads(only_l, l64, f"{name}[{c}] g_z=None")


@pytest.mark.parametrize("name", ["g3_glow_d43_h215_c8", "g4_realnvp_d21_h105_c8", "g6_glow_d43_h64_n77", "g6_realnvp_d21_h64_n33",
                                  "g5_glow_d43_h64_c2_additive", "g5_glow_d43_h64_c2_reverse_relu"])
def test_traced_forward_on_32_sample_waves(name, golden_case):
    """From 32768 rows on the traced forward sweep runs 32-sample waves (flow_kernel_hx3<..., NT = 2, TRAIN>, compiled with the
    512-register budget): the same saves, two 16-sample tiles per wave.  The tuning knob forces that form at the fixtures'
    sizes (odd tile counts, a lone tile, ragged tails: the spare half of a wave shadows the last tile)."""
    import torch
    from gbnf_amd import native
    from oracle import gbnf_oracle as oracle
    dev = torch.device("cuda:0")
    g = golden_case(name)
    rng = np.random.RandomState(11)
    spec = g.specs[0]
    tr = native.NativeTrainer(_dev_spec(spec, dev))
    x = torch.from_numpy(g.x).to(dev)
    g_z = rng.standard_normal(g.x.shape).astype(np.float32)
    g_l = rng.standard_normal(g.x.shape[0]).astype(np.float32)
    z64, ldj64 = oracle.component_forward(spec, g.x, backend="numpy64")
    gx64, grads64 = oracle.component_grads(spec, g.x, g_z, g_l)
    native.tuning_set("force_nt", 2)
    try:
        z, ldj, trace = tr.forward(x, want_trace=True)
        gx, grads = tr.backward(x, torch.from_numpy(g_z).to(dev), torch.from_numpy(g_l).to(dev), want_gx=True, trace=trace)
        torch.cuda.synchronize()
    finally:
        native.tuning_set("force_nt", 0)
    assert rel_err(ldj.cpu().numpy(), ldj64) < 1e-5
    assert np.abs(z.cpu().numpy() - z64).max() <= 1e-5 * max(1.0, float(np.abs(z64).max()))
    _check_grads(grads, grads64, f"{name} NT=2")
    assert np.abs(gx.cpu().numpy() - gx64).max() <= G_RTOL * float(np.abs(gx64).max())


@pytest.mark.parametrize("kind,d,h", [("glow", 43, 215), ("realnvp", 21, 105)])
def test_traced_forward_keeps_out_of_range_rows_finite(kind, d, h):
    """the traced training forward runs the f16x3 evaluation kernel with TRAIN = 1; a row whose operands
    leave the fp16 range must be clamped and counted there (as the round-1 train_kernel does) -- marked NaN, with no repair
    pass behind the training forward, it would make the loss and every gradient NaN."""
    import torch
    from gbnf_amd import native, synth
    dev = torch.device("cuda:0")
    spec = (synth.synth_glow_spec(d, h, 5, seed=3) if kind == "glow" else synth.synth_realnvp_spec(d, h, 5, seed=3))
    tr = native.NativeTrainer(_dev_spec(spec, dev))
    x = synth.synth_batch(200, d, seed=4)
    x[7, :] = 3.0e5            # |x| > 65504: beyond the fp16 range
    x[150, 3] = -1.0e6
    xd = torch.from_numpy(x).to(dev)
    native.saturation_count(reset=True)
    z, ldj, trace = tr.forward(xd, want_trace=True)
    assert bool(torch.isfinite(z).all()) and bool(torch.isfinite(ldj).all())
    assert native.saturation_count(reset=True) > 0            # ... and the launch is counted
    g_x, grads = tr.backward(xd, torch.ones_like(z) / 200, torch.ones_like(ldj) / 200, want_gx=True, trace=trace)
    assert bool(torch.isfinite(g_x).all())
    assert all(bool(torch.isfinite(t).all()) for t in grads if t is not None)
    # the rows inside the range are what an all-in-range batch gives
    keep = [r for r in range(200) if r not in (7, 150)]
    z2, ldj2 = tr.forward(torch.from_numpy(np.ascontiguousarray(x[keep])).to(dev))
    assert rel_err(ldj[keep].cpu().numpy(), ldj2.cpu().numpy()) < 1e-5


@pytest.mark.parametrize("name", GRADS_CASES)
def test_trainer_matches_reference_backward(name):
    """g10: the reference's own nll.backward()."""
    import torch
    from gbnf_amd import native
    dev = torch.device("cuda:0")
    cfg, spec, x, nll, flat, g_x = load_grads_case(name)
    tr = native.NativeTrainer(_dev_spec(spec, dev))
    xd = torch.from_numpy(x).to(dev)
    z, ldj = tr.forward(xd)
    n = x.shape[0]
    my_nll = float(torch.mean(-(torch.sum(-0.5 * np.log(2 * np.pi) - 0.5 * z * z, dim=1) + ldj)))
    assert abs(my_nll - nll) <= 1e-5 * abs(nll)
    gx, grads = tr.backward(xd, (z / n).contiguous(), torch.full((n,), -1.0 / n, device=dev), want_gx=True)
    mine = np.concatenate([np.zeros(cfg["d"], np.float32) if gr is None else gr.cpu().numpy().reshape(-1) for gr in grads])
    assert np.abs(mine - flat).max() <= G_RTOL * float(np.abs(flat).max())
    assert np.abs(gx.cpu().numpy() - g_x).max() <= G_RTOL * float(np.abs(g_x).max())


def _args(kind, d, h, K, C, dev, **kw):
    return argparse.Namespace(
        num_flows=K, z_size=d, density_evaluation=True, device=dev, cuda=True, component_type=kind, num_components=C,
        rho_init="decreasing", learn_top=False, y_classes=0, y_condition=False, sample_size=4, input_size=[d], h_size=h,
        num_blocks=1, actnorm_scale=1.0, flow_permutation=kw.get("permutation", "shuffle"),
        flow_coupling=kw.get("coupling", "affine"), LU_decomposed=False, num_dequant_blocks=0,
        coupling_network=kw.get("act", kw.get("coupling_network", "tanh")), coupling_network_depth=kw.get("depth", 1),
        batch_norm=kw.get("batch_norm", True))


@pytest.mark.parametrize("name", GRADS_CASES)
def test_module_autograd_matches_reference(name):
    """The drop-in module in the reference's training step: nll of component 0, nll.backward(), p.grad vs the fixture."""
    import torch
    from gbnf_amd import BoostedFlow
    dev = torch.device("cuda:0")
    cfg, spec, x, nll, flat, g_x = load_grads_case(name)
    m = BoostedFlow(_args(cfg["kind"], cfg["d"], cfg["h"], cfg["K"], 1, dev, **cfg["synth_kw"]))
    m.load_spec(0, spec)
    xd = torch.from_numpy(x).to(dev).requires_grad_(True)
    if cfg["kind"] == "glow":
        m.train()
        z, _, _, ldj, _ = m(x=xd, components=0)
    else:                                   # RealNVP: running-statistics BatchNorm, as in the fixture
        m.eval()
        z, ldj = m.component_forward(xd, 0, differentiable=True)
    loss = torch.mean(-(torch.sum(-0.5 * np.log(2 * np.pi) - 0.5 * z.pow(2), dim=-1) + ldj))
    assert abs(loss.item() - nll) <= 1e-5 * abs(nll)
    loss.backward()
    from gbnf_amd import spec as gspec
    tr_params = [t for t in m.native_trainer(0).params]
    mine = np.concatenate([np.zeros(cfg["d"], np.float32) if t is None else t.grad.cpu().numpy().reshape(-1) for t in tr_params])
    assert np.abs(mine - flat).max() <= G_RTOL * float(np.abs(flat).max())
    assert np.abs(xd.grad.cpu().numpy() - g_x).max() <= G_RTOL * float(np.abs(g_x).max())


def test_training_steps_lower_the_nll_without_rebinding():
    """A few Adam steps on the HIP path: the trainer is created once (in-place updates need no repacking), the loss goes
    down, and the evaluation path afterwards sees the updated parameters."""
    import torch
    from gbnf_amd import BoostedFlow
    dev = torch.device("cuda:0")
    torch.manual_seed(0)
    m = BoostedFlow(_args("glow", 8, 32, 3, 2, dev)).to(dev)
    m.train()
    x = torch.randn(512, 8, device=dev) * torch.linspace(0.5, 2.0, 8, device=dev) + 0.3
    opt = torch.optim.Adam(m.flows[0].parameters(), lr=5e-3)
    losses = []
    trainer_ids = set()
    for it in range(30):
        opt.zero_grad()
        z, _, _, ldj, _ = m(x=x, components=0)
        loss = torch.mean(-(torch.sum(-0.5 * np.log(2 * np.pi) - 0.5 * z.pow(2), dim=-1) + ldj))
        loss.backward()
        opt.step()
        losses.append(loss.item())
        trainer_ids.add(id(m.native_trainer(0)))
    assert len(trainer_ids) == 1
    assert losses[-1] < losses[0] - 0.2
    m.eval()
    with torch.no_grad():
        z, _, _, ldj, _ = m(x=x, components=0)           # packed evaluation kernel, re-packed from the new parameters
        after = torch.mean(-(torch.sum(-0.5 * np.log(2 * np.pi) - 0.5 * z.pow(2), dim=-1) + ldj)).item()
    assert after < losses[-1] + 0.05


def test_in_place_change_between_forward_and_backward_is_caught():
    import torch
    from gbnf_amd import BoostedFlow
    dev = torch.device("cuda:0")
    m = BoostedFlow(_args("glow", 8, 32, 2, 1, dev)).to(dev)
    m.train()
    x = torch.randn(64, 8, device=dev)
    z, _, _, ldj, _ = m(x=x, components=0)
    with torch.no_grad():
        next(m.flows[0].parameters()).add_(1.0)
    with pytest.raises(RuntimeError):
        (z.sum() + ldj.sum()).backward()


def test_trainer_argument_validation():
    import ctypes as C
    import torch
    from gbnf_amd import native
    L = native.lib()
    assert L.gbnf_trainer_forward(None, None, 4, None, None, None, None) == -1
    assert L.gbnf_trainer_backward(None, None, 4, None, None, None, None, None, None, 0, None) == -1
    assert L.gbnf_trainer_destroy(None) == 0
    with pytest.raises(native.GbnfError):          # CPU tensors: no CPU path
        native.NativeTrainer({"kind": "glow", "d": 4, "coupling": "affine", "steps": [
            {"an_bias": torch.zeros(4), "an_logs": torch.zeros(4), "perm": np.arange(4),
             "net": {"act": "tanh", "layers": [(torch.zeros(8, 2), torch.zeros(8)), (torch.zeros(4, 8), torch.zeros(4))]}}]})


@pytest.mark.parametrize("kind", ["glow", "realnvp"])
def test_boosted_training_loop_like_the_reference(kind):
    """The reference's boosted training step (compute_kl_pq_loss, density_experiment.py:606-660) on the device path, both
    ways: the reference's own statement sequence through model(x=, components=) and the fused shortcuts
    (boosting_weights + one recorded forward).  Component 0 is trained first, then component 1 on re-weighted samples;
    the mixture's NLL on fresh data must improve over component 0 alone."""
    import math
    import torch
    from gbnf_amd import BoostedFlow
    dev = torch.device("cuda:0")
    torch.manual_seed(1)
    d = 6
    m = BoostedFlow(_args(kind, d, 32, 3, 2, dev)).to(dev)     # realnvp: default batch_norm=True, batch statistics in train()

    def sample(n):          # two well separated blobs: one component cannot fit both equally well
        a = torch.randn(n, d, device=dev) * 0.5 + 2.0
        b = torch.randn(n, d, device=dev) * 0.8 - 1.5
        return torch.where(torch.rand(n, 1, device=dev) < 0.5, a, b)

    def lns(z):             # log_normal_standard(z, reduce=True, dim=-1)
        return torch.sum(-0.5 * math.log(2 * math.pi) - 0.5 * z.pow(2), dim=-1)

    m.train()
    opt = torch.optim.Adam(m.flows[0].parameters(), lr=3e-3)
    for _ in range(60):     # first component: trained like a non-boosted model (:655-659)
        x = sample(512)
        opt.zero_grad()
        z, _, _, ldj, _ = m(x=x, components="c")
        loss = torch.mean(-(lns(z) + ldj))
        loss.backward()
        opt.step()
    m.increment_component()
    assert m.component == 1
    opt = torch.optim.Adam(m.flows[1].parameters(), lr=3e-3)
    for it in range(60):
        x = sample(512)
        opt.zero_grad()
        if it % 2 == 0:     # the reference's statements (:612-651)
            with torch.no_grad():
                z_G, _, _, ldj_G, _ = m(x=x, components=0)
                G_nll = -1.0 * (lns(z_G) + ldj_G)
                w = torch.softmax(G_nll, dim=0)
                if w.max() > 0.1:
                    w = torch.max(torch.min(w, torch.tensor([0.1], device=dev)), torch.tensor([0.01], device=dev))
                w = w / w.sum()
        else:               # the fused form of the same two steps
            with torch.no_grad():
                w, _ = m.boosting_weights(x)
        xr = x[torch.multinomial(w, x.size(0), replacement=True)]
        z_g, _, _, ldj_g, _ = m(x=xr, components="c")
        loss = torch.mean(-(lns(z_g) + ldj_g))
        loss.backward()
        opt.step()
    m.eval()
    with torch.no_grad():
        xt = sample(4096)
        nll_first = -m.log_prob(xt, n_used=1).mean().item()
        m.rho[1] = 0.5
        nll_mix = -m.log_prob(xt, n_used=2).mean().item()
    assert math.isfinite(nll_mix) and nll_mix < nll_first + 0.05, (nll_first, nll_mix)


def _random_train_cases():
    rng = np.random.RandomState(77)
    cases = []
    for k in range(14):
        kind = "glow" if k % 3 else "realnvp"
        d = int(rng.choice([2, 3, 5, 8, 13, 21, 43, 50, 64]))
        h = int(rng.choice([7, 16, 33, 64, 105, 129, 215, 256]))
        K = int(rng.randint(1, 5))
        n = int(rng.choice([1, 15, 17, 33, 100, 257]))
        depth = int(rng.choice([0, 1, 1, 2]))
        if kind == "glow":
            extra = dict(act=str(rng.choice(["tanh", "relu"])), coupling=str(rng.choice(["affine", "additive"])),
                         permutation=str(rng.choice(["shuffle", "reverse"])), depth=depth)
        else:
            extra = dict(coupling_network=str(rng.choice(["tanh", "relu", "mixed"])), batch_norm=bool(rng.randint(2)),
                         flip_init=int(rng.randint(2)), depth=depth)
        cases.append((kind, d, h, K, n, extra, 900 + k))
    # hidden widths above 256 (h = h_size_factor * D in the reference: 5 x 63 = 315, 10 x 43 = 430), one or two
    # 16-sample tiles per workgroup depending on what fits the LDS
    cases.append(("glow", 63, 315, 2, 100, dict(act="tanh", coupling="affine", permutation="shuffle", depth=1), 950))
    cases.append(("glow", 43, 430, 2, 77, dict(act="relu", coupling="affine", permutation="shuffle", depth=1), 951))
    cases.append(("realnvp", 21, 512, 2, 65, dict(coupling_network="tanh", batch_norm=True, flip_init=1, depth=1), 952))
    cases.append(("glow", 8, 300, 1, 33, dict(act="tanh", coupling="additive", permutation="reverse", depth=2), 953))
    # `--coupling_network random`: the activation changes from step to step (Glow) / net to net (RealNVP)
    cases.append(("glow", 21, 64, 6, 100, dict(act="random", coupling="affine", permutation="shuffle", depth=1), 954))
    cases.append(("realnvp", 13, 33, 6, 65, dict(coupling_network="random", batch_norm=True, flip_init=0, depth=1), 955))
    # ... at widths with a per-step-activation variant of their own: the register-chained kernels' run-time activation flag
    cases.append(("glow", 43, 215, 4, 300, dict(act="random", coupling="affine", permutation="shuffle", depth=1), 960))
    cases.append(("realnvp", 21, 105, 4, 129, dict(coupling_network="random", batch_norm=True, flip_init=1, depth=1), 961))
    cases.append(("glow", 43, 256, 3, 77, dict(act="relu", coupling="affine", permutation="reverse", depth=1), 962))
    # ResidualNet coupling networks (1 and 2 blocks)
    cases.append(("realnvp", 21, 64, 3, 100, dict(coupling_network="residual", batch_norm=True, flip_init=1, depth=1), 956))
    cases.append(("realnvp", 21, 215, 2, 2049, dict(coupling_network="residual", batch_norm=False, flip_init=0, depth=1), 957))
    cases.append(("realnvp", 8, 40, 3, 77, dict(coupling_network="residual", batch_norm=True, flip_init=0, depth=2), 958))
    return cases


@pytest.mark.parametrize("kind,d,h,K,n,extra,seed", _random_train_cases())
def test_trainer_random_shapes_against_oracle(kind, d, h, K, n, extra, seed):
    """Randomised geometry sweep of the training kernels (ragged rows / columns of every Linear, odd d, 1..4 steps,
    depth 0..2, ragged batches) against the float64 autograd oracle."""
    import torch
    from gbnf_amd import native, synth
    from oracle import gbnf_oracle as oracle
    dev = torch.device("cuda:0")
    spec = (synth.synth_glow_spec(d, h, K, seed=seed, **extra) if kind == "glow"
            else synth.synth_realnvp_spec(d, h, K, seed=seed, **extra))
    x = synth.synth_batch(n, d, seed=seed + 1)
    rng = np.random.RandomState(seed)
    g_z = rng.standard_normal(x.shape).astype(np.float32)
    g_l = rng.standard_normal(n).astype(np.float32)
    tr = native.NativeTrainer(_dev_spec(spec, dev))
    xd = torch.from_numpy(x).to(dev)
    z, ldj, trace = tr.forward(xd, want_trace=True)
    z64, ldj64 = oracle.component_forward(spec, x, backend="numpy64")
    assert np.abs(ldj.cpu().numpy() - ldj64).max() <= 1e-5 * max(1.0, float(np.abs(ldj64).max()))
    assert np.abs(z.cpu().numpy() - z64).max() <= 2e-5 * max(1.0, float(np.abs(z64).max()))
    gx64, grads64 = oracle.component_grads(spec, x, g_z, g_l)
    gx, grads = tr.backward(xd, torch.from_numpy(g_z).to(dev), torch.from_numpy(g_l).to(dev), want_gx=True, trace=trace)
    _check_grads(grads, grads64, f"{kind} d={d} h={h} K={K} n={n} {extra}")
    assert np.abs(gx.cpu().numpy() - gx64).max() <= G_RTOL * max(float(np.abs(gx64).max()), 1e-3)


@pytest.mark.parametrize("kind,batch_stats", [("glow", False), ("realnvp", False), ("realnvp", True)])
def test_backward_is_invariant_to_the_scale_of_the_loss(kind, batch_stats):
    """The backward pass is linear in the upstream gradient, and its accuracy must not depend on that gradient's
    magnitude: a mean over 65536 samples hands in 1.5e-5 per sample, a summed loss 1e4 times more.  (The split-f16
    operands only carry f32 accuracy for magnitudes around 1: the kernels rescale by a power of two per call.)"""
    import torch
    from gbnf_amd import native, synth
    from oracle import gbnf_oracle as oracle
    dev = torch.device("cuda:0")
    d, h, K, n = 21, 105, 4, 700
    spec = (synth.synth_glow_spec(d, h, K, seed=71) if kind == "glow"
            else synth.synth_realnvp_spec(d, h, K, seed=71, batch_norm=True))
    x = synth.synth_batch(n, d, seed=72)
    rng = np.random.RandomState(73)
    g_z = rng.standard_normal(x.shape).astype(np.float32)
    g_l = rng.standard_normal(n).astype(np.float32)
    gx64, gr64 = oracle.component_grads(spec, x, g_z, g_l, train=batch_stats)
    dev_spec = _dev_spec(spec, dev)
    if batch_stats:
        for st in dev_spec["steps"]:
            if st["bn"] is not None:
                st["bn"]["batch_mean"] = torch.zeros(d, device=dev)
                st["bn"]["batch_var"] = torch.zeros(d, device=dev)
    tr = native.NativeTrainer(dev_spec)
    if batch_stats:
        tr.set_batch_stats(True)
    xd = torch.from_numpy(x).to(dev)
    _, _, trace = tr.forward(xd, want_trace=True)
    floor = 0.05 * max(float(np.abs(g).max()) for g in gr64 if g is not None) if batch_stats else 1e-3
    for scale in (1.0, 1.5e-5, 1e-7, 3e4):
        sc = np.float32(scale)
        gx, gr = tr.backward(xd, torch.from_numpy(g_z * sc).to(dev), torch.from_numpy(g_l * sc).to(dev), want_gx=True, trace=trace)
        for a, b in zip(gr, gr64):
            if b is not None:
                got = a.cpu().numpy().reshape(b.shape).astype(np.float64) / float(sc)
                assert np.abs(got - b).max() <= G_RTOL * max(float(np.abs(b).max()), floor), scale
        assert np.abs(gx.cpu().numpy().astype(np.float64) / float(sc) - gx64).max() <= G_RTOL * float(np.abs(gx64).max()), scale


def test_trainer_counts_saturated_operands():
    import torch
    from gbnf_amd import native, synth
    dev = torch.device("cuda:0")
    native.saturation_count(reset=True)
    spec = synth.synth_glow_spec(8, 16, 2, seed=3, act="relu")
    tr = native.NativeTrainer(_dev_spec(spec, dev))
    x = synth.synth_batch(64, 8, seed=4)
    xd = torch.from_numpy(x).to(dev)
    z, ldj, trace = tr.forward(xd, want_trace=True)
    tr.backward(xd, torch.ones_like(z) * 1e-9, torch.ones_like(ldj) * 1e9, want_gx=True, trace=trace)   # any loss scale is fine
    assert native.saturation_count() == 0
    tr.forward(torch.from_numpy(x * np.float32(1e8)).to(dev))
    assert native.saturation_count(reset=True) > 0


def test_train_mode_batch_norm_matches_reference():
    """g10 (train-mode BatchNorm): RealNVP in train() like the reference's default configuration -- BatchNorm on batch
    statistics (one launch per step), nll.backward() through the statistics, running statistics updated."""
    import torch
    from conftest import load_train_bn_case
    from gbnf_amd import BoostedFlow
    dev = torch.device("cuda:0")
    cfg, spec, x, data = load_train_bn_case()
    m = BoostedFlow(_args("realnvp", cfg["d"], cfg["h"], cfg["K"], 1, dev))
    m.load_spec(0, spec)
    m.train()
    xd = torch.from_numpy(x).to(dev).requires_grad_(True)
    z, _, _, ldj, _ = m(x=xd, components=0)
    assert np.abs(z.detach().cpu().numpy() - data["z"]).max() <= 2e-5 * float(np.abs(data["z"]).max())
    assert rel_err(ldj.detach().cpu().numpy(), data["ldj"]) < 1e-5
    loss = torch.mean(-(torch.sum(-0.5 * np.log(2 * np.pi) - 0.5 * z.pow(2), dim=-1) + ldj))
    assert abs(loss.item() - float(data["nll"])) <= 1e-5 * abs(float(data["nll"]))
    loss.backward()
    tr = m.native_trainer(0)
    mine = np.concatenate([np.zeros(cfg["d"], np.float32) if t is None else t.grad.cpu().numpy().reshape(-1) for t in tr.params])
    assert np.abs(mine - data["grads"]).max() <= G_RTOL * float(np.abs(data["grads"]).max())
    assert np.abs(xd.grad.cpu().numpy() - data["g_x"]).max() <= G_RTOL * float(np.abs(data["g_x"]).max())
    bns = [mods[2] for mods in m.flows[0].flow_param if len(mods) > 2 and mods[2] is not None]
    for k, bn in enumerate(bns):
        np.testing.assert_allclose(bn.running_mean.cpu().numpy(), data["running_mean"][k], rtol=0, atol=2e-6)
        np.testing.assert_allclose(bn.running_var.cpu().numpy(), data["running_var"][k], rtol=0, atol=2e-6)
    # eval() afterwards: running statistics, single fused launch, packed kernels see the updated buffers
    m.eval()
    with torch.no_grad():
        z2, _, _, ldj2, _ = m(x=xd.detach(), components=0)
    assert torch.isfinite(ldj2).all() and not torch.allclose(ldj2, ldj.detach())


def _has_live_blob(tr):
    import ctypes as C
    from gbnf_amd import native
    L = native.lib()
    L.gbnf_debug_trainer_blob.argtypes = [C.c_void_p, C.c_void_p, C.POINTER(C.c_int64)]
    n = C.c_int64()
    return L.gbnf_debug_trainer_blob(tr.handle, None, C.byref(n)) == 0


def _last_path(tr):
    """(forward, backward) launches of the register-chained kernels by the trainer's last calls; 0 = the round-1 kernels ran."""
    import ctypes as C
    from gbnf_amd import native
    L = native.lib()
    L.gbnf_debug_trainer_last_path.argtypes = [C.c_void_p, C.POINTER(C.c_int32), C.POINTER(C.c_int32)]
    a, b = C.c_int32(), C.c_int32()
    assert L.gbnf_debug_trainer_last_path(tr.handle, C.byref(a), C.byref(b)) == 0
    return a.value, b.value


@pytest.mark.parametrize("d,h,K,n,seed,kw", [(21, 33, 3, 100, 1, {}), (6, 16, 4, 17, 2, {}), (43, 64, 2, 257, 3, {}), (21, 105, 5, 1000, 4, {}),
                                             # round 5: the other coupling networks in the reference's default training mode (BatchNorm on batch
                                             # statistics): depth 0 / 2 and ResidualNets of one and two blocks, one launch per step range
                                             (21, 105, 3, 300, 5, {"depth": 2}), (21, 105, 3, 129, 6, {"depth": 0}),
                                             (21, 105, 4, 200, 7, {"coupling_network": "residual"}),
                                             (21, 64, 3, 100, 9, {"coupling_network": "residual", "depth": 2})])
def test_trainer_batch_stats_against_oracle(d, h, K, n, seed, kw):
    import torch
    from gbnf_amd import native, synth
    from oracle import gbnf_oracle as oracle
    dev = torch.device("cuda:0")
    spec = synth.synth_realnvp_spec(d, h, K, seed=seed, flip_init=seed % 2, **kw)
    dv = _dev_spec(spec, dev)
    for st in dv["steps"]:
        if st["bn"] is not None:
            st["bn"]["batch_mean"] = torch.zeros(d, device=dev)
            st["bn"]["batch_var"] = torch.zeros(d, device=dev)
    tr = native.NativeTrainer(dv)
    assert tr.has_batch_stats
    tr.set_batch_stats(True)
    x = synth.synth_batch(n, d, seed=seed + 5)
    xd = torch.from_numpy(x).to(dev)
    z, ldj, trace = tr.forward(xd, want_trace=True)
    # round 4: the sweep runs on the register-chained kernels, one launch per step range (a range starts at every BatchNorm step:
    # steps 0 .. K-2 carry one, models/realnvp.py:71-74)
    chained = _has_live_blob(tr)          # (a width with no TRAIN variant of its own keeps the round-1 kernels: 0 chained launches)
    assert _last_path(tr)[0] == (max(K - 1, 1) if chained else 0)
    if (d, h) == (21, 105) or kw:
        assert chained                    # the HEPMASS geometry (BASELINE.json configs[2]) and every other coupling network: the fast path
    z64, ldj64, stats = oracle.component_forward_train(spec, x)
    assert np.abs(z.cpu().numpy() - z64).max() <= 2e-5 * max(1.0, float(np.abs(z64).max()))
    assert np.abs(ldj.cpu().numpy() - ldj64).max() <= 1e-5 * max(1.0, float(np.abs(ldj64).max()))
    k = 0
    for st in dv["steps"]:
        if st["bn"] is not None:
            np.testing.assert_allclose(st["bn"]["batch_mean"].cpu().numpy(), stats[k][0], rtol=0, atol=2e-6)
            np.testing.assert_allclose(st["bn"]["batch_var"].cpu().numpy(), stats[k][1], rtol=1e-5, atol=1e-6)
            k += 1
    rng = np.random.RandomState(seed)
    g_z = rng.standard_normal(x.shape).astype(np.float32)
    g_l = rng.standard_normal(n).astype(np.float32)
    gx64, grads64 = oracle.component_grads(spec, x, g_z, g_l, train=True)
    gx, grads = tr.backward(xd, torch.from_numpy(g_z).to(dev), torch.from_numpy(g_l).to(dev), want_gx=True, trace=trace)
    assert _last_path(tr)[1] == (max(K - 1, 1) if chained else 0)
    _check_grads(grads, grads64, "batch-stats", floor=0.05 * max(float(np.abs(g).max()) for g in grads64 if g is not None))
    assert np.abs(gx.cpu().numpy() - gx64).max() <= G_RTOL * float(np.abs(gx64).max())
    with pytest.raises(native.GbnfError):          # the statistics need the forward call's trace
        tr.backward(xd, torch.from_numpy(g_z).to(dev), torch.from_numpy(g_l).to(dev))
    tr.set_batch_stats(False)                      # back to running statistics: the fused single launch
    z_e, ldj_e = tr.forward(xd)
    z_r, ldj_r = oracle.component_forward(spec, x, backend="numpy64")
    assert np.abs(ldj_e.cpu().numpy() - ldj_r).max() <= 1e-5 * max(1.0, float(np.abs(ldj_r).max()))


# ---- round 3: the forward sweep on the evaluation kernel (flow_kernel_hx3<TRAIN>, device-side packing of the live parameters)
def _blob_words(fn, handle):
    import ctypes as C
    from gbnf_amd import native
    L = native.lib()
    f = getattr(L, fn)
    f.argtypes = [C.c_void_p, C.c_void_p, C.POINTER(C.c_int64)]
    f.restype = C.c_int
    n = C.c_int64()
    native._check(f(handle, None, C.byref(n)))
    buf = np.zeros(n.value, dtype=np.uint32)
    native._check(f(handle, buf.ctypes.data_as(C.c_void_p), C.byref(n)))
    return buf


@pytest.mark.parametrize("kind,d,h,kw", [("glow", 43, 215, {}), ("glow", 8, 64, {"act": "relu"}), ("glow", 21, 105, {"coupling": "additive"}),
                                         ("glow", 43, 256, {"act": "random"}), ("realnvp", 21, 105, {}),
                                         ("realnvp", 21, 105, {"coupling_network": "mixed"}), ("realnvp", 6, 30, {"batch_norm": False}),
                                         # coupling_network_depth 0 and 2 (round 5: their own stage layouts)
                                         ("glow", 43, 215, {"depth": 0}), ("glow", 43, 215, {"depth": 2}), ("glow", 43, 64, {"depth": 2}),
                                         ("realnvp", 21, 105, {"depth": 0}), ("realnvp", 21, 105, {"depth": 2}),
                                         ("realnvp", 21, 105, {"coupling_network": "residual"})])
def test_device_packer_reproduces_the_host_packer(kind, d, h, kw):
    """The live blob (device gather + split of the CURRENT parameter tensors) must be the blob gbnf_flow_create packs on the
    host from the same values: weights and biases bit for bit, the table constants (expf / sqrtf on the device) to 1 ulp-ish."""
    import torch
    from gbnf_amd import native, synth
    dev = torch.device("cuda:0")
    spec = synth.synth_boosted_specs(kind, 1, d, h, 3, seed=21, **kw)[0]
    tr = native.NativeTrainer(_dev_spec(spec, dev))
    pats = native.activation_pattern(spec)
    per_step = len(set(pats)) > 1 or (kind == "realnvp" and any(a != b for a, b in pats) and kw.get("coupling_network") != "mixed")
    flow = native.NativeFlow(spec, math="f16x3", per_step_activation=per_step)
    host = _blob_words("gbnf_debug_flow_blob", flow.handle)
    live = _blob_words("gbnf_debug_trainer_blob", tr.handle)
    assert host.shape == live.shape
    diff = np.nonzero(host != live)[0]
    if diff.size:
        a, b = host[diff].view(np.float32), live[diff].view(np.float32)
        assert np.all(np.abs(a - b) <= 6e-7 * np.maximum(np.abs(a), 1e-30) + 1e-30), (diff[:8], a[:8], b[:8])     # (expf / sqrtf of the device: a few ulp)
        assert diff.size < 0.01 * host.size            # only table constants may differ in the last bit


def _blob_pins():
    """tests/golden/make_blob_pins.py (the cases, how their blobs are built and hashed) and the JSON it wrote."""
    import importlib.util
    import json
    import os
    path = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden", "make_blob_pins.py")
    spec = importlib.util.spec_from_file_location("make_blob_pins", path)
    mod = importlib.util.module_from_spec(spec)
    spec.loader.exec_module(mod)
    with open(mod.PINS) as f:
        return mod, json.load(f)


_PINS_MOD, _PINS = _blob_pins()


@pytest.mark.parametrize("name,math", _PINS_MOD.all_keys())
def test_packed_blobs_match_their_pins(name, math):
    """The blob of the host packer (gbnf_debug_flow_blob) and of the live packer (gbnf_debug_trainer_blob) against the words recorded
    before the two packers were given one walk of the layout: every word that is a cast, a float product or a double sum bit for
    bit (SHA-256 with the table constants zeroed), the slot words exactly, the table constants (expf / sqrtf / logf: another libm
    or device math library may round differently) within 4 ulp."""
    mp = _PINS_MOD
    blobs = mp.blobs_of(name, math)
    want = {k.split("/")[2] for k in _PINS if k.startswith(f"{name}/{math}/")}
    assert set(blobs) == want and "flow" in want and (math == "bf16x6" or "trainer" in want)
    for which, words in blobs.items():
        pin, got = _PINS[f"{name}/{math}/{which}"], mp.pin_of(words)
        assert got["n_words"] == pin["n_words"], which
        assert got["sha256"] == pin["sha256"], which
        a, b = mp.table_words(got), mp.table_words(pin)
        assert a.shape == b.shape and a.size == mp.K * 321
        print(f"{name}/{math}/{which}: {int(np.count_nonzero(a != b))} of {a.size} table words differ from the pin")
        step = np.arange(a.size) % 321              # per step: the log-det constant, the in table [160], the out table [160]
        slots = ((step >= 1) & (step < 33)) | ((step >= 161) & (step < 193))
        assert np.array_equal(a[slots], b[slots]), which
        key = lambda u: np.where(u >> 31, -(u & 0x7fffffff).astype(np.int64), (u & 0x7fffffff).astype(np.int64))     # f32 bits in value order
        assert np.all(np.abs(key(a) - key(b)) <= 4), which


@pytest.mark.parametrize("kind,d,h,K,n,kw", [("glow", 43, 215, 3, 300, {"depth": 0}), ("glow", 43, 215, 3, 300, {"depth": 2}),
                                             ("glow", 43, 64, 2, 77, {"depth": 0, "coupling": "additive"}), ("glow", 43, 64, 2, 1, {"depth": 2}),
                                             ("realnvp", 21, 105, 4, 129, {"depth": 0}), ("realnvp", 21, 105, 4, 2049, {"depth": 2}),
                                             ("glow", 43, 256, 2, 65, {"depth": 2, "act": "relu"}), ("glow", 43, 250, 2, 100, {"depth": 0, "act": "random"}),
                                             ("realnvp", 21, 250, 3, 33, {"depth": 2, "coupling_network": "random"}),
                                             # one-block ResidualNets (models/layers.py:246-301, realnvp.py:57): the skip connection in both sweeps
                                             ("realnvp", 21, 105, 4, 129, {"coupling_network": "residual"}),
                                             # (seeds: a ReLU pre-activation within float32 round-off of zero -- about one case in twelve at these
                                             #  sizes -- flips one sample's path against the float64 oracle in ANY float32 implementation; tools/
                                             #  stress_train.py brackets such cases with a shifted ReLU, the fixed cases here avoid them)
                                             ("realnvp", 21, 64, 3, 100, {"coupling_network": "residual", "batch_norm": False, "seed": 101}),
                                             ("realnvp", 43, 215, 2, 2049, {"coupling_network": "residual", "seed": 101}),
                                             ("realnvp", 8, 250, 2, 1, {"coupling_network": "residual"}),
                                             # two blocks (DEPTH = 4: three middle layers in both sweeps, the skip gradient replaced behind the second block's entry)
                                             ("realnvp", 21, 105, 3, 100, {"coupling_network": "residual", "depth": 2, "seed": 104}),
                                             ("realnvp", 21, 64, 2, 33, {"coupling_network": "residual", "depth": 2, "batch_norm": False, "seed": 104}),
                                             ("realnvp", 43, 215, 2, 257, {"coupling_network": "residual", "depth": 2, "seed": 104}),
                                             ("realnvp", 8, 40, 3, 77, {"coupling_network": "residual", "depth": 2, "seed": 104}),
                                             # 16 hidden tiles with a ragged batch (n < np, spare waves in the backward's last workgroup: the shape of the
                                             #  round's fault -- HISTORY -- in an unshipped form of the depth-2 backward), one and two blocks
                                             ("realnvp", 21, 250, 3, 17, {"coupling_network": "residual", "seed": 105}),
                                             ("realnvp", 21, 250, 2, 33, {"coupling_network": "residual", "depth": 2, "seed": 105}),
                                             ("realnvp", 21, 300, 2, 65, {"coupling_network": "residual", "seed": 102}),      # 24 / 32 hidden tiles
                                             ("realnvp", 21, 512, 2, 33, {"coupling_network": "residual", "seed": 102})])
def test_depth_0_and_2_train_on_the_register_chained_kernels(kind, d, h, K, n, kw):
    """TanhNet / ReLUNet of coupling_network_depth 0 and 2 (models/layers.py:208-243, density_experiment.py:118) ran
    the round-1 per-step kernels (23 M samples/s against 51-63 M at depth 1).  Round 5: flow_kernel_hx3<..., DEPTH, TRAIN> saves the
    operands of every hidden layer and bwd_kernel_hx3<..., DEPTH> walks the transposed chain -- one launch each, gradients against the
    float64 autograd oracle, batch sizes with ragged tails and a lone row."""
    import torch
    from gbnf_amd import native, synth
    from oracle import gbnf_oracle as oracle
    dev = torch.device("cuda:0")
    kw = dict(kw)
    seed = kw.pop("seed", 71)
    spec = (synth.synth_glow_spec(d, h, K, seed=seed, **kw) if kind == "glow" else synth.synth_realnvp_spec(d, h, K, seed=seed, **kw))
    xs = synth.synth_batch(n, d, seed=72)
    rng = np.random.RandomState(73)
    g_z = rng.standard_normal(xs.shape).astype(np.float32)
    g_l = rng.standard_normal(n).astype(np.float32)
    tr = native.NativeTrainer(_dev_spec(spec, dev))
    assert _has_live_blob(tr)
    x = torch.from_numpy(xs).to(dev)
    z, ldj, trace = tr.forward(x, want_trace=True)
    z64, ldj64 = oracle.component_forward(spec, xs, backend="numpy64")
    assert np.abs(ldj.cpu().numpy() - ldj64).max() <= 1e-5 * max(1.0, float(np.abs(ldj64).max()))
    assert np.abs(z.cpu().numpy() - z64).max() <= 2e-5 * max(1.0, float(np.abs(z64).max()))
    gx64, grads64 = oracle.component_grads(spec, xs, g_z, g_l)
    gx, grads = tr.backward(x, torch.from_numpy(g_z).to(dev), torch.from_numpy(g_l).to(dev), want_gx=True, trace=trace)
    assert _last_path(tr) == (1, 1)                        # one launch of the chained forward, one of the chained backward
    _check_grads(grads, grads64, f"{kind} d={d} h={h} K={K} n={n} {kw}")
    assert np.abs(gx.cpu().numpy() - gx64).max() <= G_RTOL * max(float(np.abs(gx64).max()), 1e-3)
    # 32-sample waves of the forward sweep (what large batches run)
    native.tuning_set("force_nt", 2)
    try:
        z2, ldj2, trace2 = tr.forward(x, want_trace=True)
        gx2, grads2 = tr.backward(x, torch.from_numpy(g_z).to(dev), torch.from_numpy(g_l).to(dev), want_gx=True, trace=trace2)
        torch.cuda.synchronize()
    finally:
        native.tuning_set("force_nt", 0)
    assert np.abs(z2.cpu().numpy() - z64).max() <= 2e-5 * max(1.0, float(np.abs(z64).max()))
    _check_grads(grads2, grads64, f"{kind} d={d} h={h} NT=2")


@pytest.mark.parametrize("kind,d,h,K,n,kw", [("glow", 8, 40, 3, 77, {"act": "relu"}), ("glow", 63, 315, 2, 100, {}), ("glow", 21, 50, 2, 33, {"depth": 2}),
                                             ("realnvp", 13, 33, 3, 65, {"coupling_network": "relu"}), ("realnvp", 21, 150, 2, 40, {"coupling_network": "residual", "seed": 103})])
def test_a_width_without_a_variant_of_its_own_trains_on_the_next_wider_one(kind, d, h, K, n, kw):
    """h = 40 with ReLU nets has no kernel variant of its own width (the nearest compiled one has 64 hidden rows); BSDS300 at the
    reference's h = 5 D = 315 has 320 rows against 384.  Rounds 3-4 kept such flows on the round-1 kernels (the register-chained sweeps
    save a row per hidden unit of their COMPILED width).  Round 5: the trainer sizes its operand workspace by the variant (the extra
    units have zero weights: zero activations, zero gradients, zero operand rows) -- gradients against the float64 oracle, the chained
    kernels asserted."""
    import torch
    from gbnf_amd import native, synth
    from oracle import gbnf_oracle as oracle
    dev = torch.device("cuda:0")
    kw = dict(kw)
    seed = kw.pop("seed", 21)
    spec = (synth.synth_glow_spec(d, h, K, seed=seed, **kw) if kind == "glow" else synth.synth_realnvp_spec(d, h, K, seed=seed, **kw))
    tr = native.NativeTrainer(_dev_spec(spec, dev))
    assert _has_live_blob(tr)
    xs = synth.synth_batch(n, d, seed=22)
    rng = np.random.RandomState(23)
    g_z = rng.standard_normal(xs.shape).astype(np.float32)
    g_l = rng.standard_normal(n).astype(np.float32)
    x = torch.from_numpy(xs).to(dev)
    z64, ldj64 = oracle.component_forward(spec, xs, backend="numpy64")
    gx64, grads64 = oracle.component_grads(spec, xs, g_z, g_l)
    z, ldj, trace = tr.forward(x, want_trace=True)
    gx, grads = tr.backward(x, torch.from_numpy(g_z).to(dev), torch.from_numpy(g_l).to(dev), want_gx=True, trace=trace)
    assert _last_path(tr) == (1, 1)
    assert np.abs(z.cpu().numpy() - z64).max() <= 2e-5 * max(1.0, float(np.abs(z64).max()))
    _check_grads(grads, grads64, f"{kind} d={d} h={h} {kw}")
    assert np.abs(gx.cpu().numpy() - gx64).max() <= G_RTOL * max(float(np.abs(gx64).max()), 1e-3)
    # the per-step kernels (an untraced forward, a backward without a trace) work on the widened rows too
    z0, ldj0 = tr.forward(x)
    assert np.abs(z0.cpu().numpy() - z64).max() <= 2e-5 * max(1.0, float(np.abs(z64).max()))
    gx0, grads0 = tr.backward(x, torch.from_numpy(g_z).to(dev), torch.from_numpy(g_l).to(dev), want_gx=True)
    _check_grads(grads0, grads64, f"{kind} d={d} h={h} {kw} (per-step kernels)")


def test_long_flows_fall_back_for_the_backward_sweep_only():
    """K = 14 > the 12 steps whose tables the backward kernel keeps in LDS: the traced forward still runs on the register-chained
    kernel (tables read from the blob), the backward on the round-1 kernels -- gradients against the float64 oracle."""
    import torch
    from gbnf_amd import native, synth
    from oracle import gbnf_oracle as oracle
    dev = torch.device("cuda:0")
    spec = synth.synth_boosted_specs("glow", 1, 8, 32, 14, seed=5)[0]
    tr = native.NativeTrainer(_dev_spec(spec, dev))
    rng = np.random.RandomState(3)
    xs = synth.synth_batch(300, 8, seed=6)
    x = torch.from_numpy(xs).to(dev)
    g_z = rng.standard_normal(xs.shape).astype(np.float32)
    g_l = rng.standard_normal(xs.shape[0]).astype(np.float32)
    z64, ldj64 = oracle.component_forward(spec, xs, backend="numpy64")
    gx64, grads64 = oracle.component_grads(spec, xs, g_z, g_l)
    z, ldj, trace = tr.forward(x, want_trace=True)
    assert rel_err(ldj.cpu().numpy(), ldj64) < 1e-5
    assert np.abs(z.cpu().numpy() - z64).max() <= 1e-5 * max(1.0, float(np.abs(z64).max()))
    gx, grads = tr.backward(x, torch.from_numpy(g_z).to(dev), torch.from_numpy(g_l).to(dev), want_gx=True, trace=trace)
    _check_grads(grads, grads64, "K=14")
    assert np.abs(gx.cpu().numpy() - gx64).max() <= G_RTOL * float(np.abs(gx64).max())


@pytest.mark.parametrize("kind,d,h,n", [("glow", 43, 215, 4096), ("glow", 43, 215, 77), ("realnvp", 21, 105, 2000)])
def test_fast_forward_writes_what_the_backward_needs(kind, d, h, n):
    """z / ldj / trace of the new forward sweep against the round-1 training kernel on the same live parameters, and the
    saved operands (net inputs, hidden activations, net outputs) against the float64 oracle's intermediate values."""
    import torch
    from gbnf_amd import native, synth
    dev = torch.device("cuda:0")
    spec = synth.synth_boosted_specs(kind, 1, d, h, 3, seed=8)[0]
    tr = native.NativeTrainer(_dev_spec(spec, dev))
    x = torch.from_numpy(synth.synth_batch(n, d, seed=9)).to(dev)
    z, ldj, trace = tr.forward(x, want_trace=True)
    z0, ldj0 = tr.forward(x)                                  # no trace requested: the round-1 kernel
    assert rel_err(ldj.cpu().numpy(), ldj0.cpu().numpy()) < 4e-6            # two f32 summation orders of the same products
    np.testing.assert_allclose(z.cpu().numpy(), z0.cpu().numpy(), rtol=0, atol=2e-5 * max(1.0, float(z0.abs().max())))
    from oracle import gbnf_oracle as oracle
    zr, lr = oracle.component_forward(spec, x.cpu().numpy())
    assert rel_err(ldj.cpu().numpy(), lr) < 1e-5


@pytest.mark.gpu
@pytest.mark.parametrize("kind,d,h,K", [("glow", 43, 215, 5), ("realnvp", 21, 105, 5)])
def test_weight_gradients_are_additive_over_the_batch_at_full_size(kind, d, h, K):
    """Size-independent property at BASELINE's N = 65536 (at K = 5 the float64 oracle's backward pass of that size takes more than
    the few seconds a test has; up to 32 k rows at K <= 5 it does not: tests/test_hip_train_large_batch.py compares the launch forms
    of large batches with the oracle itself): with
    fixed normalisation statistics the parameter gradients of a batch are the SUM of the gradients of its parts.  One call on
    65536 rows (wgrad_kernel: 8-wave blocks, 32 sample chunks per block column, two k-steps of loads in flight, float atomics)
    against eight calls on 8192 rows each (other chunk counts, other block counts per CU), and g_x row for row."""
    import torch
    from gbnf_amd import native, synth
    dev = torch.device("cuda:0")
    spec = synth.synth_glow_spec(d, h, K, seed=31) if kind == "glow" else synth.synth_realnvp_spec(d, h, K, seed=31)
    n, parts = 65536, 8
    x = torch.from_numpy(synth.synth_batch(n, d, seed=32)).to(dev)
    gen = torch.Generator(device="cpu").manual_seed(33)
    g_z = torch.randn(n, d, generator=gen).to(dev)
    g_l = torch.randn(n, generator=gen).to(dev)
    tr = native.NativeTrainer(_dev_spec(spec, dev))
    _, _, trace = tr.forward(x, want_trace=True)
    gx_full, grads_full = tr.backward(x, g_z, g_l, want_gx=True, trace=trace)
    grads_full = [None if g is None else g.double().cpu() for g in grads_full]
    gx_full = gx_full.cpu()
    acc = [None if g is None else torch.zeros_like(g) for g in grads_full]
    m = n // parts
    for p in range(parts):
        sl = slice(p * m, (p + 1) * m)
        xp = x[sl].contiguous()
        _, _, tp = tr.forward(xp, want_trace=True)
        gx, grads = tr.backward(xp, g_z[sl].contiguous(), g_l[sl].contiguous(), want_gx=True, trace=tp)
        for a, g in zip(acc, grads):
            if g is not None:
                a += g.double().cpu()
        assert (gx.cpu() - gx_full[sl]).abs().max() <= 1e-5 * max(1.0, float(gx_full[sl].abs().max()))
    for k, (a, b) in enumerate(zip(acc, grads_full)):
        if b is None:
            continue
        scale = max(float(b.abs().max()), 1e-3)
        assert float((a - b).abs().max()) <= G_RTOL * scale, f"{kind}: gradient {k} shape {tuple(b.shape)}: {float((a - b).abs().max())} vs scale {scale}"


@pytest.mark.parametrize("d,h,K,n,blocks", [(43, 215, 2, 129, 1), (21, 64, 3, 77, 2), (8, 250, 2, 33, 1)])
def test_a_glow_residualnet_descriptor_keeps_the_per_step_trainer(d, h, K, n, blocks):
    """gbnf.h is a public ABI, and a Glow descriptor whose coupling net is a ResidualNet -- a combination the
    Python front end rejects and the reference cannot construct -- used to be matched to the per-step-activation
    TRAIN variants, which have no skip connection: silently wrong values and gradients.  live_choose now refuses (no act-2 TRAIN
    variant exists for kind GLOW), so the trainer keeps the round-1 per-step kernels: no live blob, forward and gradients
    against the float64 oracle."""
    import torch
    from gbnf_amd import native, synth
    from oracle import gbnf_oracle as oracle
    dev = torch.device("cuda:0")
    spec = synth.synth_glow_spec(d, h, K, seed=31)
    rng = np.random.RandomState(32)
    for st in spec["steps"]:
        st["net"] = synth._res_net(rng, d // 2, 2 * (d - d // 2), h, blocks, 1.0)
    xs = synth.synth_batch(n, d, seed=33)
    g_z = rng.standard_normal(xs.shape).astype(np.float32)
    g_l = rng.standard_normal(n).astype(np.float32)
    tr = native.NativeTrainer(_dev_spec(spec, dev))
    assert not _has_live_blob(tr)
    x = torch.from_numpy(xs).to(dev)
    z, ldj, trace = tr.forward(x, want_trace=True)
    z64, ldj64 = oracle.component_forward(spec, xs, backend="numpy64")
    assert np.abs(ldj.cpu().numpy() - ldj64).max() <= 1e-5 * max(1.0, float(np.abs(ldj64).max()))
    assert np.abs(z.cpu().numpy() - z64).max() <= 2e-5 * max(1.0, float(np.abs(z64).max()))
    gx64, grads64 = oracle.component_grads(spec, xs, g_z, g_l)
    gx, grads = tr.backward(x, torch.from_numpy(g_z).to(dev), torch.from_numpy(g_l).to(dev), want_gx=True, trace=trace)
    assert _last_path(tr) == (0, 0)
    _check_grads(grads, grads64, f"glow residual d={d} h={h} K={K} n={n}")
    assert np.abs(gx.cpu().numpy() - gx64).max() <= G_RTOL * max(float(np.abs(gx64).max()), 1e-3)


@pytest.mark.parametrize("kind,d,h,K,n", [("glow", 21, 64, 16, 100), ("realnvp", 8, 40, 20, 65)])
def test_flows_of_more_than_twelve_steps_train_on_the_chained_kernels(kind, d, h, K, n):
    """the chained backward sweep keeps every step's tables in LDS and refused K > 12 (LDS_TABLE_STEPS); such flows
    fell back to the round-1 per-step kernels.  Round 6: 24 steps of tables (32 KB) -- one launch each way asserted, gradients against
    the float64 autograd oracle."""
    import torch
    from gbnf_amd import native, synth
    from oracle import gbnf_oracle as oracle
    dev = torch.device("cuda:0")
    spec = (synth.synth_glow_spec(d, h, K, seed=41, gain=0.5) if kind == "glow" else synth.synth_realnvp_spec(d, h, K, seed=41, gain=0.5))
    xs = synth.synth_batch(n, d, seed=42)
    rng = np.random.RandomState(43)
    g_z = rng.standard_normal(xs.shape).astype(np.float32)
    g_l = rng.standard_normal(n).astype(np.float32)
    tr = native.NativeTrainer(_dev_spec(spec, dev))
    assert _has_live_blob(tr)
    x = torch.from_numpy(xs).to(dev)
    z, ldj, trace = tr.forward(x, want_trace=True)
    z64, ldj64 = oracle.component_forward(spec, xs, backend="numpy64")
    assert np.abs(ldj.cpu().numpy() - ldj64).max() <= 1e-5 * max(1.0, float(np.abs(ldj64).max()))
    assert np.abs(z.cpu().numpy() - z64).max() <= 2e-5 * max(1.0, float(np.abs(z64).max()))
    gx64, grads64 = oracle.component_grads(spec, xs, g_z, g_l)
    gx, grads = tr.backward(x, torch.from_numpy(g_z).to(dev), torch.from_numpy(g_l).to(dev), want_gx=True, trace=trace)
    assert _last_path(tr) == (1, 1)
    _check_grads(grads, grads64, f"{kind} K={K}")
    assert np.abs(gx.cpu().numpy() - gx64).max() <= G_RTOL * max(float(np.abs(gx64).max()), 1e-3)


def test_leaving_training_mode_reports_saturated_training_kernels():
    """The training kernels saturate a split-f16 operand beyond +-65504 (include/gbnf.h, gbnf_saturation_count: no repair pass in
    training) -- finite steps with wrong gradients.  The module looks at the library's counter where the reference's loop switches
    modes anyway (density_experiment.py:336 / :545): model.eval() after a healthy epoch is silent, after a blown one it warns."""
    import warnings
    import torch
    from gbnf_amd import BoostedFlow, native
    dev = torch.device("cuda:0")
    torch.manual_seed(3)
    m = BoostedFlow(_args("glow", 8, 32, 3, 1, dev, act="relu")).to(dev)
    x = torch.randn(256, 8, device=dev)

    def epoch():
        m.train()
        z, _, _, ldj, _ = m(x=x, components=0)
        loss = torch.mean(-(torch.sum(-0.5 * np.log(2 * np.pi) - 0.5 * z.pow(2), dim=-1) + ldj))
        loss.backward()
        return float(loss.detach())

    native.saturation_count(reset=True)
    assert np.isfinite(epoch())
    # an EVALUATION launch on out-of-range rows between train() and eval() (the boosting weights of fixed components do that): marked,
    # repaired in the same call, counted as evaluation -- not the training kernels' count, nothing to report
    xbig = x.clone()
    xbig[3] = 3.0e5
    with torch.no_grad():
        m.log_prob(xbig, n_used=1)
    assert native.saturation_count() > 0 and native.training_saturation_count() == 0
    with warnings.catch_warnings():
        warnings.simplefilter("error")
        m.eval()                                   # healthy training: nothing to report
    native.saturation_count(reset=True)
    with torch.no_grad():                          # a ReLU net that has blown up: weights of a few hundred, second-layer activations ~1e6
        m.flows[0].flow.layers[0].block.network[0].weight.mul_(2000.0)
        m.flows[0].flow.layers[0].block.network[2].weight.mul_(2000.0)
    epoch()
    with pytest.warns(RuntimeWarning, match="65504"):
        m.eval()
    with warnings.catch_warnings():                # reported once per training period
        warnings.simplefilter("error")
        m.eval()
    assert native.training_saturation_count() > 0 and native.saturation_count(reset=True) >= native.training_saturation_count()
    assert native.training_saturation_count() == 0      # (saturation_count is the sum and resets both parts)
    # WEIGHTS beyond the fp16 range cannot be split at all (hi rounds to inf, the residual to -inf, a ReLU of their NaN is 0: a finite,
    # wrong step): the device packer counts them like every other operand that leaves the range
    with torch.no_grad():
        m.flows[0].flow.layers[0].block.network[0].weight.mul_(1e5)
    epoch()
    with pytest.warns(RuntimeWarning, match="65504"):
        m.eval()
    native.saturation_count(reset=True)                 # (left clean for the other tests)


@pytest.mark.parametrize("kind,d,h,K,n", [("glow", 8, 40, 26, 65), ("realnvp", 6, 30, 27, 100)])
def test_flows_of_more_than_twenty_four_steps_train_behind_the_chained_limit(kind, d, h, K, n):
    """K > LDS_TABLE_STEPS (24): the chained backward sweep refuses (its tables live in LDS), the traced forward reads its tables from
    global memory, and the backward runs on the round-1 per-step kernels (bwd path 0).  Gradients against the float64 autograd oracle."""
    import torch
    from gbnf_amd import native, synth
    from oracle import gbnf_oracle as oracle
    dev = torch.device("cuda:0")
    spec = (synth.synth_glow_spec(d, h, K, seed=51, gain=0.5) if kind == "glow" else synth.synth_realnvp_spec(d, h, K, seed=51, gain=0.5))
    xs = synth.synth_batch(n, d, seed=52)
    rng = np.random.RandomState(53)
    g_z = rng.standard_normal(xs.shape).astype(np.float32)
    g_l = rng.standard_normal(n).astype(np.float32)
    tr = native.NativeTrainer(_dev_spec(spec, dev))
    x = torch.from_numpy(xs).to(dev)
    z, ldj, trace = tr.forward(x, want_trace=True)
    z64, ldj64 = oracle.component_forward(spec, xs, backend="numpy64")
    assert np.abs(ldj.cpu().numpy() - ldj64).max() <= 1e-5 * max(1.0, float(np.abs(ldj64).max()))
    assert np.abs(z.cpu().numpy() - z64).max() <= 2e-5 * max(1.0, float(np.abs(z64).max()))
    gx64, grads64 = oracle.component_grads(spec, xs, g_z, g_l)
    gx, grads = tr.backward(x, torch.from_numpy(g_z).to(dev), torch.from_numpy(g_l).to(dev), want_gx=True, trace=trace)
    assert _last_path(tr)[1] == 0                       # the backward sweep: per-step kernels
    _check_grads(grads, grads64, f"{kind} K={K}")
    assert np.abs(gx.cpu().numpy() - gx64).max() <= G_RTOL * max(float(np.abs(gx64).max()), 1e-3)
    gx2, grads2 = tr.backward(x, torch.from_numpy(g_z).to(dev), torch.from_numpy(g_l).to(dev), want_gx=True, trace=None)
    _check_grads(grads2, grads64, f"{kind} K={K} (no trace)")
