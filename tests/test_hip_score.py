"""GPU: the score of the tabular path -- gbnf_trainer_backward_x, gbnf_score_seed, gbnf_mixture_score and BoostedFlow.score /
component_score / responsibilities -- against gbnf_trainer_backward (bit for bit) and the float64 yardstick tests/score_oracle.py.

Bars, none of them new: ll and G 1e-5 relative (BASELINE); r within eps = 1e-5 max(1, max|ll64|) (a softmax moves by at most
eps / 2 under an eps perturbation of its logits, to first order: twice that); g_x within G_RTOL = 2e-4 of sum_c max|g64_c|, the
yardstick's terms on the DEVICE's r (the backward is linear in its seeds, every component carries tests/test_hip_train.py's bar)."""
import argparse
import ctypes

import numpy as np
import pytest

from conftest import GRADS_CASES, load_grads_case, rel_err
import score_oracle

pytestmark = pytest.mark.gpu
G_RTOL = 2e-4

CASES = ["g6_glow_d43_h64_n1", "g6_glow_d43_h64_n77", "g6_realnvp_d21_h64_n33", "g6_glow_d43_h64_c3_rho", "g5_glow_d6_h30_c2",
         "g5_glow_d43_h64_c2_additive", "g5_glow_d43_h64_c2_depth0", "g5_glow_d43_h64_c2_depth2", "g5_glow_d43_h64_c2_reverse_relu",
         "g4_realnvp_d21_h105_c2_mixed", "g4_realnvp_d21_h105_c8", "g1_toy_realnvp_c2"]


def _dev_spec(spec, dev):
    """flow spec (numpy) -> device spec (CUDA tensors) for native.NativeTrainer."""
    import torch
    t = lambda a: torch.from_numpy(np.ascontiguousarray(a, dtype=np.float32)).to(dev)
    net = lambda n: {"act": n["act"], "layers": [(t(w), t(b)) for w, b in n["layers"]]}
    out = {"kind": spec["kind"], "d": spec["d"], "coupling": spec.get("coupling"), "steps": []}
    for st in spec["steps"]:
        if spec["kind"] == "glow":
            out["steps"].append({"an_bias": t(st["an_bias"]), "an_logs": t(st["an_logs"]), "perm": st["perm"], "net": net(st["net"])})
        else:
            bn = st["bn"]
            out["steps"].append({"flipped": st["flipped"],
                                 "bn": None if bn is None else {**{k: t(bn[k]) for k in ("log_gamma", "beta", "running_mean",
                                                                                         "running_var")}, "eps": bn["eps"]},
                                 "t_net": net(st["t_net"]), "s_net": net(st["s_net"])})
    return out


def _args(cfg, dev, C=None):
    skw = cfg.get("synth_kw", {})
    return argparse.Namespace(
        num_flows=cfg["K"], z_size=cfg["d"], density_evaluation=True, device=dev, cuda=True, component_type=cfg["kind"],
        num_components=cfg["C"] if C is None else C, rho_init="decreasing", learn_top=False, y_classes=0, y_condition=False, sample_size=4,
        input_size=[cfg["d"]], h_size=cfg["h"], num_blocks=1, actnorm_scale=1.0, flow_permutation=skw.get("permutation", "shuffle"),
        flow_coupling=skw.get("coupling", "affine"), LU_decomposed=False, num_dequant_blocks=0,
        coupling_network="random" if "activations" in cfg else skw.get("act", skw.get("coupling_network", "tanh")),
        coupling_network_depth=skw.get("depth", 1), batch_norm=skw.get("batch_norm", True))


def _model_from_case(g, dev):
    import torch
    from gbnf_amd import BoostedFlow
    if "activations" in g.cfg:     # `--coupling_network random`: the constructor draws from numpy's global RNG
        np.random.seed(13)
    m = BoostedFlow(_args(g.cfg, dev))
    for c, spec in enumerate(g.specs):
        m.load_spec(c, spec)
    with torch.no_grad():
        m.rho.copy_(torch.from_numpy(g.rho).to(dev))
    m.eval()
    return m


_FWD64 = {}


def _forward64(g, base):
    """The float64 forward half of a fixture's mixture, computed once per (fixture, base) and left unchanged."""
    key = (g.name, base is not None)
    if key not in _FWD64:
        _FWD64[key] = score_oracle.mixture64(g.specs[: g.n_used], g.rho, g.x, base)
    return _FWD64[key]


def _check_against_float64(g, base, g_x, G, r, ll, what):
    """The four bars of the module docstring; ``ll`` None: not judged (the call made its own table)."""
    specs = g.specs[: g.n_used]
    zs, ll64, r64, G64 = _forward64(g, base)
    r_dev = r.cpu().numpy().astype(np.float64)
    if ll is not None:
        e = rel_err(ll.cpu().numpy(), ll64)
        print(f"{what}: ll rel_err {e:.2e}")
        assert e < 1e-5
    e = rel_err(G.cpu().numpy(), G64)
    eps = 1e-5 * max(1.0, float(np.abs(ll64).max()))
    dr = float(np.abs(r_dev - r64).max())
    print(f"{what}: G rel_err {e:.2e}, |dr| {dr:.2e} (eps {eps:.2e})")
    assert e < 1e-5
    assert dr <= eps
    terms = score_oracle.score_terms64(specs, g.x, zs, r_dev, base)
    bar = G_RTOL * float(sum(np.abs(t).max() for t in terms))
    dg = float(np.abs(g_x.cpu().numpy() - terms.sum(axis=0)).max())
    print(f"{what}: |g_x - g64| {dg:.2e} (bar {bar:.2e})")
    assert dg <= bar
    return bar


# ---- 1. backward_x against backward --------------------------------------------------------------------------------------
def _upstream(shape, dev, seed=7):
    import torch
    rng = np.random.RandomState(seed)
    return (torch.from_numpy(rng.standard_normal(shape).astype(np.float32)).to(dev),
            torch.from_numpy(rng.standard_normal(shape[0]).astype(np.float32)).to(dev))


def _assert_backward_x_equals_backward(tr, x, what):
    import torch
    g_z, g_l = _upstream(tuple(x.shape), x.device)
    for traced in (False, True):
        trace = tr.forward(x, want_trace=True)[2] if traced else None
        full = tr.backward(x, g_z, g_l, want_gx=True, trace=trace)[0]
        trace = tr.forward(x, want_trace=True)[2] if traced else None       # (one trace buffer serves one forward + one backward)
        only = tr.backward_x(x, g_z, g_l, trace=trace)
        assert bool(torch.isfinite(full).all())
        assert torch.equal(only, full), f"{what}, trace={traced}: g_x of backward_x differs from backward's"
    # null upstream gradients are zeros, as in backward
    assert torch.equal(tr.backward_x(x, None, g_l), tr.backward(x, None, g_l, want_gx=True)[0])
    # accumulate: onto a pre-filled tensor, against the stored result plus the fill, to 1 ulp of the sum
    stored = tr.backward_x(x, g_z, g_l)
    fill = torch.full_like(x, 0.37) + x
    acc = tr.backward_x(x, g_z, g_l, g_x=fill.clone())
    want = (fill + stored).cpu().numpy()
    assert np.all(np.abs(acc.cpu().numpy() - want) <= np.spacing(np.abs(want)))


@pytest.mark.parametrize("math", ["f16x3", "bf16x6", "repair"])
@pytest.mark.parametrize("name", ["g6_glow_d43_h64_n77", "g6_realnvp_d21_h64_n33", "g6_glow_d43_h64_n1"])
def test_backward_x_is_backward_without_the_weight_gradients(name, math, golden_case):
    import torch
    from gbnf_amd import native
    dev = torch.device("cuda:0")
    g = golden_case(name)
    tr = native.NativeTrainer(_dev_spec(g.specs[0], dev), math=math)
    _assert_backward_x_equals_backward(tr, torch.from_numpy(g.x).to(dev), f"{name} {math}")


def test_backward_x_of_a_repairing_trainer_whose_call_is_re_run():
    """Rows beyond the fp16 range: the bf16x6 form is the one that counts, for g_x as for the gradients."""
    import torch
    from gbnf_amd import native, synth
    dev = torch.device("cuda:0")
    spec = synth.synth_glow_spec(43, 215, 5, seed=3)
    x = synth.synth_batch(200, 43, seed=4)
    x[7, :] = 3.0e5
    tr = native.NativeTrainer(_dev_spec(spec, dev), math="repair")
    tr.repair_count(reset=True)
    _assert_backward_x_equals_backward(tr, torch.from_numpy(x).to(dev), "repair, out of range")
    assert tr.repair_count() > 0


@pytest.mark.parametrize("name", ["g6_glow_d43_h64_n77", "g6_realnvp_d21_h64_n33"])
def test_backward_x_on_32_sample_waves(name, golden_case):
    import torch
    from gbnf_amd import native
    dev = torch.device("cuda:0")
    g = golden_case(name)
    tr = native.NativeTrainer(_dev_spec(g.specs[0], dev))
    native.tuning_set("force_nt", 2)
    try:
        _assert_backward_x_equals_backward(tr, torch.from_numpy(g.x).to(dev), f"{name} NT=2")
        torch.cuda.synchronize()
    finally:
        native.tuning_set("force_nt", 0)


def test_backward_x_in_deterministic_mode_keeps_backwards_refusals(golden_case):
    import torch
    from gbnf_amd import native
    dev = torch.device("cuda:0")
    g = golden_case("g6_glow_d43_h64_n77")
    tr = native.NativeTrainer(_dev_spec(g.specs[0], dev), deterministic=True)
    x = torch.from_numpy(g.x).to(dev)
    g_z, g_l = _upstream(tuple(x.shape), dev)
    with pytest.raises(native.GbnfError, match="deterministic"):        # f16x3 without the trace: the per-step kernels
        tr.backward_x(x, g_z, g_l)
    full = tr.backward(x, g_z, g_l, want_gx=True, trace=tr.forward(x, want_trace=True)[2])[0]
    assert torch.equal(tr.backward_x(x, g_z, g_l, trace=tr.forward(x, want_trace=True)[2]), full)


# ---- gbnf_score_seed ---------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("n,d,misalign", [(1, 43, 0), (77, 43, 0), (300, 21, 0), (64, 6, 0), (77, 43, 1), (257, 3, 3)])
def test_score_seed_matches_float64(n, d, misalign):
    """One row, ragged waves, more than one workgroup (256 rows each), and arrays off the 16-byte grid (the per-element form)."""
    import torch
    from gbnf_amd import native
    dev = torch.device("cuda:0")
    rng = np.random.RandomState(n + d)
    z = rng.standard_normal((n, d)).astype(np.float32) * 2
    r = rng.uniform(0.0, 1.0, n).astype(np.float32)
    mean = rng.standard_normal(d).astype(np.float32)
    std = rng.uniform(0.5, 3.0, d).astype(np.float32)
    buf = torch.zeros(n * d + 4, dtype=torch.float32, device=dev)
    zd = buf[misalign: misalign + n * d].view(n, d)
    zd.copy_(torch.from_numpy(z))
    t = lambda a: torch.from_numpy(a).to(dev)
    z64 = z.astype(np.float64)
    for base in (None, (mean, std)):
        m64, s64 = (np.zeros(d), np.ones(d)) if base is None else (mean.astype(np.float64), std.astype(np.float64))
        for rr in (None, r):
            g_z, g_ldj, ll = native.score_seed(zd, r=None if rr is None else t(rr), base=None if base is None else (t(mean), t(std)),
                                               want_ll=True)
            r64 = np.ones(n) if rr is None else rr.astype(np.float64)
            gz64 = -r64[:, None] * (z64 - m64) / (s64 * s64)
            ll64 = np.sum(-(z64 - m64) ** 2 / (2 * s64 * s64) - np.log(s64) - 0.5 * np.log(2 * np.pi), axis=1)
            assert np.abs(g_z.cpu().numpy() - gz64).max() <= 1e-6 * max(1.0, float(np.abs(gz64).max()))
            assert np.array_equal(g_ldj.cpu().numpy(), r64.astype(np.float32))
            assert rel_err(ll.cpu().numpy(), ll64) < 1e-6
    a, b = native.score_seed(zd), native.tabular_score_seed(zd)          # without ll: (g_z, g_ldj); the explicit entry point
    assert len(a) == 2 and len(b) == 2 and torch.equal(a[0], b[0]) and torch.equal(a[1], b[1])
    with pytest.raises(native.GbnfError):
        native.tabular_score_seed(zd.view(n, d, 1, 1))


# ---- 2. mixture_score and BoostedFlow.score ----------------------------------------------------------------------------------
@pytest.mark.parametrize("name", CASES)
def test_mixture_score_matches_float64(name, golden_case):
    import torch
    from gbnf_amd import native
    dev = torch.device("cuda:0")
    g = golden_case(name)
    specs = g.specs[: g.n_used]
    x = torch.from_numpy(g.x).to(dev)
    trainers = [native.NativeTrainer(_dev_spec(sp, dev)) for sp in specs]
    log_w = torch.from_numpy(score_oracle.log_weights64(g.rho, len(specs)).astype(np.float32)).to(dev)
    base = None if g.base is None else tuple(torch.from_numpy(np.ascontiguousarray(a, dtype=np.float32)).to(dev) for a in g.base)
    mix, _flows = native.mixture_from_specs(specs)
    if g.base is not None:
        mix.set_base(*g.base)
    table = mix.component_log_prob(x)
    g_x, G, r = native.mixture_score(trainers, log_w, x, ll=table, base=base, want_r=True)
    bar = _check_against_float64(g, g.base, g_x, G, r, table, f"{name} with the table")
    g_x2, G2, r2 = native.mixture_score(trainers, log_w, x, base=base, want_r=True)
    _check_against_float64(g, g.base, g_x2, G2, r2, None, f"{name} without it")
    assert float((g_x - g_x2).abs().max()) <= bar
    assert native.mixture_score(trainers, log_w, x, ll=table, base=base)[2] is None
    for t_ in trainers:
        assert not t_.batch_stats


@pytest.mark.parametrize("math", ["bf16x6", "repair"])
@pytest.mark.parametrize("name", ["g6_glow_d43_h64_c3_rho", "g6_realnvp_d21_h64_n33"])
def test_mixture_score_on_range_safe_and_repairing_trainers(name, math, golden_case):
    """The same call on the other two math modes: the g_x pair of a repairing trainer inside the call's workspace, its re-run flag
    keyed to the ONE trace buffer every component shares, the table forward that writes that buffer; twice, bit-equal."""
    import torch
    from gbnf_amd import native
    dev = torch.device("cuda:0")
    g = golden_case(name)
    specs = g.specs[: g.n_used]
    x = torch.from_numpy(g.x).to(dev)
    trainers = [native.NativeTrainer(_dev_spec(sp, dev), math=math) for sp in specs]
    log_w = torch.from_numpy(score_oracle.log_weights64(g.rho, len(specs)).astype(np.float32)).to(dev)
    table = native.mixture_from_specs(specs)[0].component_log_prob(x)
    g_x, G, r = native.mixture_score(trainers, log_w, x, ll=table, want_r=True)
    bar = _check_against_float64(g, None, g_x, G, r, table, f"{name} {math} with the table")
    g_x2, G2, r2 = native.mixture_score(trainers, log_w, x, want_r=True)
    _check_against_float64(g, None, g_x2, G2, r2, None, f"{name} {math} without it")
    assert float((g_x - g_x2).abs().max()) <= bar
    again = native.mixture_score(trainers, log_w, x, want_r=True)
    for u, v in zip((g_x2, G2, r2), again):
        assert torch.equal(u, v)
    lone = native.mixture_score(trainers[:1], torch.zeros(1, device=dev), x)          # a lone component, no table
    assert rel_err(lone[1].cpu().numpy(), _forward64(g, None)[1][0]) < 1e-5


def test_mixture_score_of_repairing_trainers_whose_calls_are_re_run():
    """A row beyond the fp16 range: every component's forward and backward_x are re-run in bf16x6 inside the one call (the re-run
    flag of each forward is keyed to the one shared trace buffer), and the result meets the bars of the in-range cases."""
    import types
    import torch
    from gbnf_amd import native, synth
    dev = torch.device("cuda:0")
    xs = synth.synth_batch(200, 43, seed=4)
    xs[7, :] = 3.0e5
    g = types.SimpleNamespace(name="repair_out_of_range", specs=synth.synth_boosted_specs("glow", 2, 43, 215, 5, seed=3), n_used=2,
                              rho=np.array([0.4, 0.6]), x=xs)
    x = torch.from_numpy(xs).to(dev)
    log_w = torch.from_numpy(score_oracle.log_weights64(g.rho, 2).astype(np.float32)).to(dev)
    rep = [native.NativeTrainer(_dev_spec(sp, dev), math="repair") for sp in g.specs]
    for t_ in rep:
        t_.repair_count(reset=True)
    g_x, G, r = native.mixture_score(rep, log_w, x, want_r=True)
    assert all(t_.repair_count() > 0 for t_ in rep)
    assert bool(torch.isfinite(g_x).all()) and bool(torch.isfinite(G).all())
    _check_against_float64(g, None, g_x, G, r, None, "repairing trainers, a row out of range")


@pytest.mark.parametrize("name", CASES)
def test_module_score_matches_float64(name, golden_case):
    """BoostedFlow.score: base N(0, I) as ``log_prob`` (the toy fixture too: its components under the standard base)."""
    import torch
    dev = torch.device("cuda:0")
    g = golden_case(name)
    m = _model_from_case(g, dev)
    x = torch.from_numpy(g.x).to(dev)
    g_x, G, r = m.score(x, n_used=g.n_used, return_log_prob=True, return_responsibilities=True)
    assert tuple(g_x.shape) == tuple(x.shape) and tuple(G.shape) == (x.shape[0],) and tuple(r.shape) == (x.shape[0], g.n_used)
    ll = m.component_log_prob(x, n_used=g.n_used)
    _check_against_float64(g, None, g_x, G, r.t().contiguous(), ll.t().contiguous(), f"{name} module")
    assert rel_err(G.cpu().numpy(), m.log_prob(x, n_used=g.n_used).cpu().numpy()) < 1e-5        # the closed form against the recursion
    assert torch.equal(m.score(x, n_used=g.n_used), g_x)


# ---- 3. component_score -----------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("name", GRADS_CASES)
def test_component_score_is_the_references_gradient(name):
    import torch
    from gbnf_amd import BoostedFlow
    dev = torch.device("cuda:0")
    cfg, spec, x, nll, flat, g_x_ref = load_grads_case(name)
    m = BoostedFlow(_args(cfg, dev, C=1))
    m.load_spec(0, spec)
    m.eval()
    g_x, ll = m.component_score(torch.from_numpy(x).to(dev), 0)
    ref = -x.shape[0] * np.asarray(g_x_ref, dtype=np.float64)
    err = float(np.abs(g_x.cpu().numpy() - ref).max())
    print(f"{name}: |component_score + N g_x| = {err:.2e} of {np.abs(ref).max():.2e}")
    assert err <= G_RTOL * float(np.abs(ref).max())
    assert abs(float(-ll.double().mean()) - nll) <= 1e-5 * abs(nll)
    assert rel_err(ll.cpu().numpy(), score_oracle.component_ll64(spec, x)[2]) < 1e-5


# ---- 4. repeats and modes ---------------------------------------------------------------------------------------------------
def test_score_repeats_bit_for_bit_in_either_mode(golden_case):
    import torch
    dev = torch.device("cuda:0")
    g = golden_case("g6_glow_d43_h64_c3_rho")
    m = _model_from_case(g, dev)
    x = torch.from_numpy(g.x).to(dev)
    a = m.score(x, n_used=g.n_used, return_log_prob=True, return_responsibilities=True)
    b = m.score(x, n_used=g.n_used, return_log_prob=True, return_responsibilities=True)
    m.train()
    c = m.score(x, n_used=g.n_used, return_log_prob=True, return_responsibilities=True)
    m.eval()
    for u, v, w in zip(a, b, c):
        assert torch.equal(u, v), "score does not repeat"
        assert torch.equal(u, w), "score differs between train() and eval()"


def test_score_touches_no_running_statistic_and_records_nothing(golden_case):
    import torch
    dev = torch.device("cuda:0")
    g = golden_case("g6_realnvp_d21_h64_n33")
    m = _model_from_case(g, dev)
    x = torch.from_numpy(g.x).to(dev)
    ref = m.score(x, n_used=g.n_used, return_log_prob=True, return_responsibilities=True)
    m.train()
    buffers = {k: v.clone() for k, v in m.named_buffers()}
    params = {k: v.clone() for k, v in m.named_parameters()}
    xr = x.clone().requires_grad_(True)
    out = m.score(xr, n_used=g.n_used, return_log_prob=True, return_responsibilities=True) + m.component_score(xr, 0) + (m.responsibilities(xr, g.n_used),)
    for t in out:
        assert not t.requires_grad and t.grad_fn is None
    for u, v in zip(ref, out[:3]):
        assert torch.equal(u, v), "train() mode must run on the running statistics too"
    for k, v in m.named_buffers():
        assert torch.equal(v, buffers[k]), f"buffer {k} moved"
    for k, v in m.named_parameters():
        assert torch.equal(v, params[k]) and v.grad is None
    assert xr.grad is None


def test_score_between_a_recorded_train_mode_forward_and_its_backward(golden_case):
    """RealNVP with BatchNorm in train(): the recorded forward leaves the batch's statistics in the trainer's live blob, where the
    backward sweep reads them; the forwards of a score call re-derive those entries from the running statistics.  So a backward
    that comes after the score call raises (as after any other forward of that component), and one that comes before is what it
    is without any score call, bit for bit."""
    import torch
    dev = torch.device("cuda:0")
    g = golden_case("g6_realnvp_d21_h64_n33")
    x = torch.from_numpy(g.x).to(dev)
    g_z, g_l = _upstream(g.x.shape, dev)

    def recorded(score_before_backward, score_after_backward):
        m = _model_from_case(g, dev)
        m.train()
        xr = x.clone().requires_grad_(True)
        z, ldj = m.component_forward(xr, 0)
        tr = m.native_trainer(0)
        assert tr.batch_stats
        loss = (z * g_z).sum() + (ldj * g_l).sum()
        if score_before_backward:
            m.score(x, n_used=g.n_used)
            m.component_score(x, 0)
            assert tr.batch_stats                       # the mode is put back ...
            with pytest.raises(RuntimeError, match="batch statistics of this call were overwritten"):
                loss.backward()                         # ... but the statistics are gone: refused, not wrong
            return None
        loss.backward()
        if score_after_backward:
            m.score(x, n_used=g.n_used)
        return [xr.grad.clone()] + [p.grad.clone() for p in m.flows[0].parameters() if p.grad is not None]

    recorded(True, False)
    plain, then_score = recorded(False, False), recorded(False, True)
    assert len(plain) == len(then_score) > 1
    # (the weight gradients are added with float atomics in no fixed order: x.grad is compared bit for bit, the rest closely)
    assert torch.equal(plain[0], then_score[0])
    for a, b in zip(plain[1:], then_score[1:]):
        assert float((a - b).abs().max()) <= 2e-4 * max(float(a.abs().max()), 1e-3)
    # a component that was NOT part of the score call keeps its pending backward
    m = _model_from_case(g, dev)
    m.train()
    xr = x.clone().requires_grad_(True)
    z, ldj = m.component_forward(xr, 2)
    m.score(x, n_used=2)
    m.component_score(x, 0)
    ((z * g_z).sum() + (ldj * g_l).sum()).backward()
    ref = _model_from_case(g, dev)
    ref.train()
    xq = x.clone().requires_grad_(True)
    z, ldj = ref.component_forward(xq, 2)
    ((z * g_z).sum() + (ldj * g_l).sum()).backward()
    assert torch.equal(xr.grad, xq.grad)


def test_score_refuses_what_it_cannot_serve(golden_case):
    import torch
    from gbnf_amd import BoostedFlow, native
    dev = torch.device("cuda:0")
    g = golden_case("g6_glow_d43_h64_c3_rho")
    m = _model_from_case(g, dev)
    for call in (lambda t: m.score(t), lambda t: m.component_score(t, 0), lambda t: m.responsibilities(t)):
        with pytest.raises(native.GbnfError):
            call(torch.from_numpy(g.x))          # a CPU tensor: as _check_ready
    with pytest.raises(ValueError):
        m.component_score(torch.from_numpy(g.x).to(dev), 3)
    with pytest.raises(ValueError):
        m.score(torch.from_numpy(g.x).to(dev), n_used=4)
    fresh = BoostedFlow(_args(g.cfg, dev)).to(dev)         # ActNorm not initialised
    fresh.eval()
    for call in (lambda t: fresh.score(t), lambda t: fresh.component_score(t, 0), lambda t: fresh.responsibilities(t)):
        with pytest.raises(ValueError, match="ActNorm"):
            call(torch.from_numpy(g.x).to(dev))


# ---- 5. responsibilities ----------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("name", ["g6_glow_d43_h64_c3_rho", "g4_realnvp_d21_h105_c8"])
def test_responsibilities(name, golden_case):
    import torch
    dev = torch.device("cuda:0")
    g = golden_case(name)
    m = _model_from_case(g, dev)
    x = torch.from_numpy(g.x).to(dev)
    r = m.responsibilities(x, n_used=g.n_used)
    assert tuple(r.shape) == (x.shape[0], g.n_used)
    assert float((r.double().sum(dim=1) - 1.0).abs().max()) <= 1e-6
    assert torch.equal(r, m.score(x, n_used=g.n_used, return_responsibilities=True)[1])


# ---- 6. the autograd short-cut ----------------------------------------------------------------------------------------------
@pytest.mark.parametrize("name", ["g6_glow_d43_h64_c3_rho", "g6_realnvp_d21_h64_n33"])
def test_frozen_parameters_take_the_data_gradient_only_backward(name, golden_case, monkeypatch):
    import torch
    from gbnf_amd import native
    dev = torch.device("cuda:0")
    g = golden_case(name)
    m = _model_from_case(g, dev)
    g_z, g_l = _upstream(g.x.shape, dev)
    calls = {"x": 0, "full": 0}
    bx, bf = native.NativeTrainer.backward_x, native.NativeTrainer.backward
    monkeypatch.setattr(native.NativeTrainer, "backward_x", lambda self, *a, **k: (calls.__setitem__("x", calls["x"] + 1), bx(self, *a, **k))[1])
    monkeypatch.setattr(native.NativeTrainer, "backward", lambda self, *a, **k: (calls.__setitem__("full", calls["full"] + 1), bf(self, *a, **k))[1])

    def x_grad():
        x = torch.from_numpy(g.x).to(dev).requires_grad_(True)
        z, ldj = m.component_forward(x, 0, differentiable=True)
        ((z * g_z).sum() + (ldj * g_l).sum()).backward()
        return x.grad

    for p in m.parameters():
        p.requires_grad_(False)
    frozen = x_grad()
    assert calls == {"x": 1, "full": 0}
    assert all(p.grad is None for p in m.parameters())
    for p in m.parameters():
        p.requires_grad_(True)
    live = x_grad()
    assert calls == {"x": 1, "full": 1}
    assert any(p.grad is not None for p in m.flows[0].parameters())
    assert torch.equal(frozen, live)


# ---- 7. refusals on the device path -----------------------------------------------------------------------------------------
def test_device_path_refusals(golden_case):
    import torch
    from gbnf_amd import native
    dev = torch.device("cuda:0")
    g = golden_case("g6_realnvp_d21_h64_n33")
    m = _model_from_case(g, dev)
    x = torch.from_numpy(g.x).to(dev)
    m.train()
    m.component_forward(x.clone().requires_grad_(True), 0)           # train(): the trainer goes to batch statistics
    tr = m.native_trainer(0)
    assert tr.batch_stats
    with pytest.raises(native.GbnfError, match=r"error -2.*batch-statistics"):
        tr.backward_x(x)
    with pytest.raises(native.GbnfError, match=r"error -2.*batch-statistics"):
        native.mixture_score([tr], torch.zeros(1, device=dev), x)
    tr.set_batch_stats(False)
    out = torch.full_like(x, 7.0)
    small = torch.empty(64, dtype=torch.float32, device=dev)
    with pytest.raises(native.GbnfError, match=r"error -1.*workspace too small"):
        tr.backward_x(x, g_x=out, workspace=small)
    with pytest.raises(native.GbnfError, match=r"error -1.*workspace too small"):
        native.mixture_score([tr], torch.zeros(1, device=dev), x, workspace=small)
    torch.cuda.synchronize()
    assert bool((out == 7.0).all())                                 # refused before any launch
    # trainers of different d: refused by the library itself
    other = native.NativeTrainer(_dev_spec(golden_case("g6_glow_d43_h64_n77").specs[0], dev))
    arr = (ctypes.c_void_p * 2)(tr.handle, other.handle)
    nb = ctypes.c_int64(-1)
    assert native.lib().gbnf_mixture_score_workspace_bytes(arr, 2, 8, ctypes.byref(nb)) == -1 and nb.value == -1
    assert b"d = 43" in native.lib().gbnf_last_error()
    # n == 0 is served
    e = x[:0].contiguous()
    assert tuple(tr.backward_x(e).shape) == (0, x.shape[1])
    assert tuple(native.mixture_score([tr], torch.zeros(1, device=dev), e)[0].shape) == (0, x.shape[1])
