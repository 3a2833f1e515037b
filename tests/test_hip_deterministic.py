"""GPU: deterministic training mode of the tabular trainer (gbnf_trainer_set_deterministic, ``NativeTrainer(deterministic=True)``,
``BoostedFlow(args.deterministic)``).

With the mode on every sample chunk of a weight-gradient block stores its partial and a second launch adds the partials in chunk
order, so ``backward``, ``nll_step`` and ``boosted_nll_step`` repeat bit for bit.  Checked here: the ordered gradients are the right
gradients (float64 oracle, the bars of tests/test_hip_train_range.py: G_RTOL of each tensor's largest entry, 1e-5 forward), repeated
calls are ``torch.equal``, two independently built modules stay ``torch.equal`` over five steps, calls that would run the per-step
kernels are refused before anything is launched, and the default mode is what it was (same bars, same workspace sizes).

Shapes: n = 600 gives every one of these nets at least 4 sample chunks (asserted from the library's own workspace sizes: the
deterministic workspace is the default one plus chunks x grad_floats floats), n = 77 is the ragged batch."""
import ctypes as C

import numpy as np
import pytest

from test_hip_train import _args
from test_hip_train_range import G_RTOL, _check_grads, _dev_spec, _forward_ok, _last_path

pytestmark = pytest.mark.gpu
MODES = ["f16x3", "bf16x6", "repair"]
REPEATS = 20


def _dev():
    import torch
    return torch.device("cuda:0")


def _spec(name):
    from gbnf_amd import synth
    if name.startswith("glow_d43_h64_depth"):
        return synth.synth_glow_spec(43, 64, 2, depth=int(name[-1]), seed=11)
    if name == "glow_d43_h272":
        return synth.synth_glow_spec(43, 272, 2, seed=12)
    if name == "glow_d43_h320":
        return synth.synth_glow_spec(43, 320, 2, seed=12)
    if name == "realnvp_d21_h105":
        return synth.synth_realnvp_spec(21, 105, 3, seed=13)
    if name == "realnvp_d6_h30_residual":
        return synth.synth_realnvp_spec(6, 30, 3, coupling_network="residual", seed=14)
    raise KeyError(name)


def _last_error():
    from gbnf_amd import native
    return native.lib().gbnf_last_error().decode(errors="replace")


def _ws_bytes(tr, n):
    from gbnf_amd import native
    nb = C.c_int64()
    assert native.lib().gbnf_trainer_workspace_bytes(tr.handle, n, C.byref(nb)) == 0
    return int(nb.value)


def _chunks(tr, n):
    """Sample chunks of the weight-gradient launch at n rows, from the sizes the library reports: on - off = chunks x grad_floats x 4."""
    assert tr.deterministic
    on = _ws_bytes(tr, n)
    tr.deterministic = False
    off = _ws_bytes(tr, n)
    tr.deterministic = True
    extra = on - off
    assert extra > 0 and extra % (4 * tr.grad_floats) == 0
    return extra // (4 * tr.grad_floats)


_ORACLE = {}


def _case(name, n, big_row=False):
    """(spec, x, g_z, g_ldj, oracle forward, oracle gradients), computed once per (geometry, n)."""
    key = (name, n, big_row)
    if key not in _ORACLE:
        from gbnf_amd import synth
        from oracle import gbnf_oracle as oracle
        spec = _spec(name)
        x = synth.synth_batch(n, spec["d"], seed=4)
        if big_row:
            x[7, :] = 3.0e5          # beyond the fp16 range: the repairing trainer commits its bf16x6 re-run
        rng = np.random.RandomState(7)
        g_z = (rng.standard_normal(x.shape) / n).astype(np.float32)
        g_l = (rng.standard_normal(n) / n).astype(np.float32)
        _ORACLE[key] = (spec, x, g_z, g_l, oracle.component_forward(spec, x, backend="numpy64"), oracle.component_grads(spec, x, g_z, g_l))
    return _ORACLE[key]


def _trainer(spec, math, deterministic, batch_stats=False):
    import torch
    from gbnf_amd import native
    ds = _dev_spec(spec, _dev())
    if batch_stats:
        for st in ds["steps"]:
            if st["bn"] is not None:
                st["bn"]["batch_mean"] = torch.zeros(spec["d"], device=_dev())
                st["bn"]["batch_var"] = torch.ones(spec["d"], device=_dev())
    tr = native.NativeTrainer(ds, math=math, deterministic=deterministic)
    if batch_stats:
        assert tr.has_batch_stats
        tr.set_batch_stats(True)
    return tr


def _gradient_case(name, n, math, deterministic=True, big_row=False, min_chunks=4):
    """Traced forward + backward against the oracle, then REPEATS repeated backward calls: identical grads and g_x."""
    import torch
    spec, xs, g_z, g_l, (z64, ldj64), (gx64, grads64) = _case(name, n, big_row)
    tr = _trainer(spec, math, deterministic)
    assert tr.deterministic == deterministic
    if deterministic:
        # (a repairing trainer reports the larger of its two halves' sizes: its halves are an f16x3 and a bf16x6 trainer of this spec)
        halves = [tr] if math != "repair" else [_trainer(spec, m, True) for m in ("f16x3", "bf16x6")]
        for half in halves:
            chunks = _chunks(half, n)
            print(f"{name} n={n} {math} ({half.math}): {chunks} sample chunks")
            assert chunks >= min_chunks
    x, gz, gl = (torch.from_numpy(a).to(_dev()) for a in (xs, g_z, g_l))
    z, ldj, trace = tr.forward(x, want_trace=True)
    gx, grads = tr.backward(x, gz, gl, want_gx=True, trace=trace)
    torch.cuda.synchronize()
    assert _last_path(tr) == (1, 1)
    if not big_row or math != "f16x3":
        assert _forward_ok(z, ldj, z64, ldj64), f"{name} {math} forward"
        _check_grads(grads, grads64, f"{name} n={n} {math} deterministic={deterministic}")
        assert np.abs(gx.cpu().numpy() - gx64).max() <= G_RTOL * float(np.abs(gx64).max())
    if big_row and math == "repair":
        assert tr.repair_count() == 2          # forward and backward were re-run: the bf16x6 form was the one committed
    if not deterministic:
        return
    first = [g.clone() for g in grads if g is not None] + [gx.clone()]
    for _ in range(REPEATS - 1):
        gx2, grads2 = tr.backward(x, gz, gl, want_gx=True, trace=trace)
        again = [g for g in grads2 if g is not None] + [gx2]
        assert all(torch.equal(a, b) for a, b in zip(first, again)), f"{name} {math}: a repeated traced backward differs"
    if math == "repair":           # its f16x3 half would serve an untraced call on the per-step kernels: refused, not served unordered
        from gbnf_amd import native
        with pytest.raises(native.GbnfError, match="deterministic"):
            tr.backward(x, gz, gl, want_gx=True)
    if math == "bf16x6":           # the untraced call of a range-safe trainer runs the traced pair on its own buffer
        ux, ugrads = tr.backward(x, gz, gl, want_gx=True)
        ufirst = [g.clone() for g in ugrads if g is not None] + [ux.clone()]
        _check_grads(ugrads, grads64, f"{name} n={n} {math} untraced")
        for _ in range(REPEATS - 1):
            ux2, ugrads2 = tr.backward(x, gz, gl, want_gx=True)
            assert all(torch.equal(a, b) for a, b in zip(ufirst, [g for g in ugrads2 if g is not None] + [ux2]))


@pytest.mark.parametrize("math", MODES)
@pytest.mark.parametrize("name", ["glow_d43_h64_depth0", "glow_d43_h64_depth1", "glow_d43_h64_depth2", "realnvp_d21_h105",
                                  "realnvp_d6_h30_residual"])
def test_ordered_gradients_are_right_and_repeat(name, math):
    _gradient_case(name, 600, math)


@pytest.mark.parametrize("math", MODES)
def test_ragged_batch(math):
    _gradient_case("glow_d43_h64_depth1", 77, math, min_chunks=1)


@pytest.mark.parametrize("name", ["glow_d43_h272", "glow_d43_h320"])
def test_several_blocks_per_layer(name):
    """f16x3 only: more than one block per layer and a ragged last block (h = 272 = 2 x 128 + 16, h = 320 = 2 x 128 + 64)."""
    _gradient_case(name, 600, "f16x3")


def test_repair_commits_the_bf16x6_form():
    _gradient_case("glow_d43_h64_depth1", 600, "repair", big_row=True)


_BN_ORACLE = []


@pytest.mark.parametrize("math", MODES)
def test_batch_statistics(math):
    """RealNVP d = 21, h = 105, K = 3 with BatchNorm on batch statistics: the ordered gradients against the float64 oracle in train
    mode (oracle.component_grads(train=True), G_RTOL of each tensor's largest entry), and REPEATS identical backward calls."""
    import torch
    from oracle import gbnf_oracle as oracle
    spec, xs, g_z, g_l, _, _ = _case("realnvp_d21_h105", 600)
    if not _BN_ORACLE:
        _BN_ORACLE.append(oracle.component_grads(spec, xs, g_z, g_l, train=True))
    gx64, grads64 = _BN_ORACLE[0]
    x, gz, gl = (torch.from_numpy(a).to(_dev()) for a in (xs, g_z, g_l))
    tr = _trainer(spec, math, True, batch_stats=True)
    z, ldj, trace = tr.forward(x, want_trace=True)
    gx, grads = tr.backward(x, gz, gl, want_gx=True, trace=trace)
    torch.cuda.synchronize()
    assert _last_path(tr)[1] >= 1, "the chained sweeps ran"
    _check_grads(grads, grads64, f"batch statistics {math}")
    assert np.abs(gx.cpu().numpy() - gx64).max() <= G_RTOL * float(np.abs(gx64).max())
    first = [g.clone() for g in grads if g is not None] + [gx.clone()]
    for _ in range(REPEATS - 1):
        gx2, grads2 = tr.backward(x, gz, gl, want_gx=True, trace=trace)
        assert all(torch.equal(a, b) for a, b in zip(first, [g for g in grads2 if g is not None] + [gx2]))


def _module(deterministic, kind="glow"):
    import torch
    from gbnf_amd import BoostedFlow
    dev = _dev()
    torch.manual_seed(0)
    args = _args(kind, 8, 32, 3, 2, dev)
    args.deterministic = deterministic
    m = BoostedFlow(args).to(dev)
    m.train()
    return m


def _state_of(m, c):
    st = m.opt_state(c)
    return [p.detach().clone() for p in m.flows[c].parameters()] + [st.exp_avg.clone(), st.exp_avg_sq.clone()]


def test_module_steps_repeat_bit_for_bit():
    """Two modules from the same seed, 5 plain steps of component 0 and 5 boosted steps (the same uniforms) of component 1, AdamW with
    the clip engaged: parameters, moments and the step's stats are equal after every step."""
    import torch
    dev = _dev()
    n = 600
    gen = torch.Generator(device=dev).manual_seed(3)
    x = torch.randn(n, 8, device=dev, generator=gen) * torch.linspace(0.5, 2.0, 8, device=dev) + 0.3
    us = [torch.rand(n, device=dev, generator=gen) for _ in range(5)]
    a, b = _module(True), _module(True)
    assert a.deterministic and b.deterministic
    clipped = False
    for c in (0, 1):
        a.component = b.component = c
        for k in range(5):
            kw = dict(lr=5e-3, weight_decay=1e-5, max_grad_norm=0.05)
            if c == 1:
                kw["uniforms"] = us[k]
            oa, ob = a.training_step(x, **kw), b.training_step(x, **kw)
            assert a.native_trainer(c).deterministic
            assert set(oa) == set(ob)
            for key in oa:
                assert torch.equal(oa[key], ob[key]), f"component {c} step {k}: {key} {oa[key].item()} vs {ob[key].item()}"
            clipped = clipped or oa["clip_coef"].item() < 1.0
            for ta, tb in zip(_state_of(a, c), _state_of(b, c)):
                assert torch.equal(ta, tb), f"component {c} step {k}"
    assert clipped, "max_grad_norm never engaged: the case does not exercise the clip"


def test_boosted_step_rows_and_state_repeat():
    """gbnf_boosted_nll_step twice from identical copies of the parameters: rows_out, stats, gradients, parameters, moments equal."""
    import torch
    from gbnf_amd import native, synth
    dev = _dev()
    specs = synth.synth_boosted_specs("glow", 2, 8, 32, 3, seed=5)
    n = 600
    x = torch.from_numpy(synth.synth_batch(n, 8, seed=2)).to(dev)
    u = torch.rand(n, device=dev, generator=torch.Generator(device=dev).manual_seed(9))
    rho = torch.tensor([1.0, 0.5], device=dev)
    mix = native.NativeMixture([native.NativeFlow(s) for s in specs])
    outs = []
    for _ in range(2):
        tr = _trainer(specs[1], "f16x3", True)
        state = native.OptState(tr, "adamw")
        stats, flat, rows = tr.boosted_nll_step(mix, 1, rho, x, u, state, want_rows=True, lr=1e-3, weight_decay=1e-5, max_grad_norm=0.05)
        outs.append([stats.clone(), flat.clone(), rows.clone(), state.exp_avg.clone(), state.exp_avg_sq.clone()] +
                    [p.clone() for p in tr.params if p is not None])
    assert all(torch.equal(p, q) for p, q in zip(*outs))
    assert outs[0][0][2].item() < 1.0          # the clip engaged


@pytest.mark.parametrize("what", ["K26", "residual_h300"])
def test_refusals_launch_nothing(what):
    """A flow of 26 steps / a two-block ResidualNet at h = 300 trains on the per-step kernels: refused in deterministic mode, with a
    reason that names it, before anything is launched; served as ever with the mode off."""
    import torch
    from gbnf_amd import native, synth
    dev = _dev()
    if what == "K26":
        spec = synth.synth_glow_spec(8, 32, 26, seed=3, gain=0.3)
    else:
        spec = synth.synth_realnvp_spec(6, 300, 2, coupling_network="residual", depth=2, seed=3)
    x = torch.from_numpy(synth.synth_batch(64, spec["d"], seed=1)).to(dev)
    gz = torch.full_like(x, 1.0 / 64)
    tr = _trainer(spec, "f16x3", True)
    z, ldj, trace = tr.forward(x, want_trace=True)
    nb = _ws_bytes(tr, 64)
    ws = torch.empty(nb // 4 + 1, dtype=torch.float32, device=dev)
    grads = torch.full((tr.grad_floats,), 123.0, device=dev)
    ptr = lambda t: C.c_void_p(t.data_ptr())
    rc = native.lib().gbnf_trainer_backward(tr.handle, ptr(x), 64, ptr(trace), ptr(gz), None, None, ptr(grads), ptr(ws), nb, None)
    torch.cuda.synchronize()
    assert rc == -2, "GBNF_ERR_UNSUPPORTED expected"
    assert "deterministic" in _last_error()
    assert bool((grads == 123.0).all()), "the refused call wrote to grads"
    with pytest.raises(native.GbnfError, match="deterministic"):
        tr.nll_step(x, native.OptState(tr, "adamw"), lr=1e-3)
    tr.deterministic = False
    _, g = tr.backward(x, gz, None, trace=trace)
    assert all(torch.isfinite(t).all() for t in g if t is not None)


def test_untraced_f16x3_call_is_refused():
    import torch
    from gbnf_amd import native
    spec, xs, g_z, g_l, _, _ = _case("glow_d43_h64_depth1", 77)
    tr = _trainer(spec, "f16x3", True)
    x, gz = torch.from_numpy(xs).to(_dev()), torch.from_numpy(g_z).to(_dev())
    with pytest.raises(native.GbnfError, match="deterministic"):
        tr.backward(x, gz, None)


def test_workspace_sized_before_the_switch_is_refused():
    import torch
    from gbnf_amd import native
    spec, xs, g_z, g_l, _, _ = _case("glow_d43_h64_depth1", 600)
    dev = _dev()
    tr = _trainer(spec, "f16x3", False)
    small = _ws_bytes(tr, 600)
    tr.deterministic = True
    assert _ws_bytes(tr, 600) > small
    x, gz = torch.from_numpy(xs).to(dev), torch.from_numpy(g_z).to(dev)
    z, ldj, trace = tr.forward(x, want_trace=True)
    ws = torch.empty(small // 4, dtype=torch.float32, device=dev)
    grads = torch.full((tr.grad_floats,), 123.0, device=dev)
    ptr = lambda t: C.c_void_p(t.data_ptr())
    rc = native.lib().gbnf_trainer_backward(tr.handle, ptr(x), 600, ptr(trace), ptr(gz), None, None, ptr(grads), ptr(ws), small, None)
    torch.cuda.synchronize()
    assert rc == -1 and "workspace too small" in _last_error()
    assert bool((grads == 123.0).all())
    # the step sizes grow with it
    nb_on, nb_off = C.c_int64(), C.c_int64()
    assert native.lib().gbnf_trainer_step_workspace_bytes(tr.handle, 600, C.byref(nb_on)) == 0
    tr.deterministic = False
    assert native.lib().gbnf_trainer_step_workspace_bytes(tr.handle, 600, C.byref(nb_off)) == 0
    assert nb_on.value > nb_off.value


# (geometry, math, n) -> gbnf_trainer_workspace_bytes in default mode.  The numbers are what a library built from the commit before this
# mode existed reports on the device for these trainers (creating a trainer allocates on the device, so they cannot be taken on the
# host), and what its layout gives by hand: (operand rows + 320 slack rows + d state rows) x np x 4.
PARENT_WORKSPACE_BYTES = {
    ("glow_d43_h64_depth1", "f16x3", 600): 2750592,        # (2 x 384 operand rows + 320 slack rows + 43 state rows) x 608 x 4
    ("realnvp_d21_h105", "bf16x6", 77): 1273728,           # (3 x 2 x 496 + 320 + 21) x 96 x 4
}


@pytest.mark.parametrize("key", sorted(PARENT_WORKSPACE_BYTES))
def test_default_mode_is_unchanged(key):
    name, math, n = key
    spec = _spec(name)
    tr = _trainer(spec, math, False)
    assert tr.deterministic is False
    print(f"{key}: gbnf_trainer_workspace_bytes = {_ws_bytes(tr, n)}")
    assert _ws_bytes(tr, n) == PARENT_WORKSPACE_BYTES[key]
    _gradient_case(name, n, math, deterministic=False)


def test_image_module_refuses_at_the_first_training_call(monkeypatch):
    """The image trainer has no ordered path: with the flag set (here through the environment) an image module still builds and
    evaluates, and its first training call raises GbnfError naming determinism; with the flag off the same module trains."""
    import torch
    import image_grad_oracle as igo
    from gbnf_amd import native
    monkeypatch.setenv("GBNF_DETERMINISTIC", "1")
    cfg, data = igo.g21_load(igo.G21[0])
    dev = _dev()
    m = igo.g21_module(cfg, data, dev)
    assert m.deterministic is True
    x, noise = (torch.from_numpy(np.ascontiguousarray(data[k], dtype=np.float32)).to(dev) for k in ("x", "noise"))
    m.eval()
    with torch.no_grad():
        assert torch.isfinite(m.log_prob(x, noise=noise)).all()
    m.train()
    with pytest.raises(native.GbnfError, match="deterministic"):
        m.training_step(x, noise=noise, lr=0.0)
    m.deterministic = False
    out = m.training_step(x, noise=noise, lr=0.0)
    assert torch.isfinite(out["nll"]).item()
