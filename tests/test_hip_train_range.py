"""GPU: the range-safe trainer (``native.NativeTrainer(spec, math="bf16x6")``, gbnf_trainer_create_mode(GBNF_MATH_BF16X6)).

Every sweep of such a trainer -- traced and untraced, on running and on batch statistics -- the live weight re-pack and the weight
gradients run on three bf16 pieces per operand with the range of f32: operands beyond the fp16 range (+-65504), which the f16x3
trainer clamps (finite steps, wrong gradients, gbnf_training_saturation_count), give the float64 oracle's numbers.  Tolerances are
those of tests/test_hip_train.py: forward 1e-5, gradients G_RTOL of each tensor's largest entry, against
oracle.component_forward(backend="numpy64") and oracle.component_grads."""
import argparse
import ctypes as C
import warnings

import numpy as np
import pytest

from conftest import GRADS_CASES, load_grads_case, load_train_bn_case, rel_err

pytestmark = pytest.mark.gpu
G_RTOL = 2e-4
SAFE_MODES = ["bf16x6", "repair"]          # the trainer modes that give f32-range results: always bf16x6, or f16x3 with the same-call re-run

TRAIN_CASES = ["g3_glow_d43_h215_c8", "g5_glow_d43_h64_c2_additive", "g5_glow_d43_h64_c2_reverse_relu",
               "g5_glow_d43_h64_c2_depth2", "g5_glow_d43_h64_c2_depth0", "g5_glow_d6_h30_c2", "g5_glow_d63_h128_c2",
               "g4_realnvp_d21_h105_c8", "g4_realnvp_d21_h105_c2_mixed", "g4_realnvp_d21_h105_c2_relu_nobn",
               "g5_realnvp_d6_h30_c3", "g6_glow_d43_h64_n77", "g6_glow_d43_h64_n1", "g6_realnvp_d21_h64_n33",
               "g1_toy_realnvp_c2"]


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


def _grad_misses(dev_grads, ref_grads, floor=1e-3):
    """[(k, error, scale)] of the gradient tensors beyond G_RTOL of their largest entry (a copy of test_hip_train._check_grads)."""
    assert len(dev_grads) == len(ref_grads)
    out = []
    for k, (a, b) in enumerate(zip(dev_grads, ref_grads)):
        if b is None:
            assert a is None
            continue
        a = a.detach().cpu().numpy().reshape(b.shape)
        scale = max(float(np.abs(b).max()), floor)
        err = float(np.abs(a - b).max())
        if not err <= G_RTOL * scale:
            out.append((k, err, scale))
    return out


def _check_grads(dev_grads, ref_grads, what, floor=1e-3):
    miss = _grad_misses(dev_grads, ref_grads, floor)
    assert not miss, f"{what}: gradient tensors (index, error, scale) beyond {G_RTOL}: {miss}"


def _last_path(tr):
    from gbnf_amd import native
    L = native.lib()
    L.gbnf_debug_trainer_last_path.argtypes = [C.c_void_p, C.POINTER(C.c_int32), C.POINTER(C.c_int32)]
    a, b = C.c_int32(-1), C.c_int32(-1)
    assert L.gbnf_debug_trainer_last_path(tr.handle, C.byref(a), C.byref(b)) == 0
    return a.value, b.value


def _forward_ok(z, ldj, z64, ldj64):
    return (rel_err(ldj.cpu().numpy(), ldj64) < 1e-5 and
            float(np.abs(z.cpu().numpy() - z64).max()) <= 1e-5 * max(1.0, float(np.abs(z64).max())))


def _parity(spec, xs, what, math="bf16x6", seed=7):
    """Traced and untraced, 16-sample waves and forced 32-sample waves, against the float64 oracle; the chained kernels ran."""
    import torch
    from gbnf_amd import native
    from oracle import gbnf_oracle as oracle
    dev = torch.device("cuda:0")
    rng = np.random.RandomState(seed)
    tr = native.NativeTrainer(_dev_spec(spec, dev), math=math)
    assert tr.math == math
    x = torch.from_numpy(xs).to(dev)
    g_z = rng.standard_normal(xs.shape).astype(np.float32)
    g_l = rng.standard_normal(xs.shape[0]).astype(np.float32)
    gz, gl = torch.from_numpy(g_z).to(dev), torch.from_numpy(g_l).to(dev)
    z64, ldj64 = oracle.component_forward(spec, xs, backend="numpy64")
    gx64, grads64 = oracle.component_grads(spec, xs, g_z, g_l)
    native.saturation_count(reset=True)
    for nt in (0, 2):
        native.tuning_set("force_nt", nt)
        try:
            z, ldj = tr.forward(x)
            assert _last_path(tr)[0] == 1, "the untraced forward of a range-safe trainer runs the chained sweep"
            gx_u, grads_u = tr.backward(x, gz, gl, want_gx=True)
            assert _last_path(tr) == (1, 1), "the untraced backward of a range-safe trainer runs the traced pair"
            z2, ldj2, trace = tr.forward(x, want_trace=True)
            gx_t, grads_t = tr.backward(x, gz, gl, want_gx=True, trace=trace)
            assert _last_path(tr) == (1, 1)
            torch.cuda.synchronize()
        finally:
            native.tuning_set("force_nt", 0)
        assert _forward_ok(z, ldj, z64, ldj64), f"{what} nt={nt} untraced forward"
        assert _forward_ok(z2, ldj2, z64, ldj64), f"{what} nt={nt} traced forward"
        _check_grads(grads_u, grads64, f"{what} nt={nt} untraced")
        _check_grads(grads_t, grads64, f"{what} nt={nt} traced")
        for gx in (gx_u, gx_t):
            assert np.abs(gx.cpu().numpy() - gx64).max() <= G_RTOL * float(np.abs(gx64).max()), f"{what} nt={nt} g_x"
    assert native.training_saturation_count() == 0


@pytest.mark.parametrize("name", TRAIN_CASES)
def test_safe_trainer_matches_oracle_in_range(name, golden_case):
    g = golden_case(name)
    for c in sorted({0, len(g.specs) - 1}):
        _parity(g.specs[c], g.x, f"{name}[{c}]")


@pytest.mark.parametrize("name", GRADS_CASES)
def test_safe_trainer_matches_oracle_on_the_reference_gradient_cases(name):
    cfg, spec, x, nll, flat, g_x = load_grads_case(name)
    _parity(spec, x, name)


def _range_case(spec, xs, what):
    """Shared body of the out-of-range tests: upstream gradients 1 / n; the f16x3 trainer saturates, is counted and misses the
    tolerance somewhere (the inputs really leave the fp16 range); every range-safe mode meets it everywhere."""
    import torch
    from gbnf_amd import native
    from oracle import gbnf_oracle as oracle
    dev = torch.device("cuda:0")
    n = xs.shape[0]
    x = torch.from_numpy(xs).to(dev)
    g_z = np.full(xs.shape, 1.0 / n, np.float32)
    g_l = np.full(n, 1.0 / n, np.float32)
    gz, gl = torch.from_numpy(g_z).to(dev), torch.from_numpy(g_l).to(dev)
    z64, ldj64 = oracle.component_forward(spec, xs, backend="numpy64")
    gx64, grads64 = oracle.component_grads(spec, xs, g_z, g_l)
    assert np.isfinite(z64).all() and np.isfinite(ldj64).all() and np.isfinite(gx64).all()
    print(f"{what}: oracle max |z| {np.abs(z64).max():.3g}, max gradient {max(float(np.abs(g).max()) for g in grads64 if g is not None):.3g}")

    def run(math):
        tr = native.NativeTrainer(_dev_spec(spec, dev), math=math)
        z, ldj, trace = tr.forward(x, want_trace=True)
        gx, grads = tr.backward(x, gz, gl, want_gx=True, trace=trace)
        torch.cuda.synchronize()
        ok_f = _forward_ok(z, ldj, z64, ldj64)
        ok_x = bool(np.abs(gx.cpu().numpy() - gx64).max() <= G_RTOL * float(np.abs(gx64).max()))
        miss = _grad_misses(grads, grads64)
        print(f"{what} {math}: forward ok {ok_f}, g_x ok {ok_x}, gradient misses {miss}")
        return tr, ok_f, ok_x, miss

    native.saturation_count(reset=True)
    _, ok_f, ok_x, miss = run("f16x3")
    assert native.training_saturation_count() > 0, "the inputs do not leave the fp16 range"
    assert not (ok_f and ok_x and not miss), "the saturating trainer meets every tolerance: the case shows nothing"
    native.saturation_count(reset=True)
    for math in SAFE_MODES:
        tr, ok_f, ok_x, miss = run(math)
        assert ok_f, f"{what} {math}: z / ldj"
        assert ok_x, f"{what} {math}: g_x"
        assert not miss, f"{what} {math}: gradient tensors (index, error, scale) beyond {G_RTOL}: {miss}"
        assert _last_path(tr) == (1, 1)
        assert native.training_saturation_count() == 0, f"{math}: a range-safe trainer moved the training counter"
        if math == "repair":
            assert tr.repair_count() == 2 and native.saturation_count() > 0      # the forward and the backward call were re-run
        else:
            assert tr.repair_count() == 0 and native.saturation_count() == 0
        # ... and the same without a trace
        z, ldj = tr.forward(x)
        gx, grads = tr.backward(x, gz, gl, want_gx=True)
        assert _forward_ok(z, ldj, z64, ldj64)
        _check_grads(grads, grads64, f"{what} {math} untraced")
        assert np.abs(gx.cpu().numpy() - gx64).max() <= G_RTOL * float(np.abs(gx64).max())
        if math == "bf16x6":
            assert _last_path(tr) == (1, 1)
        assert native.training_saturation_count() == 0
        native.saturation_count(reset=True)
    native.saturation_count(reset=True)


@pytest.mark.parametrize("kind,d,h", [("glow", 43, 215), ("realnvp", 21, 105)])
def test_out_of_range_inputs(kind, d, h):
    from gbnf_amd import synth
    spec = synth.synth_glow_spec(d, h, 5, seed=3) if kind == "glow" else synth.synth_realnvp_spec(d, h, 5, seed=3)
    x = synth.synth_batch(200, d, seed=4)
    x[7, :] = 3.0e5
    x[150, 3] = -1.0e6
    _range_case(spec, x, f"{kind} out-of-range rows")


def test_blown_relu_net():
    """A ReLU net that has grown during boosting: hidden activations of ~1e6 inside step 0's net, brought back by a small output layer."""
    from gbnf_amd import synth
    spec = synth.synth_glow_spec(8, 32, 3, seed=3, act="relu")
    layers = spec["steps"][0]["net"]["layers"]
    for l in (0, 1):
        layers[l] = (np.ascontiguousarray(layers[l][0] * np.float32(2000.0)), layers[l][1])
    layers[-1] = (np.ascontiguousarray(layers[-1][0] / np.float32(4.0e6)), layers[-1][1])
    _range_case(spec, synth.synth_batch(256, 8, seed=4), "blown ReLU net")


def _args(kind, d, h, K, C_, dev, **kw):
    return argparse.Namespace(
        num_flows=K, z_size=d, density_evaluation=True, device=dev, cuda=True, component_type=kind, num_components=C_,
        rho_init="decreasing", learn_top=False, y_classes=0, y_condition=False, sample_size=4, input_size=[d], h_size=h,
        num_blocks=1, actnorm_scale=1.0, flow_permutation=kw.get("permutation", "shuffle"),
        flow_coupling=kw.get("coupling", "affine"), LU_decomposed=False, num_dequant_blocks=0,
        coupling_network=kw.get("act", kw.get("coupling_network", "tanh")), coupling_network_depth=kw.get("depth", 1),
        batch_norm=kw.get("batch_norm", True), train_math=kw.get("train_math"))


@pytest.mark.parametrize("math", SAFE_MODES)
def test_module_trains_a_blown_net_in_silence(math):
    """The blown-net epoch of test_leaving_training_mode_reports_saturated_training_kernels with args.train_math: leaving training
    mode is silent (the training counter did not move) and every p.grad is the float64 oracle's.
    The net is blown as in test_blown_relu_net -- layers 0 and 1 x 2000 AND the output layer / 4e6: with the first two alone (what the
    f16x3 test does, whose clamped step is finite whatever the net returns) the raw scale reaches -1e6, log(sigmoid(raw + 2)) is -inf in
    the reference's own formula (models/glow.py:333-338) in float32 and in float64 alike, and there is no finite gradient to compare with."""
    import torch
    from gbnf_amd import BoostedFlow, native
    from gbnf_amd import spec as gspec
    from oracle import gbnf_oracle as oracle
    dev = torch.device("cuda:0")

    def run(mode):
        torch.manual_seed(3)
        m = BoostedFlow(_args("glow", 8, 32, 3, 1, dev, act="relu", train_math=mode)).to(dev)
        assert m.train_math == mode
        x = torch.randn(256, 8, device=dev)

        def epoch():
            m.train()
            z, _, _, ldj, _ = m(x=x, components=0)
            loss = torch.mean(-(torch.sum(-0.5 * np.log(2 * np.pi) - 0.5 * z.pow(2), dim=-1) + ldj))
            loss.backward()
            return float(loss.detach())

        native.saturation_count(reset=True)
        assert np.isfinite(epoch())
        net = m.flows[0].flow.layers[0].block.network
        linears = [mod for mod in net if isinstance(mod, torch.nn.Linear)]
        assert len(linears) == 3
        with torch.no_grad():
            linears[0].weight.mul_(2000.0)
            linears[1].weight.mul_(2000.0)
            linears[2].weight.div_(4.0e6)
        m.zero_grad(set_to_none=True)
        spec = gspec.spec_from_component(m.flows[0])
        loss = epoch()
        assert m.native_trainer(0).math == mode
        return m, x, spec, loss

    # the saturating module on the same epoch: counted (the net really leaves the fp16 range), reported when training mode is left
    m, x, spec, _ = run("f16x3")
    assert native.training_saturation_count() > 0
    with pytest.warns(RuntimeWarning, match="65504"):
        m.eval()
    native.saturation_count(reset=True)

    m, x, spec, loss = run(math)
    assert np.isfinite(loss)
    with warnings.catch_warnings():
        warnings.simplefilter("error")
        m.eval()
    assert native.training_saturation_count() == 0
    xs = x.cpu().numpy()
    n = xs.shape[0]
    z64, ldj64 = oracle.component_forward(spec, xs, backend="numpy64")
    assert np.isfinite(z64).all() and np.isfinite(ldj64).all()
    gx64, grads64 = oracle.component_grads(spec, xs, (z64 / n).astype(np.float32), np.full(n, -1.0 / n, np.float32))
    print(f"module {math}: oracle max gradient {max(float(np.abs(g).max()) for g in grads64 if g is not None):.3g}")
    params = m.native_trainer(0).params
    _check_grads([None if t is None else t.grad for t in params], grads64, f"module {math}")
    native.saturation_count(reset=True)


@pytest.mark.parametrize("math", SAFE_MODES)
def test_batch_statistics_with_out_of_range_rows(math):
    """RealNVP in the reference's train() mode (BatchNorm on batch statistics, one launch per step range) on the geometry of
    g10_realnvp_grads_train_bn with two rows beyond the fp16 range; tolerances of test_train_mode_batch_norm_matches_reference."""
    import torch
    from gbnf_amd import native
    from oracle import gbnf_oracle as oracle
    dev = torch.device("cuda:0")
    cfg, spec, x, data = load_train_bn_case()
    x = x.copy()
    n, d = x.shape
    x[7, :] = 3.0e5
    x[n - 2, 3] = -1.0e6
    dv = _dev_spec(spec, dev)
    for st in dv["steps"]:
        if st["bn"] is not None:
            st["bn"]["batch_mean"] = torch.zeros(d, device=dev)
            st["bn"]["batch_var"] = torch.zeros(d, device=dev)
    tr = native.NativeTrainer(dv, math=math)
    assert tr.has_batch_stats
    tr.set_batch_stats(True)
    xd = torch.from_numpy(x).to(dev)
    native.saturation_count(reset=True)
    z, ldj, trace = tr.forward(xd, want_trace=True)
    K = len(spec["steps"])
    if math == "bf16x6":
        assert _last_path(tr)[0] == max(K - 1, 1)
    z64, ldj64, _ = oracle.component_forward_train(spec, x)
    print(f"batch statistics {math}: z err {np.abs(z.cpu().numpy() - z64).max():.3g} of {np.abs(z64).max():.3g}, "
          f"ldj rel err {rel_err(ldj.cpu().numpy(), ldj64):.3g}")
    assert np.abs(z.cpu().numpy() - z64).max() <= 2e-5 * float(np.abs(z64).max())
    assert rel_err(ldj.cpu().numpy(), ldj64) < 1e-5
    g_z = (z64 / n).astype(np.float32)
    g_l = np.full(n, -1.0 / n, np.float32)
    gx64, grads64 = oracle.component_grads(spec, x, g_z, g_l, train=True)
    gx, grads = tr.backward(xd, torch.from_numpy(g_z).to(dev), torch.from_numpy(g_l).to(dev), want_gx=True, trace=trace)
    if math == "bf16x6":
        assert _last_path(tr)[1] == max(K - 1, 1)
    mine = np.concatenate([np.zeros(d, np.float32) if g is None else g.cpu().numpy().reshape(-1) for g in grads])
    ref = np.concatenate([np.zeros(d) if g is None else np.asarray(g).reshape(-1) for g in grads64])
    print(f"batch statistics {math}: gradient err {np.abs(mine - ref).max():.3g} of {np.abs(ref).max():.3g}, "
          f"g_x err {np.abs(gx.cpu().numpy() - gx64).max():.3g} of {np.abs(gx64).max():.3g}")
    assert np.abs(mine - ref).max() <= G_RTOL * float(np.abs(ref).max())
    assert np.abs(gx.cpu().numpy() - gx64).max() <= G_RTOL * float(np.abs(gx64).max())
    assert native.training_saturation_count() == 0
    native.saturation_count(reset=True)


def test_unsupported_modes_and_geometries_are_refused_with_a_reason():
    import torch
    from gbnf_amd import native, synth
    dev = torch.device("cuda:0")
    long_flow = _dev_spec(synth.synth_glow_spec(8, 40, 26, seed=51, gain=0.5), dev)
    for math in ("bf16x6", "repair"):
        with pytest.raises(native.GbnfError, match="24"):
            native.NativeTrainer(long_flow, math=math)
    with pytest.raises(native.GbnfError):                    # a width beyond the compiled bf16x6 training sweeps: no silent downgrade
        native.NativeTrainer(_dev_spec(synth.synth_glow_spec(43, 300, 2, seed=5), dev), math="bf16x6")
    with pytest.raises(native.GbnfError):
        native.NativeTrainer(_dev_spec(synth.synth_glow_spec(43, 300, 2, seed=5), dev), math="repair")
    for bad in ("f32", "default", "", None):
        with pytest.raises(native.GbnfError):
            native.NativeTrainer(long_flow, math=bad)
    # GBNF_MATH_F32 is refused by the library itself
    L = native.lib()
    h = C.c_void_p()
    assert L.gbnf_trainer_create_mode(None, native.MATH["f32"], C.byref(h)) != 0
    assert "f32" in L.gbnf_last_error().decode()
    # the saturating trainer still builds for the long flow, and never reports a re-run
    tr = native.NativeTrainer(long_flow)
    assert tr.math == "f16x3" and tr.repair_count() == 0


def test_repair_bookkeeping():
    """The repairing trainer: on in-range data it IS the f16x3 trainer (z, ldj, g_x bit for bit; weight gradients within tolerance of
    it: atomics reorder the sums) and nothing is re-run; on out-of-range data the calls are re-run, counted as repairs and as range
    events of the evaluation kind, not as wrong training steps; the scale of the upstream gradients triggers nothing."""
    import torch
    from gbnf_amd import native, synth
    dev = torch.device("cuda:0")
    native.saturation_count(reset=True)
    for kind, d, h in (("glow", 43, 215), ("realnvp", 21, 105)):
        spec = synth.synth_glow_spec(d, h, 5, seed=3) if kind == "glow" else synth.synth_realnvp_spec(d, h, 5, seed=3)
        xs = synth.synth_batch(200, d, seed=4)
        x = torch.from_numpy(xs).to(dev)
        rng = np.random.RandomState(5)
        gz = torch.from_numpy(rng.standard_normal(xs.shape).astype(np.float32)).to(dev)
        gl = torch.from_numpy(rng.standard_normal(200).astype(np.float32)).to(dev)
        fast = native.NativeTrainer(_dev_spec(spec, dev), math="f16x3")
        rep = native.NativeTrainer(_dev_spec(spec, dev), math="repair")
        for traced in (True, False):
            outs = []
            for tr in (fast, rep):
                if traced:
                    z, ldj, trace = tr.forward(x, want_trace=True)
                else:
                    (z, ldj), trace = tr.forward(x), None
                gx, grads = tr.backward(x, gz, gl, want_gx=True, trace=trace)
                outs.append((z, ldj, gx, grads))
            (z0, l0, g0, w0), (z1, l1, g1, w1) = outs
            assert torch.equal(z0, z1) and torch.equal(l0, l1) and torch.equal(g0, g1), f"{kind} traced={traced}"
            _check_grads(w1, [None if t is None else t.cpu().numpy() for t in w0], f"{kind} repair vs f16x3")
        assert rep.repair_count() == 0 and native.saturation_count() == 0
        # out of range: re-run, counted where it belongs
        xb = xs.copy()
        xb[7, :] = 3.0e5
        xb[150, 3] = -1.0e6
        xbd = torch.from_numpy(xb).to(dev)
        z, ldj, trace = rep.forward(xbd, want_trace=True)
        assert rep.repair_count() == 1
        rep.backward(xbd, gz, gl, want_gx=True, trace=trace)
        assert rep.repair_count() == 2
        assert native.training_saturation_count() == 0 and native.saturation_count() > 0
        assert rep.repair_count(reset=True) == 2 and rep.repair_count() == 0
        native.saturation_count(reset=True)
        # a healthy call afterwards is not re-run (the decision belongs to the call)
        z, ldj, trace = rep.forward(x, want_trace=True)
        rep.backward(x, gz, gl, trace=trace)
        assert rep.repair_count() == 0
    # the scale of the loss triggers nothing (test_trainer_counts_saturated_operands)
    spec = synth.synth_glow_spec(8, 16, 2, seed=3, act="relu")
    tr = native.NativeTrainer(_dev_spec(spec, dev), math="repair")
    xd = torch.from_numpy(synth.synth_batch(64, 8, seed=4)).to(dev)
    z, ldj, trace = tr.forward(xd, want_trace=True)
    tr.backward(xd, torch.ones_like(z) * 1e-9, torch.ones_like(ldj) * 1e9, want_gx=True, trace=trace)
    assert tr.repair_count() == 0 and native.saturation_count() == 0


def test_device_packer_reproduces_the_bf16x6_host_packer():
    """The bf16x6 twin of the live re-pack: the blob of a range-safe trainer, re-packed on the device from the live weights, is the
    blob the host packs for a bf16x6 evaluation handle of the same geometry -- weights (three bf16 pieces per tile, both rounded to
    nearest even) and biases bit for bit, the table constants (expf / sqrtf on the device) to a few ulp."""
    import torch
    from gbnf_amd import native, synth
    dev = torch.device("cuda:0")
    L = native.lib()

    def words(name, handle):
        fn = getattr(L, name)
        fn.argtypes = [C.c_void_p, C.c_void_p, C.POINTER(C.c_int64)]
        fn.restype = C.c_int
        n = C.c_int64()
        native._check(fn(handle, None, C.byref(n)))
        buf = np.zeros(n.value, np.uint32)
        native._check(fn(handle, buf.ctypes.data_as(C.c_void_p), C.byref(n)))
        return buf

    # (a geometry whose evaluation handle and trainer run the same compiled variant, so that the two blobs have one layout)
    for kind, d, h in (("glow", 43, 215),):
        spec = synth.synth_glow_spec(d, h, 3, seed=21) if kind == "glow" else synth.synth_realnvp_spec(d, h, 3, seed=21)
        assert set(native.activation_pattern(spec)) <= {"tanh", ("tanh", "tanh")}
        # a weight beyond the fp16 range is legal here (and not counted)
        first = spec["steps"][0]["net" if kind == "glow" else "t_net"]["layers"][0]
        first[0][0, 0] = np.float32(3.0e5)
        flow = native.NativeFlow(spec, math="bf16x6")
        tr = native.NativeTrainer(_dev_spec(spec, dev), math="bf16x6")
        native.saturation_count(reset=True)
        host = words("gbnf_debug_flow_blob", flow.handle)
        live = words("gbnf_debug_trainer_blob", tr.handle)
        assert native.saturation_count(reset=True) == 0
        assert host.shape == live.shape, kind
        diff = np.nonzero(host != live)[0]
        if diff.size:
            a, b = host[diff].view(np.float32), live[diff].view(np.float32)
            assert np.all(np.abs(a - b) <= 6e-7 * np.maximum(np.abs(a), 1e-30) + 1e-30), (kind, diff[:8], a[:8], b[:8])
            assert diff.size < 0.01 * host.size, kind            # only table constants may differ in the last bit
