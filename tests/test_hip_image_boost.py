"""GPU: boosting for image components -- gbnf_image_mixture_rho_step / gbnf_image_boosted_nll_step (csrc/gbnf_image_boost.hip),
native.NativeImageFlow.rho_step, native.NativeImageTrainer.boosted_nll_step and BoostedImageFlow.update_rho / training_step(fixed=...)
-- against the float64 oracle (oracle.image_component_forward) and the float64 replay of the update_rho loop
(tests/test_image_boost_host.py).

Tolerances: every log-likelihood within the project's 1e-5 relative bar of float64; the rho gradient within 1e-5 x max(|fixed_ll|,
|new_ll|) of float64 arithmetic on the device's own table (the bound of tests/test_hip_boost.py::test_rho_step) and within twice that of
the oracle's (a difference of two log-likelihoods, each good to 1e-5); parameters of two runs of the same training kernels within
PARAM_TOL (tests/test_hip_image_fused_step.py)."""
import ctypes as C
import functools
import math

import numpy as np
import pytest

import image_step_oracle as iso
import test_image_boost_host as host
from test_hip_image_fused_step import LR, PARAM_TOL, _assert_close, _trainer

pytestmark = pytest.mark.gpu

LL_RTOL = 1e-5
RHO0 = np.array([1.0, 0.5, 0.25], dtype=np.float32)
# name -> (input size, synth_image_glow_spec keywords, the three components' seeds)
RHO_CASES = {
    "2x8x12": ((2, 8, 12), dict(h=16, K=1, L=1), (1, 2, 3)),              # a one-level 4 x 6 map in 8-wide storage
    "1x16x16": ((1, 16, 16), dict(h=32, K=2, L=2), (1, 5, 2)),
    "3x32x32": ((3, 32, 32), dict(h=32, K=1, L=3, depth=0), (1, 2, 3)),   # three levels, a 4 x 4 top map
}
# (300 rows: more than one workgroup of every per-image kernel, a ragged tail of the 256-thread reductions)
RHO_PARAMS = [("2x8x12", 3), ("2x8x12", 300), ("1x16x16", 3), ("3x32x32", 3)]
# float64 gradients of these cases, computed on the CPU when the cases were chosen: the oracle must still say so
GRAD64 = {("2x8x12", 3): 0.921, ("2x8x12", 300): 0.794, ("1x16x16", 3): 9.566, ("3x32x32", 3): -15.41}


def _cuda():
    import torch
    return torch.device("cuda:0")


def _to(a, dev):
    import torch
    return torch.from_numpy(np.ascontiguousarray(a)).to(dev)


@functools.lru_cache(maxsize=None)
def _specs(name):
    from gbnf_amd import synth
    size, kw, seeds = RHO_CASES[name]
    return tuple(synth.synth_image_glow_spec(size, seed=s, **kw) for s in seeds)


def _ll64(specs, x, noise):
    """(components, n) float64 log-likelihoods of the oracle."""
    import torch
    from oracle import gbnf_oracle as oracle
    return np.stack([np.asarray(oracle.image_component_forward(sp, x, noise, dtype=torch.float64)[4], dtype=np.float64) for sp in specs])


@functools.lru_cache(maxsize=None)
def _rho_case(name, n):
    """(x, noise, float64 table) of a rho case: computed once, shared, left unchanged."""
    from gbnf_amd import synth
    x, noise = synth.synth_image_batch(n, RHO_CASES[name][0], seed=104)
    return x, noise, _ll64(_specs(name), x, noise)


@functools.lru_cache(maxsize=None)
def _flows(name):
    from gbnf_amd import native
    return tuple(native.NativeImageFlow(sp) for sp in _specs(name))


def _expect_rho(before, step_size, grad):
    """min(max(rho - step * grad, 0.01), 100) on the float32 values the kernel sees, in float64, rounded once."""
    return np.float32(min(max(float(before) - float(np.float32(step_size)) * float(grad), 0.01), 100.0))


@pytest.mark.parametrize("name,n", RHO_PARAMS)
def test_rho_step_against_float64(name, n):
    """1. C = 3, component = 2: the table and the gradient against float64, the clamp formula, both ends of the clamp, a NaN gradient for
    rho[1] > 1, component = 1."""
    import torch
    from gbnf_amd import native
    dev = _cuda()
    x, noise, ll64 = _rho_case(name, n)
    flows = _flows(name)
    xd, nd = _to(x, dev), _to(noise, dev)
    fixed64 = host.fixed_ll64(ll64, RHO0, 2)
    g64 = host.grad64(ll64, RHO0, 2)
    assert abs(g64 - GRAD64[(name, n)]) <= 1e-3 * abs(GRAD64[(name, n)]), "the oracle no longer gives the gradient this case was chosen for"
    assert np.isfinite(ll64).all()

    def run(step_size, rho_np=RHO0, component=2):
        rho = _to(rho_np.copy(), dev)
        stats = native.NativeImageFlow.rho_step(flows, xd, nd, component, rho, step_size).cpu().numpy()
        return stats, rho.cpu().numpy(), flows[component].rho_ll.cpu().double().numpy()

    step = 0.05 / abs(g64)
    stats, rho, ll = run(step)
    assert ll.shape == (3, n)
    rel = np.abs(ll - ll64) / np.abs(ll64)
    print(f"{name} n = {n}: worst relative ll error {rel.max():.3e}")
    assert (rel <= LL_RTOL).all()
    fixed = host.fixed_ll64(ll, RHO0, 2)
    g_dev = float(np.mean(fixed - ll[2]))
    bound = 1e-5 * max(np.abs(fixed).max(), np.abs(ll[2]).max())
    bound64 = 2e-5 * max(np.abs(fixed64).max(), np.abs(ll64[2]).max())
    print(f"{name} n = {n}: grad {stats[0]} vs {g_dev} on the device table (bound {bound:.3e}), vs {g64} of the oracle (bound {bound64:.3e})")
    assert abs(float(stats[0]) - g_dev) <= bound
    assert abs(float(stats[0]) - g64) <= bound64
    want = _expect_rho(RHO0[2], step, stats[0])
    assert stats[1] == RHO0[2] and stats[2] == rho[2]
    assert abs(float(rho[2]) - float(want)) <= float(np.spacing(want))
    assert 0.01 < rho[2] < 100.0 and rho[2] != RHO0[2], "the step was meant to move rho inside the clamp"
    assert stats[3] == np.abs(stats[2] - stats[1])
    assert (rho[:2] == RHO0[:2]).all()
    # both ends of the clamp
    sign = 1.0 if g64 > 0 else -1.0
    for step_size, end in ((sign * 1e6 / abs(g64), np.float32(0.01)), (-sign * 1e6 / abs(g64), np.float32(100.0))):
        s, r, _ = run(step_size)
        assert r[2] == end and s[2] == end and s[1] == RHO0[2] and (r[:2] == RHO0[:2]).all()
    # the reference's recursion does not normalise rho: rho[1] > 1 is the log of a negative number there, and here
    s, r, _ = run(step, np.array([1.0, 1.5, 0.25], dtype=np.float32))
    assert np.isnan(s[0]) and (r[:2] == [1.0, 1.5]).all()
    # component = 1: the recursion loop is empty, fixed_ll = ll_0
    s, r, t = run(0.001, component=1)
    assert t.shape == (2, n) and (np.abs(t - ll64[:2]) <= LL_RTOL * np.abs(ll64[:2])).all()
    g1 = float(np.mean(t[0] - t[1]))
    assert abs(float(s[0]) - g1) <= 1e-5 * np.abs(t).max()
    assert abs(float(s[0]) - host.grad64(ll64, RHO0, 1)) <= 2e-5 * np.abs(ll64[:2]).max()
    want = _expect_rho(RHO0[1], 0.001, s[0])
    assert s[1] == RHO0[1] and abs(float(r[1]) - float(want)) <= float(np.spacing(want)) and r[0] == RHO0[0] and r[2] == RHO0[2]


def _boost_case(name, dev):
    """(spec, x, noise, fixed spec) of a listed kink-free training case and a second component of its geometry (seed 2)."""
    from gbnf_amd import synth
    size, kw, _, _ = iso.STEP_CASES[name]
    sp, x, noise = iso.make_case(name)
    return sp, x, noise, synth.synth_image_glow_spec(size, seed=2, **kw)


def test_refusals():
    """2. Every GBNF_ERR_INVALID case of both calls: -1 with a message, nothing written; then one good call of each."""
    import torch
    from gbnf_amd import native
    dev = _cuda()
    L = native.lib()
    ptr = lambda t: C.c_void_p(t.data_ptr())
    x, noise, _ = _rho_case("2x8x12", 3)
    xd, nd = _to(x, dev), _to(noise, dev)
    n = x.shape[0]
    flows, other = _flows("2x8x12"), _flows("1x16x16")[0]
    arr = lambda fs: (C.c_void_p * len(fs))(*[f.handle.value if f is not None else None for f in fs])
    good = arr(flows)
    nb = C.c_int64()
    assert L.gbnf_image_rho_step_workspace_bytes(good, 3, n, C.byref(nb)) == 0
    per = []
    for f in flows:
        b = C.c_int64()
        assert L.gbnf_image_flow_workspace_bytes(f.handle, n, C.byref(b)) == 0
        per.append(b.value)
    a256 = lambda v: (v + 255) // 256 * 256
    assert nb.value == a256(max(per)) + a256(4 * n)
    ws = torch.empty(nb.value // 4 + 1, dtype=torch.float32, device=dev)
    rho = _to(RHO0.copy(), dev)
    stats = torch.full((4,), 7.0, dtype=torch.float32, device=dev)
    table = torch.full((3, n), 7.0, dtype=torch.float32, device=dev)

    def rho_call(flows_=good, component=2, x_=xd, n_=n, rho_=rho, table_=table, stats_=stats, ws_=ws, nbytes=nb.value):
        p = lambda t: ptr(t) if t is not None else None
        return L.gbnf_image_mixture_rho_step(flows_, component, p(x_), ptr(nd), n_, p(rho_), 0.1, p(table_), p(stats_), p(ws_), nbytes, None)

    bad = {"null flows": dict(flows_=None), "null x": dict(x_=None), "null rho": dict(rho_=None), "null table": dict(table_=None),
           "null stats": dict(stats_=None), "null workspace": dict(ws_=None), "null entry": dict(flows_=arr([flows[0], None, flows[2]])),
           "component 0": dict(component=0), "component -1": dict(component=-1), "n = 0": dict(n_=0),
           "shapes differ": dict(flows_=arr([flows[0], other, flows[2]])), "short workspace": dict(nbytes=nb.value - 256)}
    for what, kw in bad.items():
        assert rho_call(**kw) == -1, f"rho step, {what}: accepted"
        assert L.gbnf_last_error(), f"rho step, {what}: no message"
    assert L.gbnf_image_rho_step_workspace_bytes(arr([flows[0], other]), 2, n, C.byref(nb)) == -1
    torch.cuda.synchronize()
    assert (stats == 7.0).all() and (table == 7.0).all() and (rho.cpu().numpy() == RHO0).all()
    assert rho_call() == 0
    torch.cuda.synchronize()
    assert torch.isfinite(stats).all() and torch.isfinite(table).all() and float(rho[2]) != float(RHO0[2])

    # ---- the boosted step
    sp, xs, ns, fsp = _boost_case("A", dev)
    tr, tensors = _trainer(sp, dev)
    fixed = native.NativeImageFlow(fsp)
    xs_d, ns_d = _to(xs, dev), _to(ns, dev)
    m = xs.shape[0]
    assert L.gbnf_image_boosted_step_workspace_bytes(fixed.handle, tr.handle, m, C.byref(nb)) == 0
    ws = torch.empty(nb.value // 4 + 1, dtype=torch.float32, device=dev)
    flat = torch.full((tr.step_grad_floats,), 7.0, dtype=torch.float32, device=dev)
    stats = torch.full((8,), 7.0, dtype=torch.float32, device=dev)
    before = {p: t.clone() for p, t in tensors.items()}
    sgd = native._OptHyper(kind=native.OPT_KIND["sgd"], step=1, lr=LR)
    adamw = native._OptHyper(kind=native.OPT_KIND["adamw"], step=1, lr=LR, beta1=0.9, beta2=0.999, eps=1e-8)

    def step_call(fixed_=fixed.handle, tr_=tr.handle, x_=xs_d, n_=m, flat_=flat, h=sgd, stats_=stats, ws_=ws, nbytes=nb.value):
        p = lambda t: ptr(t) if t is not None else None
        return L.gbnf_image_boosted_nll_step(fixed_, -10.0, tr_, p(x_), ptr(ns_d), n_, 1.0, p(flat_), None, None,
                                             C.byref(h) if h is not None else None, p(stats_), p(ws_), nbytes, None)

    bad = {"null fixed": dict(fixed_=None), "null trainer": dict(tr_=None), "null x": dict(x_=None), "null grads": dict(flat_=None),
           "null stats": dict(stats_=None), "null workspace": dict(ws_=None), "n = 0": dict(n_=0), "n = 65536": dict(n_=65536),
           "null hyper": dict(h=None), "AdamW without moments": dict(h=adamw), "fixed of another shape": dict(fixed_=other.handle),
           "short workspace": dict(nbytes=nb.value - 256)}
    for what, kw in bad.items():
        assert step_call(**kw) == -1, f"boosted step, {what}: accepted"
        assert L.gbnf_last_error(), f"boosted step, {what}: no message"
    small = C.c_int64()
    assert L.gbnf_image_boosted_step_workspace_bytes(other.handle, tr.handle, m, C.byref(small)) == -1
    assert L.gbnf_image_boosted_step_workspace_bytes(fixed.handle, tr.handle, 0, C.byref(small)) == -1
    torch.cuda.synchronize()
    assert (stats == 7.0).all() and (flat == 7.0).all()
    assert all(torch.equal(t, before[p]) for p, t in tensors.items())
    assert step_call() == 0
    torch.cuda.synchronize()
    assert torch.isfinite(stats).all() and torch.isfinite(flat).all() and float(stats[7]) == 0.0
    assert any(not torch.equal(t, before[p]) for p, t in tensors.items())


@pytest.mark.parametrize("name", ["A", "F"])
def test_the_boosted_step_is_its_parts(name):
    """3. boosted_nll_step on one trainer, nll_step on its twin: the same parameters and statistics; the G term against float64, with
    no floor, the reference's floor, and floors between, below and above the rows.  SGD (with weight decay and clipping): the two
    trainers run the backward pass independently, its weight gradients are summed with float atomics, and SGD is linear in them --
    AdamW's first step is sign(g), which turns the rounding of a near-zero entry into a full step."""
    import torch
    from gbnf_amd import native
    dev = _cuda()
    sp, x, noise, fsp = _boost_case(name, dev)
    n = x.shape[0]
    xd, nd = _to(x, dev), _to(noise, dev)
    fixed = native.NativeImageFlow(fsp)
    llG = _ll64((fsp,), x, noise)[0]
    assert np.isfinite(llG).all() and llG.max() < -100.0
    k = 1.0 / (math.log(2.0) * float(np.prod(sp["input_size"])))
    tr_a, tensors_a = _trainer(sp, dev)
    tr_b, tensors_b = _trainer(sp, dev)
    before = {p: t.clone() for p, t in tensors_a.items()}
    probe, _ = tr_b.nll_step(xd, nd, native.OptState(tr_b, "sgd"), loss_scale=k, lr=0.0)
    hyper = dict(loss_scale=k, lr=LR, weight_decay=1e-3, max_grad_norm=0.5 * float(probe[1]))
    sa, _ = tr_a.boosted_nll_step(fixed, xd, nd, native.OptState(tr_a, "sgd"), g_floor=-math.inf, **hyper)
    sb, _ = tr_b.nll_step(xd, nd, native.OptState(tr_b, "sgd"), **hyper)
    sa, sb = sa.cpu().numpy(), sb.cpu().numpy()
    print(f"{name}: boosted stats {sa}, plain stats {sb}, float64 G_nll {-llG.mean()}")
    assert sa.shape == (8,) and sb.shape == (4,)
    assert abs(float(sa[2]) - 0.5) <= 1e-4, "the step was meant to clip"
    for i in range(4):
        assert abs(float(sa[i]) - float(sb[i])) <= PARAM_TOL * abs(float(sb[i])), f"stats[{i}]"
    for path in tensors_a:
        _assert_close(tensors_a[path], tensors_b[path], str(path))
    assert any(not torch.equal(t, before[p]) for p, t in tensors_a.items()), "the step did not move the parameters"

    def check(s, floor):
        g64 = float(np.mean(-np.maximum(llG, floor)))
        count = int(np.sum(llG < floor))
        assert np.all(np.abs(llG - floor) > 1e-5 * np.abs(llG)), "the floor is too close to a row for the count to be decided"
        assert abs(float(s[4]) - g64) <= LL_RTOL * abs(g64), f"floor {floor}: G_nll {s[4]} vs {g64}"
        assert float(s[6]) == count, f"floor {floor}: count {s[6]} vs {count}"
        want5 = np.float32(s[0]) - np.float32(s[4])
        assert abs(float(s[5]) - float(want5)) <= float(np.spacing(np.abs(want5))), f"floor {floor}: stats[5] {s[5]} vs {want5}"
        assert float(s[7]) == 0.0

    check(sa, -math.inf)
    frozen = native.OptState(tr_a, "sgd")

    def at(floor):
        return tr_a.boosted_nll_step(fixed, xd, nd, frozen, g_floor=floor, loss_scale=k, lr=0.0)[0].cpu().numpy()

    s = at(-10.0)                      # the reference's G_MAX_LOSS: every image ll lies far below it
    assert float(s[4]) == 10.0 and float(s[6]) == n
    check(s, -10.0)
    rows = np.sort(llG)
    floors = [2.0 * rows[0], 0.5 * rows[-1]]             # below every row, above every row
    if n >= 2:                                           # the largest gap between two rows
        j = int(np.argmax(np.diff(rows)))
        floors.append(0.5 * (rows[j] + rows[j + 1]))
    for floor in floors:
        check(at(float(np.float32(floor))), float(np.float32(floor)))


def _module(dev, rho_lr):
    """A 3-component BoostedImageFlow of the 2x8x12 geometry with the three specs loaded, at component 2."""
    import torch
    from gbnf_amd import BoostedFlow, image_glow
    size, kw, _ = RHO_CASES["2x8x12"]
    torch.manual_seed(0)
    m = BoostedFlow(host.image_args(size, kw["h"], kw["K"], kw["L"], dev, C_=3, rho_iters=12, rho_lr=rho_lr))
    for c, sp in enumerate(_specs("2x8x12")):
        image_glow.load_image_spec(m.flows[c], sp)
    m.component = 2
    return m


class _Loader:
    """A list of batches that counts what it hands out."""

    def __init__(self, batches):
        self.batches, self.served = batches, 0

    def __iter__(self):
        for b in self.batches:
            self.served += 1
            yield b


def test_module_update_rho_against_the_replay():
    """4a. update_rho over 12 iterations against the float64 replay on the oracle's log-likelihoods of the same batches and noise."""
    import torch
    from gbnf_amd import native, synth
    dev = _cuda()
    size = RHO_CASES["2x8x12"][0]
    rho_lr = 0.01
    m = _module(dev, rho_lr)
    assert (m.rho.cpu().numpy() == RHO0).all()
    xs = [synth.synth_image_batch(5, size, seed=s)[0] for s in (104, 105)]
    loader = _Loader([(_to(x, dev), None) for x in xs])
    version = m.rho._version
    m.train()
    m.update_rho(loader, noise_generator=torch.Generator(device=dev).manual_seed(7))
    assert not m.training
    g = torch.Generator(device=dev).manual_seed(7)
    noises = [torch.rand(xs[k % 2].shape, generator=g, device=dev).cpu().numpy() for k in range(12)]
    tables = [_ll64(_specs("2x8x12"), xs[k % 2], noises[k]) for k in range(12)]
    r = host.replay_update_rho(tables, RHO0, 2, rho_lr, 12)
    print(f"replay: rho {r['rho']} after {r['iters']} iterations, difs {r['difs']}")
    assert r["difs"][11] >= 2 * host.TOLERANCE or r["difs"][11] <= 0.5 * host.TOLERANCE, "the stop rule could flip on rounding"
    assert 0.01 < r["rho"] < 100.0 and all(0.01 < v < 100.0 for v in r["rhos"]), "the replay was meant to stay inside the clamp"
    assert loader.served == r["iters"] == 12
    rho = m.rho.cpu().numpy()
    worst = max(np.abs(t).max() for t in tables)
    bound = sum(r["steps"]) * 2e-5 * worst + r["iters"] * float(np.spacing(np.float32(max(r["rhos"] + [float(RHO0[2])]))))
    print(f"module: rho[2] {rho[2]} vs {r['rho']} (bound {bound:.3e})")
    assert abs(float(rho[2]) - r["rho"]) <= bound
    assert (rho[:2] == RHO0[:2]).all() and m.rho._version > version
    # _rho_gradients against the library call on the same input
    xd, nd = _to(xs[0], dev), _to(noises[0], dev)
    new_ll, fixed_ll, full_ll = m._rho_gradients(xd, nd)
    scratch = m.rho.clone()
    stats = native.NativeImageFlow.rho_step([m.native_flow(c) for c in range(3)], xd, nd, 2, scratch, 0.0).cpu().numpy()
    g_mod = float((fixed_ll.double() - new_ll.double()).mean())
    assert abs(g_mod - float(stats[0])) <= 1e-5 * max(float(fixed_ll.abs().max()), float(new_ll.abs().max()))
    assert new_ll.shape == fixed_ll.shape == full_ll.shape == (5,) and torch.isfinite(full_ll).all()


def test_module_update_rho_guards():
    """4b. component 0 before all_trained and rho_iters = 0 leave rho alone and never touch the loader; component 0 of a second pass
    clamps rho[0]; a rho that is not contiguous float32 is refused."""
    import torch
    dev = _cuda()
    m = _module(dev, 0.01)

    class Untouchable:
        def __iter__(self):
            raise AssertionError("the loader was read")

    with torch.no_grad():
        m.rho[0] = 500.0
    m.component, m.all_trained = 0, False
    m.update_rho(Untouchable())
    assert float(m.rho[0]) == 500.0
    m.all_trained, m.args.rho_iters = True, 0
    m.update_rho(Untouchable())
    assert float(m.rho[0]) == 500.0
    m.args.rho_iters = 12
    m.update_rho(Untouchable())
    assert m.rho.cpu().tolist() == [100.0, 0.5, 0.25]
    m.component = 2
    m.rho = m.rho.double()
    with pytest.raises(ValueError, match="float32"):
        m.update_rho(Untouchable())


def test_module_training_step_with_a_fixed_component():
    """4c. fixed=None keeps today's keys; fixed=1 and fixed="sample" add the boosted loss; component 2 moves, the others do not."""
    import torch
    from gbnf_amd import synth
    dev = _cuda()
    m = _module(dev, 0.01)
    m.train()
    x, noise = synth.synth_image_batch(5, RHO_CASES["2x8x12"][0], seed=104)
    xd, nd = _to(x, dev), _to(noise, dev)
    frozen = [[p.detach().clone() for p in m.flows[c].parameters()] for c in (0, 1)]
    before = [p.detach().clone() for p in m.flows[2].parameters()]
    out = m.training_step(xd, noise=nd, lr=LR)
    assert set(out) == {"nll", "bpd", "grad_norm", "clip_coef"}
    per_dim = 1.0 / (math.log(2.0) * 2 * 8 * 12)
    for fixed, allowed in ((1, {1}), ("sample", {0, 1})):
        out = m.training_step(xd, noise=nd, lr=LR, fixed=fixed)
        assert set(out) == {"nll", "bpd", "grad_norm", "clip_coef", "G_nll", "boosted_nll", "boosted_bpd", "fixed_component"}
        assert isinstance(out["fixed_component"], int) and out["fixed_component"] in allowed
        for key in ("nll", "bpd", "grad_norm", "clip_coef", "G_nll", "boosted_nll", "boosted_bpd"):
            assert out[key].dim() == 0 and out[key].is_cuda and bool(torch.isfinite(out[key])), key
        assert float(out["G_nll"]) == 10.0           # every image ll lies far below the reference's floor of -10
        assert abs(float(out["boosted_nll"]) - (float(out["nll"]) - 10.0)) <= 1e-6 * abs(float(out["nll"]))
        assert abs(float(out["boosted_bpd"]) - float(out["boosted_nll"]) * per_dim) <= 1e-6 * abs(float(out["boosted_bpd"]))
    assert m.opt_state(2).step == 3
    assert any(not torch.equal(a, b) for a, b in zip(before, m.flows[2].parameters()))
    assert all(torch.equal(a, b) for c in (0, 1) for a, b in zip(frozen[c], m.flows[c].parameters()))
    with pytest.raises(ValueError):
        m.training_step(xd, noise=nd, lr=LR, fixed=3)
    with pytest.raises(ValueError):
        m.training_step(xd, noise=nd, lr=LR, fixed="all")
