"""GPU: what boosting adds to a training step (csrc/gbnf_boost.hip) -- gbnf_resample_rows against the float64 numpy definition of
tests/test_boost_host.py, gbnf_boosted_nll_step against the sequence of calls it stands for, gbnf_mixture_rho_step against float64 on
the device's own log-likelihood table, and the two module entries (BoostedFlow.training_step(uniforms=), update_rho(fused=True)).

Bounds.  Rows: equal, outside the reference's own 1e-9 margin around a cdf entry (f64 sums in another order differ by ~1e-16 T).
Frequencies: the 6-sigma binomial bound.  One call against its parts: PARAM_TOL of test_hip_fused_step (same kernels on the same rows;
only the float atomics of the weight gradients may differ).  rho_step: the gradient is a mean of differences of log-likelihoods each
good to the project's 1e-5 relative bar, so |grad - grad64| <= 1e-5 x max(|fixed_ll|, |new_ll|)."""
import ctypes as C

import numpy as np
import pytest

from test_boost_host import (FREQ_M, MAX_EXCLUDED, RESAMPLE_CASES, case_seed, frequency_case, frequency_violations, reference_rows,
                             seeded_G, seeded_uniforms)
from test_hip_fused_step import PARAM_TOL, _assert_close
from test_hip_train import _args, _dev_spec

pytestmark = pytest.mark.gpu
LR = 1e-3


def _dev():
    import torch
    return torch.device("cuda:0")


def _shaped_device_weights(n, seed, dev):
    """boosting_weights of seeded G on the device; every 7th row gets none, and the sum is not 1."""
    import torch
    from gbnf_amd import native
    w = native.boosting_weights(torch.from_numpy(seeded_G(n, seed)).to(dev)) * 0.75
    w[6::7] = 0.0
    return w.contiguous()


def _rows(w, u):
    import torch
    from gbnf_amd import native
    dev = _dev()
    return native.resample_rows(torch.from_numpy(np.ascontiguousarray(w, dtype=np.float32)).to(dev),
                                torch.from_numpy(np.ascontiguousarray(u, dtype=np.float32)).to(dev)).cpu().numpy()


@pytest.mark.parametrize("n,m", RESAMPLE_CASES)
def test_resampler_matches_the_float64_reference(n, m):
    """1. Every draw outside the margin lands on the reference's row; no row without weight is drawn."""
    import torch
    from gbnf_amd import native
    dev = _dev()
    w = _shaped_device_weights(n, case_seed(n, m), dev)
    u = seeded_uniforms(m, case_seed(n, m))
    rows = native.resample_rows(w, torch.from_numpy(u).to(dev)).cpu().numpy()
    w = w.cpu().numpy()
    ref, near = reference_rows(w, u)
    print(f"n = {n}, m = {m}: {int(near.sum())} draws within the margin, {int((rows != ref)[~near].sum())} others differ")
    assert near.sum() <= MAX_EXCLUDED * m
    assert rows.dtype == np.int64 and rows.min() >= 0 and rows.max() < n
    assert (w[rows] > 0).all()
    assert (rows[~near] == ref[~near]).all()


def test_resampler_exact_uniform_weights_pin_the_strict_comparison():
    """1. w = 1/512, u = k/512: exact in every operation, no exclusion: u * T == cdf_{k-1} belongs to row k."""
    w = np.full(512, 1.0 / 512, dtype=np.float32)
    u = (np.arange(512) / 512.0).astype(np.float32)
    assert (_rows(w, u) == np.arange(512)).all()
    assert (_rows(w, u) == reference_rows(w, u)[0]).all()


def test_resampler_edges():
    """2. The ends of the cdf, one heavy row, out-of-contract inputs, run-to-run identity."""
    import torch
    from gbnf_amd import native
    dev = _dev()
    n, m = 1025, 1000
    w = _shaped_device_weights(n, 5, dev).cpu().numpy()
    w[:3] = 0.0
    w[-5:] = 0.0
    w[-6] = 0.01
    first, last = int(np.nonzero(w > 0)[0][0]), int(np.nonzero(w > 0)[0][-1])
    assert first == 3 and last == n - 6
    below_one = np.nextafter(np.float32(1.0), np.float32(0.0))
    assert (_rows(w, np.zeros(7, dtype=np.float32)) == first).all()
    assert (_rows(w, np.full(7, below_one, dtype=np.float32)) == last).all()
    u = seeded_uniforms(m, 9)
    one = np.zeros(n, dtype=np.float32)
    one[37] = 2.5
    assert (_rows(one, u) == 37).all()
    # out of contract: the indices stay valid and on rows that have weight
    assert (_rows(w, np.array([1.0, 1.5, np.inf, np.nan, -0.5, -np.inf], dtype=np.float32)) == [last, last, last, last, first, first]).all()
    bad = w.copy()
    bad[10], bad[20], bad[30], bad[n - 6] = np.nan, -3.0, np.inf, -np.inf
    rows = _rows(bad, np.concatenate([u, [1.0, np.nan]]).astype(np.float32))
    assert rows.min() >= 0 and rows.max() < n
    assert (np.isfinite(bad[rows]) & (bad[rows] > 0)).all()
    ref, near = reference_rows(bad, u)
    assert (rows[:m][~near] == ref[~near]).all()
    # no weight anywhere: row i % n
    assert (_rows(np.zeros(5, dtype=np.float32), u[:12]) == np.arange(12) % 5).all()
    assert (_rows(np.full(5, np.nan, dtype=np.float32), u[:12]) == np.arange(12) % 5).all()
    # two runs, bit for bit (70 001 rows: 69 per thread of the scan)
    wd = _shaped_device_weights(70001, 2, dev)
    ud = torch.from_numpy(seeded_uniforms(8192, 2)).to(dev)
    assert torch.equal(native.resample_rows(wd, ud), native.resample_rows(wd, ud))


def test_resampler_frequencies():
    """3. n = 64, 2^18 draws on seeded torch.rand: every row's count within the 6-sigma binomial bound."""
    import torch
    from gbnf_amd import native
    dev = _dev()
    w, _ = frequency_case()
    u = torch.rand(FREQ_M, device=dev, generator=torch.Generator(device=dev).manual_seed(1234))
    rows = native.resample_rows(torch.from_numpy(w).to(dev), u).cpu().numpy()
    assert frequency_violations(rows, w, FREQ_M).size == 0
    assert (w[rows] > 0).all()


BOOST_GEOMETRIES = {
    "glow_d8_h32_K3_C2_n512": ("glow", 8, 32, 3, 2, 1, 512),
    "realnvp_d6_h30_K2_bn_C3_n96": ("realnvp", 6, 30, 2, 3, 2, 96),       # batch-statistics BatchNorm, a ragged batch
}


def _boost_setup(name, dev, trainers=2):
    """(mixture of all C components, n_fixed, rho, x, trainers of component n_fixed on their own parameter copies, BatchNorm momentum)."""
    import torch
    from gbnf_amd import native, synth
    kind, d, h, K, n_comp, n_fixed, n = BOOST_GEOMETRIES[name]
    specs = synth.synth_boosted_specs(kind, n_comp, d, h, K, seed=3)
    mix, _ = native.mixture_from_specs(specs)
    out = []
    for _ in range(trainers):
        ds = _dev_spec(specs[n_fixed], dev)
        bns = [st["bn"] for st in ds["steps"] if st.get("bn") is not None]
        for bn in bns:
            bn["batch_mean"] = torch.zeros(d, device=dev)
            bn["batch_var"] = torch.zeros(d, device=dev)
        tr = native.NativeTrainer(ds)
        if bns:
            assert tr.has_batch_stats
            tr.set_batch_stats(True)
        out.append(tr)
    rho = torch.tensor([1.0, 0.5, 0.25][:n_comp], device=dev)
    x = torch.from_numpy(synth.synth_batch(n, d, seed=2)).to(dev)
    return mix, n_fixed, rho, x, out, (0.9 if kind == "realnvp" else -1.0)


@pytest.mark.parametrize("name", sorted(BOOST_GEOMETRIES))
def test_one_call_equals_the_composed_sequence(name):
    """4. boosted_nll_step(u) == mixture.log_prob -> boosting_weights -> resample_rows(u) -> nll_step(rows)."""
    import torch
    from gbnf_amd import native
    dev = _dev()
    mix, n_fixed, rho, x, (tr_a, tr_b), momentum = _boost_setup(name, dev)
    n = x.shape[0]
    u = torch.from_numpy(seeded_uniforms(n, 31)).to(dev)
    hyper = dict(lr=LR, weight_decay=1e-5, max_grad_norm=5.0, bn_momentum=momentum)
    G_before, _ = mix.log_prob(x, rho, n_used=n_fixed)
    G_before = G_before.clone()
    state_a, state_b = native.OptState(tr_a, "adamw"), native.OptState(tr_b, "adamw")

    stats_a, flat_a, rows_a = tr_a.boosted_nll_step(mix, n_fixed, rho, x, u, state_a, want_rows=True, **hyper)
    G, _ = mix.log_prob(x, rho, n_used=n_fixed)
    w = native.boosting_weights(G)
    rows_b = native.resample_rows(w, u)
    stats_b, flat_b = tr_b.nll_step(x, state_b, rows=rows_b, **hyper)

    assert state_a.step == 1 and stats_a.shape == (8,)
    assert torch.equal(rows_a, rows_b)
    assert rows_a.unique().numel() < n                      # drawn with replacement
    sa, sb = stats_a.cpu().double().numpy(), stats_b.cpu().double().numpy()
    print(f"{name}: stats one call {sa}, composed {sb}")
    assert np.isfinite(sa).all()
    for k in range(3):
        assert abs(sa[k] - sb[k]) <= PARAM_TOL * abs(sb[k]), f"stats[{k}]: {sa[k]} vs {sb[k]}"
    assert sa[3] == 0.0 and sa[7] == 0.0
    for k, (a, b) in enumerate(zip(tr_a.params, tr_b.params)):
        if a is not None:
            _assert_close(a, b, f"parameter {k}")
    _assert_close(state_a.exp_avg, state_b.exp_avg, "exp_avg")
    _assert_close(state_a.exp_avg_sq, state_b.exp_avg_sq, "exp_avg_sq")
    G64, w64 = G.cpu().double().numpy(), w.cpu().double().numpy()
    assert abs(sa[4] - (-G64.mean())) <= 1e-6 * abs(G64.mean())
    ess = w64.sum() ** 2 / (w64 * w64).sum()
    assert abs(sa[5] - ess) <= 1e-5 * ess and 1.0 <= sa[5] <= n * (1 + 1e-5)
    assert sa[6] == 0.0
    # the fixed components were only read
    G_after, _ = mix.log_prob(x, rho, n_used=n_fixed)
    assert torch.equal(G_before, G_after) and torch.equal(G_before, G)


def test_boosted_step_argument_validation():
    """5. Bad arguments: GBNF_ERR_INVALID with a message, nothing launched (parameters, gradient buffer and stats untouched)."""
    import torch
    from gbnf_amd import native, synth
    dev = _dev()
    L = native.lib()
    mix, n_fixed, rho, x, (tr,), _ = _boost_setup("glow_d8_h32_K3_C2_n512", dev, trainers=1)
    other, _ = native.mixture_from_specs(synth.synth_boosted_specs("glow", 1, 6, 30, 2, seed=3))       # d = 6: not the trainer's
    before = [t.clone() for t in tr.params]
    n = x.shape[0]
    u = torch.rand(n, device=dev)
    flat = torch.ones(tr.grad_floats, device=dev)
    m, v = torch.zeros_like(flat), torch.zeros_like(flat)
    stats = torch.full((8,), -7.0, device=dev)
    rows = torch.full((n,), -5, dtype=torch.int64, device=dev)
    nb = C.c_int64()
    assert L.gbnf_boosted_step_workspace_bytes(mix.handle, n_fixed, tr.handle, n, C.byref(nb)) == 0
    step_nb = C.c_int64()
    assert L.gbnf_trainer_step_workspace_bytes(tr.handle, n, C.byref(step_nb)) == 0
    # the nll_step workspace, the (n_fixed, n) table, G, w, the cdf and the rows; n = 512: every piece is a multiple of 256 bytes
    assert nb.value == step_nb.value + n_fixed * n * 4 + 2 * n * 4 + 2 * n * 8
    ws = torch.empty(nb.value // 8, dtype=torch.float64, device=dev)
    ptr = lambda t: C.c_void_p(t.data_ptr()) if t is not None else C.c_void_p(0)
    hyper = lambda **kw: native._OptHyper(**{**dict(kind=1, step=1, lr=1e-3, beta1=0.9, beta2=0.999, eps=1e-8, bn_momentum=-1.0), **kw})

    def step(h, mix_=mix.handle, nf=n_fixed, rho_=rho, tr_=tr.handle, x_=x, n_=n, u_=u, flat_=flat, m_=m, v_=v, stats_=stats, ws_=ws,
             ws_bytes=None):
        return L.gbnf_boosted_nll_step(mix_, nf, ptr(rho_), 1.0, tr_, ptr(x_), n_, ptr(u_), ptr(flat_), ptr(m_), ptr(v_),
                                       C.byref(h) if h is not None else None, ptr(stats_), ptr(rows), ptr(ws_),
                                       nb.value if ws_bytes is None else ws_bytes, None)

    bad = [lambda: step(hyper(kind=2)), lambda: step(hyper(), m_=None), lambda: step(hyper(), v_=None), lambda: step(hyper(step=0)),
           lambda: step(None), lambda: step(hyper(), ws_bytes=nb.value - 256), lambda: step(hyper(), n_=0),
           lambda: step(hyper(), nf=0), lambda: step(hyper(), nf=mix.n_components + 1), lambda: step(hyper(), mix_=other.handle),
           lambda: step(hyper(), u_=None), lambda: step(hyper(), x_=None), lambda: step(hyper(), rho_=None),
           lambda: step(hyper(), tr_=None), lambda: step(hyper(), mix_=None), lambda: step(hyper(), flat_=None),
           lambda: step(hyper(), stats_=None), lambda: step(hyper(), ws_=None)]
    for k, call in enumerate(bad):
        assert call() == -1, f"bad call {k} was accepted"
        assert L.gbnf_last_error(), f"bad call {k} left no message"
    assert L.gbnf_boosted_step_workspace_bytes(other.handle, 1, tr.handle, n, C.byref(nb)) == -1
    torch.cuda.synchronize()
    assert all(torch.equal(a, b) for a, b in zip(before, tr.params))
    assert torch.equal(stats, torch.full((8,), -7.0, device=dev)) and not m.any() and torch.equal(flat, torch.ones_like(flat))
    assert (rows == -5).all()
    nb = C.c_int64(ws.numel() * 8)
    assert step(hyper()) == 0
    torch.cuda.synchronize()
    assert torch.isfinite(stats).all() and float(stats[1]) > 0 and int(rows.min()) >= 0 and int(rows.max()) < n


@pytest.mark.parametrize("n", [33, 512])
def test_rho_step(n):
    """6. C = 3, component = 2: the gradient against float64 on the device's own table, the clamp formula, both ends of the clamp."""
    import torch
    from gbnf_amd import native, synth
    dev = _dev()
    mix, _ = native.mixture_from_specs(synth.synth_boosted_specs("glow", 3, 8, 32, 3, seed=3))
    x = torch.from_numpy(synth.synth_batch(n, 8, seed=4)).to(dev)
    rho0 = np.array([1.0, 0.5, 0.25], dtype=np.float32)

    def run(step_size, rho_np=rho0):
        rho = torch.from_numpy(rho_np.copy()).to(dev)
        stats = mix.rho_step(x, 2, rho, step_size).cpu().numpy()
        return stats, rho.cpu().numpy(), mix.rho_ll.cpu().double().numpy()

    stats, rho, ll = run(0.1)
    assert ll.shape == (3, n)
    fixed = np.logaddexp(np.log(1.0 - np.float64(rho0[1])) + ll[0], np.log(np.float64(rho0[1])) + ll[1])
    grad64 = float(np.mean(fixed - ll[2]))
    bound = 1e-5 * max(np.abs(fixed).max(), np.abs(ll[2]).max())
    print(f"n = {n}: grad {stats[0]} vs {grad64} (bound {bound})")
    assert abs(float(stats[0]) - grad64) <= bound

    def expect(before, step_size, grad):
        return np.float32(min(max(float(before) - float(np.float32(step_size)) * float(grad), 0.01), 100.0))

    want = expect(rho0[2], 0.1, stats[0])
    assert stats[1] == rho0[2] and stats[2] == rho[2]
    assert abs(float(rho[2]) - float(want)) <= float(np.spacing(want))
    assert 0.01 < rho[2] < 100.0 and rho[2] != rho0[2], "the step was meant to move rho inside the clamp"
    assert stats[3] == np.abs(stats[2] - stats[1])
    assert (rho[:2] == rho0[:2]).all()
    # both ends of the clamp
    sign = 1.0 if stats[0] > 0 else -1.0
    for step_size, end in ((sign * 1e6, np.float32(0.01)), (-sign * 1e6, np.float32(100.0))):
        s, r, _ = run(step_size)
        assert r[2] == end and s[2] == end and (r[:2] == rho0[:2]).all()
    # the reference's recursion does not normalise rho: rho[1] > 1 is log of a negative number there, and here
    s, r, _ = run(0.1, np.array([1.0, 1.5, 0.25], dtype=np.float32))
    assert np.isnan(s[0]) and (r[:2] == [1.0, 1.5]).all()


def _module(C_, dev, n=512):
    """A BoostedFlow of C_ Glow components, every component trained one step in turn (ActNorm initialised), at component C_ - 1."""
    import torch
    from gbnf_amd import BoostedFlow
    torch.manual_seed(0)
    m = BoostedFlow(_args("glow", 8, 32, 3, C_, dev)).to(dev)
    m.train()
    x = torch.randn(n, 8, device=dev) * torch.linspace(0.5, 2.0, 8, device=dev) + 0.3
    for c in range(C_):
        m.component = c
        m.training_step(x, lr=5e-3)
    return m, x


def test_module_training_step_on_uniforms():
    """7. training_step(uniforms=u) at component 1: five finite entries, component 1 moves, component 0 does not; the default path
    keeps its keys."""
    import torch
    dev = _dev()
    m, x = _module(2, dev)
    assert m.component == 1
    params = list(m.flows[1].parameters())
    before = [p.clone() for p in params]
    versions = [p._version for p in params]
    fixed = [p.clone() for p in m.flows[0].parameters()]
    u = torch.rand(x.shape[0], device=dev, generator=torch.Generator(device=dev).manual_seed(5))
    for uniforms in (u, True):
        out = m.training_step(x, lr=5e-3, max_grad_norm=5.0, uniforms=uniforms)
        assert set(out) == {"nll", "grad_norm", "clip_coef", "G_nll", "ess"}
        assert all(v.dim() == 0 and v.is_cuda and torch.isfinite(v).item() for v in out.values())
        assert 1.0 <= out["ess"].item() <= x.shape[0] * (1 + 1e-5)
    assert any(not torch.equal(a, b) for a, b in zip(before, params))
    assert all(p._version > v for p, v in zip(params, versions))
    assert all(torch.equal(a, b) for a, b in zip(fixed, m.flows[0].parameters()))
    assert m.opt_state(1).step == 3
    torch.manual_seed(0)
    out = m.training_step(x, lr=5e-3, max_grad_norm=5.0)
    assert set(out) == {"nll", "grad_norm", "clip_coef", "G_nll"}
    with pytest.raises(ValueError):
        m.training_step(x, lr=5e-3, uniforms=u[:-1])


def test_module_update_rho_fused():
    """7. update_rho(fused=True) against the eager loop on the same three batches, rho_iters = 12 (neither loop can stop before its
    12th iteration).  rho[component] is never read by the recursion, so the two runs differ by sum_it step_it |grad - grad'| at most,
    each gradient good to 1e-5 x max|ll|."""
    import torch
    dev = _dev()
    m, x = _module(3, dev, n=256)
    m.args.rho_iters, m.args.rho_lr = 12, 0.1
    g = torch.Generator(device=dev).manual_seed(8)
    loader = [(x[:128].clone(), None), (x[128:].clone(), None),
              (torch.randn(128, 8, device=dev, generator=g) * torch.linspace(0.5, 2.0, 8, device=dev) + 0.3, None)]
    rho0 = m.rho.clone()
    m.update_rho(loader)
    eager = m.rho.clone()
    with torch.no_grad():
        m.rho.copy_(rho0)
    version = m.rho._version
    m.update_rho(loader, fused=True)
    fused = m.rho.clone()
    assert m.rho._version > version
    ll_max = max(float(m.component_log_prob(b, n_used=3).abs().max()) for b, _ in loader)
    tol = sum(0.1 / (0.05 * it + 1) for it in range(12)) * 1e-5 * ll_max
    print(f"rho eager {eager.tolist()}, fused {fused.tolist()}, tolerance {tol}")
    assert torch.equal(fused[:2], rho0[:2]) and torch.equal(eager[:2], rho0[:2])
    assert abs(float(fused[2]) - float(eager[2])) <= tol
    assert 0.01 <= float(fused[2]) <= 100.0 and float(fused[2]) != float(rho0[2])
