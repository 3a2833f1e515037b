"""GPU: the validation pass on the device -- gbnf_eval_accumulate / gbnf_eval_accumulate_class_loss (csrc/gbnf_eval.hip), the one-call
forms gbnf_mixture_evaluate and gbnf_image_mixture_evaluate[_y], and BoostedFlow.evaluate / BoostedImageFlow.evaluate -- against the
float64 yardstick of tests/eval_oracle.py and against the eager loops the reference's two ``evaluate`` functions run.

Bounds.  A sum of n values v_i in double, in ANY order, lies within n 2^-52 sum|v_i| of the exact sum (each of the n - 1 additions adds
at most 2^-53 of a partial sum that is at most sum|v_i|); a dropped or doubled row is off by about |v|, orders of magnitude more.  That
is the bound wherever the device's own float32 per-row values are available (G_out, the table); per-row values the device forms in
double (E_ll, w CE) are elementwise IEEE arithmetic in index order, restated the same way by the yardstick.  Against float64
log-likelihoods the bound is the project's parity bar, 1e-5 max|ll|."""
import ctypes as C
import functools
import math

import numpy as np
import pytest

import eval_oracle as eo
from conftest import rel_err

pytestmark = pytest.mark.gpu

EPS = 2.0 ** -52
LL_RTOL = 1e-5
RHO3 = np.array([1.0, 0.5, 0.25], dtype=np.float32)


def _cuda():
    import torch
    return torch.device("cuda:0")


def _to(a, dev):
    import torch
    return torch.from_numpy(np.ascontiguousarray(a)).to(dev)


def _table(n, C_=3, seed=0):
    rng = np.random.RandomState(seed)
    return (rng.standard_normal((C_, n)) * 50.0 - 100.0).astype(np.float32)


def _wrap_n():
    from gbnf_amd import native
    return native.EVAL_MAX_PARTIALS * native.EVAL_ROWS_PER_WORKGROUP + 7


def _sum_bound(v):
    v = np.asarray(v, dtype=np.float64)
    return v.size * EPS * float(np.abs(v).sum())


def _check_state_against_device_values(s, ll, G, rho, component):
    """Entries 0 - 9 of a one-batch state against float64 sums of the device's own float32 values."""
    n = ll.shape[1]
    g = ll[component]
    per_row = {2: G, 3: g, 4: (G - g), 5: eo.expected_ll(ll, rho)}      # (G - g in float32, as the device forms it)
    assert s[0] == n and s[1] == 1
    for k, v in per_row.items():
        want, bound = eo.fsum(v), _sum_bound(v)
        print(f"n = {n}: state[{k}] {s[k]!r} vs {want!r} (bound {bound:.3e}, off by {abs(s[k] - want):.3e})")
        assert abs(s[k] - want) <= bound, k
    for k, src in ((6, 2), (7, 3), (8, 5)):                              # the batch means: the device's own sum, one division
        assert abs(s[k] - s[src] / n) <= abs(s[src] / n) * EPS, k
    assert s[9] == 0 and (s[10:] == 0).all()


# ---- 1. eval_accumulate on synthetic tables ---------------------------------------------------------------------------------------------
@pytest.mark.parametrize("n", [1, 33, 1025, "wrap"])
def test_accumulate_on_a_synthetic_table(n):
    import torch
    from gbnf_amd import native
    dev = _cuda()
    n = _wrap_n() if n == "wrap" else n
    ll = _table(n)
    lld, rho = _to(ll, dev), _to(RHO3, dev)
    for component in (0, 1):
        state = native.eval_state(dev)
        G = native.eval_accumulate(lld, rho, component, state, want_G=True)
        assert torch.equal(G, native.mixture_lse(lld, rho)), "G_out is not the recursion of gbnf_mixture_lse, bit for bit"
        _check_state_against_device_values(state.cpu().numpy(), ll, G.cpu().numpy(), RHO3, component)
    # without G_out: the same sums
    again = native.eval_state(dev)
    assert native.eval_accumulate(lld, rho, 1, again) is None
    assert again.cpu().numpy().tobytes() == state.cpu().numpy().tobytes()
    # a strided table (row stride n + 5)
    wide = torch.full((3, n + 5), float("nan"), dtype=torch.float32, device=dev)
    wide[:, :n] = lld
    strided = native.eval_state(dev)
    native.eval_accumulate(wide[:, :n], rho, 1, strided)
    assert strided.cpu().numpy().tobytes() == state.cpu().numpy().tobytes()


def test_accumulate_over_batches_adds_and_repeats():
    """Two calls (128 and 37 rows) give the sum of the two single-call states, batch means included; the sequence repeats to the byte;
    an empty call leaves the state alone."""
    import torch
    from gbnf_amd import native
    dev = _cuda()
    rho = _to(RHO3, dev)
    t1, t2 = _to(_table(128, seed=1), dev), _to(_table(37, seed=2), dev)

    def run(tables):
        state = native.eval_state(dev)
        for t in tables:
            native.eval_accumulate(t, rho, 2, state)
        return state.cpu().numpy()

    s1, s2, s12 = run([t1]), run([t2]), run([t1, t2])
    assert s12[0] == 165 and s12[1] == 2
    assert s12.tobytes() == (s1 + s2).tobytes()
    for k, src in ((6, 2), (7, 3), (8, 5)):                  # the sum of the batch means, not the mean over rows
        assert abs(s12[k] - (s1[src] / 128 + s2[src] / 37)) <= 2 * EPS * abs(s12[k]), k
        assert abs(s12[k] / 2 - s12[src] / 165) > 1e-3, "the two batches were meant to have different means"
    assert run([t1, t2]).tobytes() == s12.tobytes()
    # n == 0 through the library itself: GBNF_OK, nothing added, `batches` included
    state = _to(s12.copy(), dev)
    ws = torch.empty(4096, dtype=torch.float64, device=dev)
    p = lambda t: C.c_void_p(t.data_ptr())
    assert native.lib().gbnf_eval_accumulate(p(t1), 0, 3, 0, p(rho), 2, None, p(state), p(ws), ws.numel() * 8, None) == 0
    torch.cuda.synchronize()
    assert state.cpu().numpy().tobytes() == s12.tobytes()
    empty = torch.empty((3, 0), dtype=torch.float32, device=dev)
    assert native.eval_accumulate(empty, rho, 2, state, want_G=True).numel() == 0
    assert state.cpu().numpy().tobytes() == s12.tobytes()


def test_accumulate_counts_and_keeps_non_finite_rows():
    from gbnf_amd import native
    dev = _cuda()
    ll = _table(33, seed=3)
    ll[1, 5] = np.nan
    ll[:, 7] = -np.inf
    state = native.eval_state(dev)
    G = native.eval_accumulate(_to(ll, dev), _to(RHO3, dev), 1, state, want_G=True).cpu().numpy()
    s = state.cpu().numpy()
    want = eo.state_of([ll], RHO3, 1, G_of=[G])
    assert np.isnan(G[5]) and G[7] == -np.inf and np.isfinite(np.delete(G, [5, 7])).all()
    assert s[9] == 2 == want[9] and s[0] == 33 and s[1] == 1
    for k in (2, 3, 4, 5, 6, 7, 8):
        assert np.isnan(s[k]) and np.isnan(want[k]), k
    # only an infinite row: the sums are -inf where numpy's are, NaN where it forms inf - inf
    ll = _table(33, seed=3)
    ll[:, 7] = -np.inf
    state = native.eval_state(dev)
    G = native.eval_accumulate(_to(ll, dev), _to(RHO3, dev), 1, state, want_G=True).cpu().numpy()
    s, want = state.cpu().numpy(), eo.state_of([ll], RHO3, 1, G_of=[G])
    assert s[9] == 1 and s[2] == s[3] == s[5] == -np.inf == want[2] == want[3] == want[5] and np.isnan(s[4]) and np.isnan(want[4])


def test_accumulate_refusals_leave_the_state_alone():
    import torch
    from gbnf_amd import native
    dev = _cuda()
    L = native.lib()
    n = 33
    ll, rho = _to(_table(n), dev), _to(RHO3, dev)
    state = torch.full((16,), 7.0, dtype=torch.float64, device=dev)
    G = torch.full((n,), 7.0, dtype=torch.float32, device=dev)
    nb = C.c_int64()
    assert L.gbnf_eval_workspace_bytes(n, C.byref(nb)) == 0
    ws = torch.zeros(nb.value // 8, dtype=torch.float64, device=dev)
    p = lambda t: None if t is None else C.c_void_p(t.data_ptr())

    def acc(ll_=ll, stride=n, n_used=3, n_=n, rho_=rho, component=1, state_=state, ws_=ws, nbytes=nb.value):
        return L.gbnf_eval_accumulate(p(ll_), stride, n_used, n_, p(rho_), component, p(G), p(state_), p(ws_), nbytes, None)

    bad = {"null ll": dict(ll_=None), "null rho": dict(rho_=None), "null state": dict(state_=None), "null workspace": dict(ws_=None),
           "n < 0": dict(n_=-1), "n_used = 0": dict(n_used=0), "component = n_used": dict(component=3), "component < 0": dict(component=-1),
           "stride < n": dict(stride=n - 1), "short workspace": dict(nbytes=nb.value - 8)}
    for what, kw in bad.items():
        assert acc(**kw) == -1, f"{what}: accepted"
        assert L.gbnf_last_error(), what
    y = torch.zeros((n, 10), dtype=torch.float32, device=dev)
    for kw in (dict(Y=0), dict(Y=257), dict(c=3), dict(n_used=0), dict(nbytes=8)):
        a = dict(Y=10, c=0, n_used=3, nbytes=nb.value)
        a.update(kw)
        assert L.gbnf_eval_accumulate_class_loss(p(y), p(y), n, a["Y"], p(rho), a["n_used"], a["c"], p(state), p(ws), a["nbytes"], None) == -1, kw
    torch.cuda.synchronize()
    assert (state == 7.0).all() and (G == 7.0).all()
    assert acc() == 0
    torch.cuda.synchronize()
    assert float(state[0]) == 7.0 + n and float(state[1]) == 8.0 and torch.equal(G, native.mixture_lse(ll, rho))
    with pytest.raises(native.GbnfError):
        native.eval_accumulate(ll, rho, 1, state.float())
    with pytest.raises(native.GbnfError):
        native.eval_accumulate(ll, rho[:2], 1, state)


# ---- 2. eval_accumulate_class_loss ------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("Y", [1, 10, 256])
@pytest.mark.parametrize("n", [1, 33])
def test_class_loss(n, Y):
    """Entries 10 - 12 against the float64 yardstick, rows and batches untouched.  Both sides form CE_i with the same IEEE operations in
    the same order (the exponentials added in index order); what is left is the any-order bound on the sum over rows of v_i = w CE_i.
    Ties in y and in the logits pick the first of the largest."""
    from gbnf_amd import native
    dev = _cuda()
    rng = np.random.RandomState(10 * n + Y)
    logits = (rng.standard_normal((n, Y)) * 3.0).astype(np.float32)
    y = np.zeros((n, Y), dtype=np.float32)
    y[np.arange(n), rng.randint(0, Y, size=n)] = 1.0
    if n > 4 and Y > 2:
        y[2] = 0.0                                   # all tied: the first entry
        y[3] = 0.0
        y[3, [Y - 1, 1]] = 0.5                       # two tied maxima: the first of them
        logits[4, :] = logits[4, 0]                  # tied logits: prediction 0
    ce, label, pred = eo.cross_entropy(logits, y)
    if n > 4 and Y > 2:
        assert label[2] == 0 and label[3] == 1 and pred[4] == 0
    c = 1
    want = eo.class_state(logits, y, RHO3, 3, c)
    w = eo.weights(RHO3, 3)[c]
    bound = _sum_bound(w * ce)
    state = native.eval_state(dev)
    native.eval_accumulate_class_loss(_to(logits, dev), _to(y, dev), _to(RHO3, dev), c, state)
    s = state.cpu().numpy()
    print(f"n = {n}, Y = {Y}: state[10:13] {s[10:13]} vs {want} (bound {bound:.3e}, off by {np.abs(s[10:13] - want)})")
    assert abs(s[10] - want[0]) <= bound
    assert abs(s[11] - want[1]) <= bound / n
    assert s[12] == want[2]
    assert (s[:10] == 0).all() and (s[13:] == 0).all()
    if Y == 1:
        assert s[10] == 0.0 and s[12] == w * n
    # a second component adds its own share
    native.eval_accumulate_class_loss(_to(logits, dev), _to(y, dev), _to(RHO3, dev), 2, state)
    s2 = state.cpu().numpy()
    assert abs(s2[12] - (want[2] + eo.class_state(logits, y, RHO3, 3, 2)[2])) <= 4 * EPS * n


def test_class_loss_nan_logit_never_wins():
    from gbnf_amd import native
    dev = _cuda()
    logits = np.array([[0.5, np.nan, 0.25], [np.nan, np.nan, np.nan]], dtype=np.float32)
    y = np.array([[1, 0, 0], [1, 0, 0]], dtype=np.float32)
    state = native.eval_state(dev)
    native.eval_accumulate_class_loss(_to(logits, dev), _to(y, dev), _to(RHO3, dev), 0, state)
    s = state.cpu().numpy()
    assert np.isnan(s[10]) and np.isnan(s[11])
    assert s[12] == eo.weights(RHO3, 3)[0] * 2          # predictions 0 and 0 (a row of NaNs gives 0), labels 0 and 0


# ---- 3. gbnf_mixture_evaluate is its parts ----------------------------------------------------------------------------------------------
@pytest.mark.parametrize("kind,kw", [("glow", {}), ("realnvp", {"batch_norm": True})])
@pytest.mark.parametrize("n", [33, 512])
def test_mixture_evaluate_is_component_log_prob_then_accumulate(kind, kw, n):
    import torch
    from gbnf_amd import native, synth
    dev = _cuda()
    mix, _flows = native.mixture_from_specs(synth.synth_boosted_specs(kind, 3, 8, 32, 3, seed=3, **kw))
    x = _to(synth.synth_batch(n, 8, seed=4), dev)
    rho = _to(RHO3, dev)
    for component, n_used in ((2, 3), (0, 2)):
        one = native.eval_state(dev)
        G = mix.evaluate(x, component, rho, one, n_used=n_used, want_G=True)
        table = mix.eval_ll.clone()
        parts = native.eval_state(dev)
        ll = mix.component_log_prob(x, 0, n_used)
        G2 = native.eval_accumulate(ll, rho, component, parts, want_G=True)
        assert torch.equal(table, ll) and torch.equal(G, G2)
        assert one.cpu().numpy().tobytes() == parts.cpu().numpy().tobytes()
        assert float(one[0]) == n and float(one[9]) == 0 and torch.isfinite(one).all()
    with pytest.raises(native.GbnfError):
        mix.evaluate(x, 2, rho, one, n_used=2)
    with pytest.raises(native.GbnfError):
        mix.evaluate(x, 0, rho, one, n_used=4)


@pytest.mark.parametrize("name", ["g2_glow_native_d43_h32_c3", "g4_realnvp_d21_h105_c8"])
def test_mixture_evaluate_against_the_yardstick_on_the_fixture(name, golden_case):
    from gbnf_amd import native
    dev = _cuda()
    g = golden_case(name)
    mix, _flows = native.mixture_from_specs(g.specs)
    if g.base is not None:
        mix.set_base(*g.base)
    component = g.n_used - 1
    state = native.eval_state(dev)
    mix.evaluate(_to(g.x, dev), component, _to(g.rho, dev), state, n_used=g.n_used)
    s = state.cpu().numpy()
    want = eo.state_of([g.ll[:g.n_used]], g.rho, component)        # the yardstick fed with the reference's own ll
    n, bar = g.x.shape[0], LL_RTOL * float(np.abs(g.ll[:g.n_used]).max())
    assert s[0] == n == want[0] and s[1] == 1 and s[9] == 0
    for k in (2, 3, 4, 5):
        print(f"{name}: mean of state[{k}] {s[k] / n} vs {want[k] / n} (bar {bar:.3e})")
        assert abs(s[k] - want[k]) / n <= bar, k
    for k in (6, 7, 8):
        assert abs(s[k] - want[k]) <= bar, k


# ---- 4. BoostedFlow.evaluate against the reference's loop -----------------------------------------------------------------------------
def _reference_evaluate(model, loader, boosted=True):
    """density_experiment.py:544-594 with module forwards, as a caller writes it."""
    import torch
    G_nll, g_nll = [], []
    for (x, _) in loader:
        G_ll = None
        for c in range(model.component + 1):
            z_G, _, _, ldj_G, _ = model(x=x, components=c)
            ll = torch.sum(-0.5 * math.log(2 * math.pi) - 0.5 * z_G.pow(2), dim=-1) + ldj_G
            if c == 0:
                G_ll = ll
            else:
                rho_simplex = model.rho[0:(c + 1)] / torch.sum(model.rho[0:(c + 1)])
                last_ll = torch.log(1 - rho_simplex[c]) + G_ll
                next_ll = torch.log(rho_simplex[c]) + ll
                G_ll = torch.logsumexp(torch.cat([last_ll.view(-1, 1), next_ll.view(-1, 1)], dim=1), dim=1)
        G_nll.append(-1.0 * G_ll.detach())
        if model.component > 0 or model.all_trained:
            z_g, _, _, ldj_g, _ = model(x=x, components="c")
            g_nll.append(-1.0 * (torch.sum(-0.5 * math.log(2 * math.pi) - 0.5 * z_g.pow(2), dim=-1) + ldj_g).detach())
    batch_mean = torch.stack([t.mean() for t in G_nll], -1).mean().item()
    G_nll = torch.cat(G_nll, dim=0)
    losses = {"nll": G_nll.mean().item(), "nll_batch_mean": batch_mean}
    if model.component > 0 or model.all_trained:
        g_nll = torch.cat(g_nll, dim=0)
        losses["g_nll"] = g_nll.mean().item()
        losses["ratio"] = torch.mean(g_nll - G_nll).item()
    else:
        losses["g_nll"], losses["ratio"] = losses["nll"], 0.0
    return losses


def test_module_evaluate_against_the_reference_loop(golden_case):
    import torch
    from test_hip_module import _model_from_case
    dev = _cuda()
    g = golden_case("g2_glow_native_d43_h32_c3")
    m = _model_from_case(g, dev)
    x = torch.from_numpy(g.x).to(dev)
    x = torch.cat([x, x.flip(1)[:37]], dim=0)                 # 293 rows: batches of 128 / 128 / 37
    loader = [(x[0:128], None), (x[128:256], None), (x[256:293], None)]
    with torch.no_grad():
        bar = LL_RTOL * float(m.component_log_prob(x, n_used=3).abs().max())

    def check(out, ref):
        for key in ("nll", "g_nll", "ratio", "nll_batch_mean"):
            print(f"component {m.component}, all_trained {m.all_trained}: {key} {out[key]} vs {ref[key]} (bar {bar:.3e})")
            assert isinstance(out[key], float) and abs(out[key] - ref[key]) <= bar, key
        assert out["rows"] == 293 and out["batches"] == 3 and out["non_finite_rows"] == 0
        assert isinstance(out["expected_component_nll"], float) and math.isfinite(out["expected_component_nll"])

    m.component = 2
    m.train()
    out = m.evaluate(loader)
    assert not m.training, "evaluate puts the module in eval mode"
    assert set(out) == {"nll", "g_nll", "ratio", "expected_component_nll", "nll_batch_mean", "rows", "batches", "non_finite_rows"}
    with torch.no_grad():
        check(out, _reference_evaluate(m, loader))
        assert abs(out["nll"] + float(m.log_prob(x).double().mean())) <= bar
        # component 1 of 3, the reference's range: n_used = component + 1 (also the default before all_trained)
        m.component = 1
        check(m.evaluate(loader), _reference_evaluate(m, loader))
        explicit = m.evaluate(loader, n_used=2)
        check(explicit, _reference_evaluate(m, loader))
        # the first pass's component 0: g_nll = nll, ratio = 0.0
        m.component = 0
        out0 = m.evaluate(loader)
        check(out0, _reference_evaluate(m, loader))
        assert out0["g_nll"] == out0["nll"] and out0["ratio"] == 0.0
        # after the last boosting pass: component back at 0, all components by default; n_used = 1 is the reference's range
        m.all_trained = True
        check(m.evaluate(loader, n_used=1), _reference_evaluate(m, loader))
        full = m.evaluate(loader)
        assert abs(full["nll"] + float(m.log_prob(x, n_used=3).double().mean())) <= bar and full["ratio"] != 0.0
        m.component = 2
        with pytest.raises(ValueError):
            m.evaluate(loader, n_used=2)                      # g is not among the first two components
    with pytest.raises(ValueError):
        m.evaluate([])
    with pytest.raises(ValueError):
        m.evaluate(loader, n_used=4)


# ---- 5. the image one-call ----------------------------------------------------------------------------------------------------------------
IMAGE_CASES = {"3x32x32": ((3, 32, 32), dict(h=32, K=2, L=2)), "1x28x20": ((1, 28, 20), dict(h=32, K=2, L=2))}
RHO2 = np.array([1.0, 0.5], dtype=np.float32)


@functools.lru_cache(maxsize=None)
def _image_case(name):
    """(specs of 2 components, x, noise, float64 table) at 32 images: computed once, shared, left unchanged (n = 5: its first rows)."""
    import torch
    from gbnf_amd import synth
    from oracle import gbnf_oracle as oracle
    size, kw = IMAGE_CASES[name]
    specs = tuple(synth.synth_image_glow_spec(size, seed=s, **kw) for s in (1, 2))
    x, noise = synth.synth_image_batch(32, size, seed=104)
    ll64 = np.stack([np.asarray(oracle.image_component_forward(sp, x, noise, dtype=torch.float64)[4], dtype=np.float64) for sp in specs])
    return specs, x, noise, ll64


@pytest.mark.parametrize("name", sorted(IMAGE_CASES))
@pytest.mark.parametrize("n", [5, 32])
def test_image_evaluate_is_forwards_then_accumulate(name, n):
    import torch
    from gbnf_amd import native
    dev = _cuda()
    specs, x, noise, ll64 = _image_case(name)
    xd, nd, rho = _to(x[:n], dev), _to(noise[:n], dev), _to(RHO2, dev)
    # deterministic handles: to the byte
    flows = [native.NativeImageFlow(sp) for sp in specs]
    for f in flows:
        f.deterministic = True
    for component in (0, 1):
        one = native.eval_state(dev)
        table = native.NativeImageFlow.evaluate(flows, xd, nd, component, rho, one).clone()
        ll = torch.stack([f.forward(xd, nd, want_z=False)[2] for f in flows])
        parts = native.eval_state(dev)
        native.eval_accumulate(ll, rho, component, parts)
        assert torch.equal(table, ll)
        assert one.cpu().numpy().tobytes() == parts.cpu().numpy().tobytes()
    # default handles: within the bar of the float64 yardstick
    flows = [native.NativeImageFlow(sp) for sp in specs]
    state = native.eval_state(dev)
    table = native.NativeImageFlow.evaluate(flows, xd, nd, 1, rho, state)
    assert rel_err(table.cpu().numpy(), ll64[:, :n]) < LL_RTOL
    s, want = state.cpu().numpy(), eo.state_of([ll64[:, :n]], RHO2, 1)
    bar = LL_RTOL * float(np.abs(ll64[:, :n]).max())
    assert s[0] == n and s[1] == 1 and s[9] == 0 and (s[10:] == 0).all()
    for k in (2, 3, 4, 5):
        print(f"{name} n = {n}: mean of state[{k}] {s[k] / n} vs {want[k] / n} (bar {bar:.3e})")
        assert abs(s[k] - want[k]) / n <= bar, k
    for k in (6, 7, 8):
        assert abs(s[k] - want[k]) <= bar, k
    # one component: G = g = E
    single = native.eval_state(dev)
    native.NativeImageFlow.evaluate(flows[:1], xd, nd, 0, rho, single)
    s1 = single.cpu().numpy()
    assert s1[2] == s1[3] and s1[4] == 0.0 and abs(s1[5] - s1[2]) <= _sum_bound(ll64[0, :n]) + n * EPS * abs(s1[2])


def test_image_evaluate_refusals():
    """A short workspace, a mixed plain / conditioned handle list, a conditioned handle without a class head and the argument checks
    are refused before any launch: the state and the table keep their sentinels."""
    import torch
    import image_ycond_oracle as iyo
    from gbnf_amd import native, synth
    dev = _cuda()
    L = native.lib()
    size, kw = (1, 16, 16), dict(h=32, K=2, L=2)
    plain = [native.NativeImageFlow(synth.synth_image_glow_spec(size, seed=s, **kw)) for s in (1, 2)]
    cond = [native.NativeImageFlow(synth.synth_image_glow_spec(size, seed=s, y_classes=10, **kw)) for s in (1, 2)]
    headless_spec = synth.synth_image_glow_spec(size, seed=3, y_classes=10, **kw)
    for key in ("class_w", "class_b", "class_logs"):
        headless_spec["ycond"][key] = None
    other = native.NativeImageFlow(synth.synth_image_glow_spec((2, 8, 12), seed=1, h=16, K=1, L=1))
    n = 4
    x, noise = synth.synth_image_batch(n, size, seed=104)
    xd, nd, yd, rho = _to(x, dev), _to(noise, dev), _to(iyo.synth_y(n, 10), dev), _to(RHO2, dev)
    arr = lambda fs: (C.c_void_p * len(fs))(*[f.handle.value if f is not None else None for f in fs])
    nb = C.c_int64()
    assert L.gbnf_image_mixture_evaluate_workspace_bytes(arr(cond), 2, n, C.byref(nb)) == 0
    plain_nb = C.c_int64()
    assert L.gbnf_image_mixture_evaluate_workspace_bytes(arr(plain), 2, n, C.byref(plain_nb)) == 0
    assert 0 < plain_nb.value < nb.value and nb.value % 256 == 0
    ws = torch.empty(nb.value // 4, dtype=torch.float32, device=dev)
    state = torch.full((16,), 7.0, dtype=torch.float64, device=dev)
    table = torch.full((2, n), 7.0, dtype=torch.float32, device=dev)
    p = lambda t: None if t is None else C.c_void_p(t.data_ptr())

    def call(flows_=arr(plain), n_used=2, component=1, x_=xd, y_=None, n_=n, rho_=rho, table_=table, state_=state, ws_=ws, nbytes=nb.value):
        if y_ is not None:
            return L.gbnf_image_mixture_evaluate_y(flows_, n_used, component, p(x_), p(nd), p(y_), n_, p(rho_), p(table_), None, p(state_),
                                                   p(ws_), nbytes, None)
        return L.gbnf_image_mixture_evaluate(flows_, n_used, component, p(x_), p(nd), n_, p(rho_), p(table_), None, p(state_), p(ws_),
                                             nbytes, None)

    bad = {"null flows": dict(flows_=None), "null x": dict(x_=None), "null rho": dict(rho_=None), "null table": dict(table_=None),
           "null state": dict(state_=None), "null workspace": dict(ws_=None), "null entry": dict(flows_=arr([plain[0], None])),
           "n = 0": dict(n_=0), "n_used = 0": dict(n_used=0), "component = n_used": dict(component=2), "component < 0": dict(component=-1),
           "shapes differ": dict(flows_=arr([plain[0], other])), "short workspace": dict(nbytes=plain_nb.value - 256),
           "mixed plain / conditioned": dict(flows_=arr([plain[0], cond[1]])), "conditioned without y": dict(flows_=arr(cond)),
           "y with plain handles": dict(y_=yd), "y, mixed": dict(flows_=arr([cond[0], plain[1]]), y_=yd),
           "y, short workspace": dict(flows_=arr(cond), y_=yd, nbytes=nb.value - 256)}
    for what, kw_ in bad.items():
        assert call(**kw_) == -1, f"{what}: accepted"
        assert L.gbnf_last_error(), what
    headless = native.NativeImageFlow(headless_spec)
    assert headless.y_classes == 10 and not headless.has_class_head
    assert call(flows_=arr([cond[0], headless]), y_=yd) == -1 and b"class head" in L.gbnf_last_error()
    torch.cuda.synchronize()
    assert (state == 7.0).all() and (table == 7.0).all()
    assert call() == 0 and call(flows_=arr(cond), y_=yd) == 0
    torch.cuda.synchronize()
    assert float(state[0]) == 7.0 + 2 * n and float(state[1]) == 9.0 and float(state[10]) != 7.0 and torch.isfinite(table).all()


# ---- 6. BoostedImageFlow.evaluate against the eager replay ----------------------------------------------------------------------------
def _image_module(dev):
    import torch
    import test_image_boost_host as host
    from gbnf_amd import BoostedFlow, image_glow
    size, kw = IMAGE_CASES["1x28x20"]
    torch.manual_seed(0)
    m = BoostedFlow(host.image_args(size, kw["h"], kw["K"], kw["L"], dev, C_=2))
    for c, sp in enumerate(_image_case("1x28x20")[0]):
        image_glow.load_image_spec(m.flows[c], sp)
    return m


def test_image_module_evaluate_against_the_eager_replay():
    import torch
    from gbnf_amd import native
    dev = _cuda()
    m = _image_module(dev)
    m.component = 1
    x = _image_case("1x28x20")[1]
    batches = [_to(x[0:5], dev), _to(x[5:10], dev), _to(x[10:13], dev)]
    loader = [(b, None) for b in batches]
    m.train()
    out = m.evaluate(loader, noise_generator=torch.Generator(device=dev).manual_seed(7))
    assert not m.training
    assert set(out) == {"bpd", "g_bpd", "expected_component_bpd", "loss", "rows", "batches", "non_finite_rows"}
    # the replay: component_log_prob + the recursion per batch, with the same noise draws
    g = torch.Generator(device=dev).manual_seed(7)
    per_dim = 1.0 / (math.log(2.0) * 28 * 20)
    G, ll1, E, batch_loss, worst = [], [], [], [], 0.0
    w = eo.weights(m.rho.cpu().numpy(), 2)
    for b in batches:
        noise = torch.rand(b.shape, generator=g, device=dev)
        ll = m.component_log_prob(b, 2, noise)                       # (n, 2)
        G.append(native.mixture_lse(ll.t().contiguous(), m.rho).double().cpu().numpy())
        ll = ll.double().cpu().numpy()
        worst = max(worst, float(np.abs(ll).max()))
        ll1.append(ll[:, 1])
        E.append(ll @ w)
        batch_loss.append(-float(np.mean(ll @ w)) * per_dim)
    bar = LL_RTOL * worst * per_dim
    want = {"bpd": -float(np.mean(np.concatenate(G))) * per_dim, "g_bpd": -float(np.mean(np.concatenate(ll1))) * per_dim,
            "expected_component_bpd": -float(np.mean(np.concatenate(E))) * per_dim, "loss": float(np.mean(batch_loss))}
    for key, v in want.items():
        print(f"{key}: {out[key]} vs {v} (bar {bar:.3e})")
        assert isinstance(out[key], float) and abs(out[key] - v) <= bar, key
    assert out["rows"] == 13 and out["batches"] == 3 and out["non_finite_rows"] == 0
    assert abs(out["loss"] - out["expected_component_bpd"]) > 0.0, "the ragged batch was meant to tell the two means apart"
    # defaults of n_used: component + 1 before all_trained, all components after; g among them
    m.component = 0
    first = m.evaluate(loader, noise_generator=torch.Generator(device=dev).manual_seed(7))
    assert first["bpd"] == first["g_bpd"] == first["expected_component_bpd"]
    m.all_trained = True
    full = m.evaluate(loader, noise_generator=torch.Generator(device=dev).manual_seed(7))
    assert abs(full["bpd"] - want["bpd"]) <= bar and abs(full["g_bpd"] - first["g_bpd"]) <= bar
    m.component = 1
    with pytest.raises(ValueError):
        m.evaluate(loader, n_used=1)
    with pytest.raises(ValueError):
        m.evaluate([])
    with pytest.raises(ValueError, match="class-conditional"):
        m.evaluate(loader, labels=True)                              # a model without conditioning


def test_image_module_evaluate_with_labels():
    """labels=True on a class-conditional model of 10 classes: the class loss, the accuracy and the two losses against float64 values
    formed from component_forward(..., y_onehot=) logits and component_log_prob(..., y_onehot=) of the same batches and noise."""
    import torch
    import image_ycond_oracle as iyo
    from gbnf_amd import synth
    from test_hip_image_class_table import _module
    dev = _cuda()
    m, data = _module(dev)
    m.image_eval_deterministic = True
    m.component = 2
    size, Y = tuple(m.flows[0].input_size), int(m.flows[0].y_classes)
    assert Y == 10
    xs = [synth.synth_image_batch(k, size, seed=s)[0] for k, s in ((4, 104), (3, 105))]
    ys = [iyo.synth_y(k, Y, seed=s) for k, s in ((4, 4), (3, 5))]
    loader = [(_to(x, dev), _to(y, dev)) for x, y in zip(xs, ys)]
    with pytest.raises(NotImplementedError, match="labels=True"):
        m.evaluate(loader)
    y_weight = 0.5
    out = m.evaluate(loader, noise_generator=torch.Generator(device=dev).manual_seed(7), labels=True, y_weight=y_weight)
    assert set(out) == {"bpd", "g_bpd", "expected_component_bpd", "loss", "loss_classes", "accuracy", "total_loss", "rows", "batches",
                        "non_finite_rows"}
    g = torch.Generator(device=dev).manual_seed(7)
    rho = m.rho.cpu().numpy()
    w = eo.weights(rho, 3)
    per_dim = 1.0 / (math.log(2.0) * float(np.prod(size)))
    G, ce_rows, hit_rows, batch_loss, worst, ce_max = [], [], [], [], 0.0, 0.0
    with torch.no_grad():
        for xb, yb in loader:
            noise = torch.rand(xb.shape, generator=g, device=dev)
            ll = m.component_log_prob(xb, 3, noise, y_onehot=yb).double().cpu().numpy()         # (n, 3)
            worst = max(worst, float(np.abs(ll).max()))
            G.append(eo.mixture_G(ll.T, rho))
            ce_b, hit_b = np.zeros(xb.shape[0]), np.zeros(xb.shape[0])
            for c in range(3):
                logits = m.component_forward(xb, c, noise, y_onehot=yb)[4].cpu().numpy()
                ce, label, pred = eo.cross_entropy(logits, yb.cpu().numpy())
                ce_b += w[c] * ce
                hit_b += w[c] * (label == pred)
                ce_max = max(ce_max, float(np.abs(ce).max()))
            ce_rows.append(ce_b)
            hit_rows.append(hit_b)
            batch_loss.append(-float(np.mean(ll @ w)) * per_dim + y_weight * float(np.mean(ce_b)))
    bar = LL_RTOL * worst * per_dim
    # the class terms come from the same float32 logits on both sides: what differs is double rounding over 7 rows x 3 components
    ce_bar = 64 * EPS * ce_max
    want = {"bpd": -float(np.mean(np.concatenate(G))) * per_dim, "loss_classes": float(np.mean(np.concatenate(ce_rows))),
            "accuracy": float(np.mean(np.concatenate(hit_rows))), "loss": float(np.mean(batch_loss))}
    want["total_loss"] = want["bpd"] + y_weight * want["loss_classes"]
    bars = {"bpd": bar, "loss_classes": ce_bar, "accuracy": 64 * EPS, "loss": bar + y_weight * ce_bar, "total_loss": bar + y_weight * ce_bar}
    for key, v in want.items():
        print(f"{key}: {out[key]} vs {v} (bar {bars[key]:.3e})")
        assert isinstance(out[key], float) and abs(out[key] - v) <= bars[key], key
    assert out["rows"] == 7 and out["batches"] == 2 and out["non_finite_rows"] == 0 and 0.0 <= out["accuracy"] <= 1.0
    # y_weight defaults to args.y_weight, else 0.01
    default = m.evaluate(loader, noise_generator=torch.Generator(device=dev).manual_seed(7), labels=True)
    assert abs(default["total_loss"] - (default["bpd"] + 0.01 * default["loss_classes"])) <= 4 * EPS * abs(default["total_loss"])
    m.args.y_weight = 0.25
    again = m.evaluate(loader, noise_generator=torch.Generator(device=dev).manual_seed(7), labels=True)
    assert abs(again["total_loss"] - (again["bpd"] + 0.25 * again["loss_classes"])) <= 4 * EPS * abs(again["total_loss"])
    assert again["bpd"] == default["bpd"]                            # deterministic handles: the pass repeats to the bit
