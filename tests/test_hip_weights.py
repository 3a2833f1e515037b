"""GPU: all mixture weights at once -- gbnf_weights_em / gbnf_weights_to_rho (csrc/gbnf_weights.hip), BoostedFlow.fit_weights and
BoostedImageFlow.fit_weights -- against the float64 yardstick of tests/weights_oracle.py on the same float32 table.

Bounds.  Both sides iterate in float64; they differ in the order of their sums and in the last bits of exp / log.
tests/test_weights_host.py measures what a change of order and of format does to the yardstick's own final weights after the 100
updates used here: below 1e-11 relative over all cases.  The bar for the device is a hundred times that, 1e-9 relative for
w_c > 1e-12; L_0 and the final L, means of N values of one evaluation, are held to 1e-12 relative."""
import functools
import math

import numpy as np
import pytest

import weights_cases as wc
import weights_oracle as wo

pytestmark = pytest.mark.gpu

W_RTOL = 1e-9
L_RTOL = 1e-12
LL_RTOL = 1e-5            # the bar of tests/test_hip_eval.py for nll against float64: 1e-5 max|ll|


def _cuda():
    import torch
    return torch.device("cuda:0")


def _to(a, dev):
    import torch
    return torch.from_numpy(np.array(a, order="C")).to(dev)          # (a copy: the shared tables are read-only)


def _em(ll, rho, max_iters, tol, stride=None):
    """weights_em on the device -> the state as numpy.  ``stride``: the table sits in a wider one whose gap holds poison."""
    import torch
    from gbnf_amd import native
    dev = _cuda()
    C_, n = ll.shape
    if stride is None:
        t = _to(ll, dev)
    else:
        wide = torch.full((C_, stride), float("nan"), dtype=torch.float32, device=dev)
        wide[:, :n] = _to(ll, dev)
        t = wide[:, :n]
    s = native.weights_em(t, _to(np.asarray(rho, dtype=np.float32), dev), max_iters, tol)
    return s.cpu().numpy()


def _check_fixed(ll, rho, got, want):
    C_ = ll.shape[0]
    w, ww = got[8:8 + C_], want[8:8 + C_]
    big = ww > 1e-12
    rel = float((np.abs(w[big] - ww[big]) / ww[big]).max())
    print(f"C = {C_}, n = {ll.shape[1]}: weights off by {rel:.3e} relative; L_0 {got[4]!r} vs {want[4]!r}; L {got[5]!r} vs {want[5]!r}")
    assert (got[:4] == want[:4]).all() and got[7] == want[7] == 0
    assert rel <= W_RTOL and (np.abs(w[~big]) <= 1e-12).all()
    assert abs(got[4] - want[4]) <= L_RTOL * abs(want[4]) and abs(got[5] - want[5]) <= L_RTOL * abs(want[5])
    assert abs(got[6] - want[6]) <= 2 * L_RTOL * abs(want[5])
    assert (got[8 + C_:] == 0).all(), "the state beyond the weights is not written"


# ---- 1. a fixed number of updates ---------------------------------------------------------------------------------------------------------
@functools.lru_cache(maxsize=None)
def _fixed_reference(C_, n):
    """(table, rho, the yardstick's state after FIXED_UPDATES updates): computed once, shared, left unchanged."""
    ll = wc.shape_table(C_, n)
    rho = np.arange(1, C_ + 1, dtype=np.float32)          # an uneven start
    return ll, rho, wo.em(ll, rho, wc.FIXED_UPDATES, 0.0)


@pytest.mark.parametrize("C_,n", [(3, 1), (3, 63), (3, 64), (3, 65), (3, 257), (3, 4096), (5, 262145),
                                  (1, 257), (2, 257), (5, 257), (33, 257), (64, 257)])
def test_fixed_iteration_count(C_, n):
    ll, rho, want = _fixed_reference(C_, n)
    assert want[0] == wc.FIXED_UPDATES and want[1] == 0
    _check_fixed(ll, rho, _em(ll, rho, wc.FIXED_UPDATES, 0.0), want)


def test_fixed_iteration_count_on_a_strided_table():
    ll, rho, want = _fixed_reference(5, 257)
    _check_fixed(ll, rho, _em(ll, rho, wc.FIXED_UPDATES, 0.0, stride=257 + 37), want)


# ---- 2. stopping ----------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("name", wc.CONVERGING)
def test_stops_where_the_yardstick_stops_and_later_launches_do_nothing(name):
    C_, _, _, _, _, evaluations = wc.CASES[name]
    ll, rho = wc.table(name), wc.uniform_rho(C_)
    got = _em(ll, rho, wc.MAX_ITERS, wc.TOL)
    print(f"{name}: {int(got[0]) + 1} evaluations on the device, {evaluations} in the yardstick; last step {got[6]:.3e}")
    assert got[1] == 1 and got[7] == 0 and abs(int(got[0]) + 1 - evaluations) <= 1 and 0 <= got[6] <= wc.TOL
    iters = int(got[0])
    want = wo.em(ll, rho, iters, 0.0)                       # the yardstick after the same number of updates
    w, ww = got[8:8 + C_], want[8:8 + C_]
    assert (np.abs(w - ww) / ww).max() <= W_RTOL and abs(got[5] - want[5]) <= L_RTOL * abs(want[5])
    # the gate: whether the stopping evaluation is the last one enqueued or 50 more launches follow it, the state has the same bits
    exact = _em(ll, rho, iters, wc.TOL)
    longer = _em(ll, rho, iters + 50, wc.TOL)
    assert exact.tobytes() == longer.tobytes() == got.tobytes()


def test_a_case_that_does_not_converge_reports_it():
    name = wc.NOT_CONVERGING
    C_ = wc.CASES[name][0]
    ll, rho = wc.table(name), wc.uniform_rho(C_)
    got = _em(ll, rho, wc.MAX_ITERS, wc.TOL)
    want = wo.em(ll, rho, wc.MAX_ITERS, wc.TOL)
    assert want[1] == 0 and got[0] == wc.MAX_ITERS and got[1] == 0 and got[7] == 0 and got[6] > wc.TOL
    assert got[5] >= got[4] and abs(got[5] - want[5]) <= 1e-9 * abs(want[5])
    zero = _em(ll, rho, 0, wc.TOL)                          # max_iters = 0: one evaluation at the starting weights
    assert zero[0] == 0 and zero[1] == 0 and zero[4] == zero[5] == got[4] and zero[6] == 0 and (zero[8:8 + C_] == 1.0 / C_).all()


# ---- 3. edges -------------------------------------------------------------------------------------------------------------------------------
def test_minus_infinity_entries_and_excluded_rows():
    ll = np.array(wc.table("c3_n4096")[:, :300])
    ll[1, 3] = ll[0, 70] = ll[2, 299] = -np.inf             # single -inf entries: legal, r = 0
    ll[:, 5] = -np.inf                                       # -inf under every component
    ll[0, 130] = np.nan
    ll[2, 257] = np.inf
    rho = wc.uniform_rho(3)
    got, want = _em(ll, rho, 30, 0.0), wo.em(ll, rho, 30, 0.0)
    assert got[2] == 297 and got[3] == 3 and np.isfinite(got).all()
    _check_fixed(ll, rho, got, want)


def test_a_component_without_support_ends_at_weight_zero():
    ll = np.array(wc.table("c3_n4096")[:, :300])
    ll[1, :] = -np.inf
    rho = wc.uniform_rho(3)
    got, want = _em(ll, rho, 30, 0.0), wo.em(ll, rho, 30, 0.0)
    assert got[9] == 0.0 and want[9] == 0.0 and not np.isnan(got).any() and got[3] == 0
    _check_fixed(ll, rho, got, want)
    again = _em(ll, got[8:11], 5, 0.0)                       # started AT weight 0 (log w = -inf): a fixed point, no NaN
    assert again[9] == 0.0 and not np.isnan(again).any() and again[5] >= got[5] - L_RTOL * abs(got[5])


def test_far_negative_log_likelihoods_need_the_subtracted_maximum():
    ll = np.array(wc.table("c3_n4096")[:, :300]) - np.float32(1e4)
    rho = wc.uniform_rho(3)
    got, want = _em(ll, rho, 30, 0.0), wo.em(ll, rho, 30, 0.0)
    assert np.isfinite(got).all() and got[5] < -9e3
    _check_fixed(ll, rho, got, want)


def test_bad_starts_write_the_flag_and_leave_rho_alone():
    import torch
    from gbnf_amd import native
    dev = _cuda()
    ll = np.array(wc.table("c3_n4096")[:, :300])
    nan_rows = np.full((3, 4), np.nan, dtype=np.float32)
    for table, rho in ((ll[:, :0], [1, 1, 1]), (nan_rows, [1, 1, 1]), (ll, [0, 0, 0]), (ll, [1, -1, 1]), (ll, [1, float("inf"), 1])):
        rho_d = _to(np.asarray(rho, dtype=np.float32), dev)
        state = native.weights_em(_to(table, dev), rho_d, 10, 1e-9)
        s = state.cpu().numpy()
        want = wo.em(table, rho, 10, 1e-9)
        assert s[7] == 1 and s[0] == 0 and s[1] == 0 and s[2] == want[2] and s[3] == want[3], (rho, s[:8])
        target = _to(np.array([3.0, 2.0, 1.0, 0.5], dtype=np.float32), dev)
        native.weights_to_rho(state, target, n_components=3)
        assert target.tolist() == [3.0, 2.0, 1.0, 0.5] and float(state[7]) == 1.0


def test_one_component_has_weight_one():
    ll = wc.table("c3_n4096")[1:2, :300]
    got = _em(ll, [0.37], 5, 0.0)
    assert got[8] == 1.0 and got[0] == 5 and got[4] == got[5]
    assert abs(got[5] - float(ll.astype(np.float64).mean())) <= L_RTOL * abs(got[5])


# ---- 4. repeats ------------------------------------------------------------------------------------------------------------------------------
def test_two_identical_calls_give_the_same_bits():
    import torch
    from gbnf_amd import native
    dev = _cuda()
    ll = _to(wc.table("c5_n70001"), dev)
    out = []
    for _ in range(2):
        rho = _to(np.array([1.0, 0.5, 0.25, 0.125, 0.0625, 9.0], dtype=np.float32), dev)
        state = native.weights_em(ll, rho[:5], 40, 0.0, state=torch.full((wo.STATE_DOUBLES,), 7.0, dtype=torch.float64, device=dev))
        native.weights_to_rho(state, rho, n_components=5)
        out.append((state.cpu().numpy().tobytes(), rho.cpu().numpy().tobytes()))
    assert out[0] == out[1]


# ---- 5. the weights back into rho -----------------------------------------------------------------------------------------------------------
def test_weights_to_rho():
    import torch
    from gbnf_amd import native
    dev = _cuda()
    ll = _to(wc.table("c3_n4096"), dev)
    start = np.array([1.0, 0.5, 0.25, 0.125, 7.0], dtype=np.float32)
    rho = _to(start, dev)
    state = native.weights_em(ll, rho[:3].contiguous(), 20, 0.0)
    before = state.cpu().numpy()
    w = before[8:11]
    native.weights_to_rho(state, rho, n_components=3)
    got = rho.cpu().numpy()
    want, flags = wo.to_rho(before, start, 3)
    assert (got == want).all() and float(state[7]) == flags == 0
    assert (got[3:] == start[3:]).all(), "entries beyond C are untouched"
    assert np.abs(got[:3].astype(np.float64) / got[:3].astype(np.float64).sum() - w).max() <= 4 * 2.0 ** -24
    assert abs(got[:3].astype(np.float64).sum() - 1.75) <= 3 * 2.0 ** -24 * 1.75, "the total is kept"
    # a case built to meet the lower bound: three components of which two have no support to speak of
    far = np.array(wc.table("c3_n4096")[:, :500])
    far[1:, :] -= np.float32(40.0)
    rho = _to(np.ones(3, dtype=np.float32), dev)
    state = native.weights_em(_to(far, dev), rho, 20, 0.0)
    native.weights_to_rho(state, rho)
    got = rho.cpu().numpy()
    assert (got[1:] == np.float32(0.01)).all() and abs(got[0] - 3.0) <= 1e-6 and float(state[7]) == 4.0      # 2 * (two clamped entries)
    # a second call adds its own count: the word reads bad_start + 2 * clamped
    native.weights_to_rho(state, rho)
    assert float(state[7]) == 8.0


# ---- 6. the modules ---------------------------------------------------------------------------------------------------------------------------
def _tabular_model(dev):
    import argparse
    import torch
    from gbnf_amd import BoostedFlow, synth
    d, h, K, C_ = 2, 8, 1, 3
    args = argparse.Namespace(
        num_flows=K, z_size=d, density_evaluation=True, device=dev, cuda=True, component_type="glow", num_components=C_,
        rho_init="decreasing", learn_top=False, y_classes=0, y_condition=False, sample_size=4, input_size=[d], h_size=h, num_blocks=1,
        actnorm_scale=1.0, flow_permutation="shuffle", flow_coupling="affine", LU_decomposed=False, num_dequant_blocks=0,
        coupling_network="tanh", coupling_network_depth=1, batch_norm=False)
    m = BoostedFlow(args)
    specs = synth.synth_boosted_specs("glow", C_, d, h, K, seed=7)
    # component 1 fits standard-normal rows worse than the others; it keeps a weight above the floor of rho's range
    specs[1]["steps"][0]["an_bias"] = specs[1]["steps"][0]["an_bias"] + np.float32(1.0)
    for c, sp in enumerate(specs):
        m.load_spec(c, sp)
    m.all_trained = True
    return m.eval()


def _check_module(m, loader, fit, evaluate_nll, bad, bar):
    import torch
    rho0 = m.rho.detach().clone()
    w0 = (rho0 / rho0.sum()).cpu().numpy()
    version = m.rho._version
    m.train()
    out = fit()
    assert not m.training, "fit_weights puts the module in eval mode"
    assert set(out) == {"nll_before", "nll_after", "iters", "converged", "rows", "excluded", "weights", "clamped"}
    print({k: v for k, v in out.items()})
    assert out["nll_after"] <= out["nll_before"] and out["excluded"] == 0 and out["iters"] >= 1
    assert m.rho._version > version and not torch.equal(m.rho, rho0)
    assert out["converged"] and out["clamped"] == 0, "the case was built to converge inside rho's range"
    assert abs(float(m.rho.sum()) - float(rho0.sum())) <= 1e-6 * float(rho0.sum()), "the total is kept"
    after = evaluate_nll()
    print(f"nll_after {out['nll_after']} vs evaluate under the written rho {after} (bar {bar:.3e})")
    assert abs(out["nll_after"] - after) <= bar
    assert out["weights"][bad] < w0[bad], "the badly fitting component loses weight"
    second = fit()
    assert second["iters"] <= 1 and abs(second["nll_before"] - after) <= bar
    return out


def test_tabular_module_fit_weights():
    import torch
    from gbnf_amd import synth
    dev = _cuda()
    m = _tabular_model(dev)
    x = _to(synth.synth_batch(700, 2, seed=3), dev)
    loader = [(x[0:256], None), (x[256:512], None), (x[512:700], None)]
    with torch.no_grad():
        bar = LL_RTOL * float(m.component_log_prob(x, n_used=3).abs().max())
    out = _check_module(m, loader, lambda: m.fit_weights(loader), lambda: m.evaluate(loader)["nll"], 1, bar)
    assert out["rows"] == 700
    # a loader with a dataset sizes the table once; write=False leaves rho alone
    ds = torch.utils.data.TensorDataset(x.cpu(), torch.zeros(700))
    rho = m.rho.detach().clone()
    dry = m.fit_weights(torch.utils.data.DataLoader(ds, batch_size=256), write=False, max_iters=3, tol=0.0)
    assert dry["rows"] == 700 and dry["iters"] == 3 and dry["clamped"] == 0 and torch.equal(m.rho, rho)
    with pytest.raises(ValueError):
        m.fit_weights([])
    with pytest.raises(ValueError):
        m.fit_weights(loader, n_used=4)


def test_image_module_fit_weights():
    import torch
    import test_image_boost_host as host
    from gbnf_amd import BoostedFlow, image_glow, synth
    dev = _cuda()
    size, kw = (1, 16, 16), dict(h=32, K=2, L=2)
    torch.manual_seed(0)
    m = BoostedFlow(host.image_args(size, kw["h"], kw["K"], kw["L"], dev, C_=2))
    for c in range(2):
        image_glow.load_image_spec(m.flows[c], synth.synth_image_glow_spec(size, seed=1 + c, **kw))
    m.all_trained = True
    x, _ = synth.synth_image_batch(13, size, seed=104)
    batches = [_to(x[0:5], dev), _to(x[5:10], dev), _to(x[10:13], dev)]
    loader = [(b, None) for b in batches]
    gen = lambda: torch.Generator(device=dev).manual_seed(7)
    with torch.no_grad():
        ll = m.component_log_prob(_to(x, dev), 2, torch.rand(x.shape, generator=gen(), device=dev))
    # the components differ by several nats per image, so a row belongs to one of them: the one that wins fewer rows loses weight
    worse = int(torch.bincount(ll.argmax(dim=1), minlength=2).argmin())
    with torch.no_grad():
        m.rho.copy_(torch.tensor([1.0, 1.0], device=dev))
    bar = LL_RTOL * float(ll.abs().max())
    per_dim = 1.0 / (math.log(2.0) * 16 * 16)
    out = _check_module(m, loader, lambda: m.fit_weights(loader, noise_generator=gen()),
                        lambda: m.evaluate(loader, noise_generator=gen())["bpd"] / per_dim, worse, bar)
    assert out["rows"] == 13
    with pytest.raises(ValueError, match="class-conditional"):
        m.fit_weights(loader, labels=True)
