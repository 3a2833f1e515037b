"""The on-data numerics guard of the z -> x direction (include/gbnf.h, gbnf_numerics_status / gbnf_flow_numerics_inverse,
gbnf_image_flow_inverse_check_counts): a DEFAULT handle re-checks its f16x3 choice on the caller's z on a schedule of its own, and a
failed check re-evaluates that very call on the safe arithmetic and demotes the handle for both directions."""
import numpy as np
import pytest

pytestmark = pytest.mark.gpu

X_BAR = 2e-5          # the direction's bar for x (tests/test_hip_inverse.py)
TOL = 2.5e-6          # check_tolerance_e9 = 2500: a quarter of the 1e-5 log|det| bar


@pytest.fixture(scope="module")
def dev():
    import torch
    assert torch.cuda.is_available()
    return torch.device("cuda:0")


@pytest.fixture()
def tuning():
    from gbnf_amd import native
    keys = ("force_nt", "wg_pairs", "repair", "check_every", "check_tolerance_e9")
    saved = {k: native.tuning_get(k) for k in keys}
    yield native
    for k, v in saved.items():
        native.tuning_set(k, v)


def _z(n, d, seed, dev):
    import torch
    return torch.from_numpy(np.random.RandomState(seed).standard_normal((n, d)).astype(np.float32)).to(dev)


def _row_dev(x, ref):
    """per row: max|x - ref| / max(1, max|ref|) over the row's features (tests/test_hip_inverse.py)"""
    return np.abs(x - ref).max(axis=1) / np.maximum(1.0, np.abs(ref).max(axis=1))


def test_inverse_guard_checks_the_first_launch_and_every_nth_on_its_own_schedule(dev, tuning):
    import torch
    from gbnf_amd import native, synth
    spec = synth.synth_glow_spec(43, 215, 5, seed=1)
    z = _z(1024, 43, 11, dev)
    flow = native.NativeFlow(spec, math="default")
    assert native.MATH_NAME[flow.info().math_mode] == "f16x3"
    st = flow.numerics("inverse")
    assert (st.checks, st.demoted) == (0, 0) and abs(st.tolerance - TOL) < 1e-9
    x0, l0 = flow.inverse(z)                                    # launch 0: checked
    torch.cuda.synchronize()
    st = flow.numerics("inverse")
    print(f"INVGUARD schedule worst {st.worst_rel_err:.3e} tolerance {st.tolerance:.3e}")
    assert st.checks == 1 and st.demoted == 0 and 0.0 <= st.worst_rel_err <= st.tolerance
    assert flow.numerics().checks == 0
    for _ in range(5):                                          # check_every = 256: launches 1..5 are not checked
        x1, l1 = flow.inverse(z)
    torch.cuda.synchronize()
    assert flow.numerics("inverse").checks == 1 and flow.numerics().checks == 0
    assert torch.equal(x1, x0) and torch.equal(l1, l0)          # checked and unchecked calls: the same bits
    tuning.tuning_set("check_every", 2)
    for _ in range(6):                                          # launches 6..11: the even ones are checked
        x2, l2 = flow.inverse(z)
    torch.cuda.synchronize()
    assert flow.numerics("inverse").checks == 4 and flow.numerics().checks == 0
    assert torch.equal(x2, x0) and torch.equal(l2, l0)
    flow.forward(z)                                             # the forward direction keeps its own count
    torch.cuda.synchronize()
    assert flow.numerics().checks == 1 and flow.numerics("forward").checks == 1
    assert flow.numerics("inverse").checks == 4 and flow.numerics().demoted == 0
    # an explicit f16x3 handle keeps the caller's choice: no guard in either direction
    f = native.NativeFlow(spec, math="f16x3")
    xf, lf = f.inverse(z)
    torch.cuda.synchronize()
    assert f.numerics("inverse").checks == 0 and f.numerics().checks == 0
    assert torch.equal(xf, x0) and torch.equal(lf, l0)          # a passed check changes nothing
    with pytest.raises(ValueError):
        flow.numerics("sideways")


def _fail_spec(kind):
    from gbnf_amd import synth
    if kind == "glow":
        return synth.synth_glow_spec(43, 64, 3, seed=5)
    return synth.synth_realnvp_spec(21, 105, 3, batch_norm=True, seed=7)


@pytest.mark.parametrize("n", [77, 300])
@pytest.mark.parametrize("kind", ["glow", "realnvp"])
def test_failed_inverse_check_repairs_the_call_and_demotes_the_handle(kind, n, dev, tuning):
    """tolerance 0 => the first z -> x check fails: the checked call comes back as the bf16x6 handle's x and log|det| for ALL rows
    (n = 300: beyond the 256 the check looked at), the verdict is the handle's (both directions), later calls run bf16x6."""
    import torch
    from gbnf_amd import native
    spec = _fail_spec(kind)
    z = _z(n, spec["d"], 21, dev)
    safe = native.NativeFlow(spec, math="bf16x6")
    want_x, want_l = safe.inverse(z)
    fast = native.NativeFlow(spec, math="f16x3")
    assert not torch.equal(fast.inverse(z)[0], want_x)          # the two modes do differ in the last bits
    tuning.tuning_set("check_tolerance_e9", 0)
    flow = native.NativeFlow(spec, math="default")
    assert flow.numerics("inverse").math_mode == native.MATH["f16x3"]
    x, l = flow.inverse(z)                                      # launch 0: checked, fails, re-evaluated on the device
    torch.cuda.synchronize()
    st = flow.numerics("inverse")
    assert st.checks == 1 and st.demoted == 1 and st.math_mode == native.MATH["bf16x6"]
    assert flow.numerics().demoted == 1 and flow.numerics().checks == 0
    assert torch.equal(x, want_x) and torch.equal(l, want_l)
    tuning.tuning_set("check_tolerance_e9", 2500)
    x2, l2 = flow.inverse(z)                                    # the host saw the flag: plain bf16x6 launches, both directions
    assert torch.equal(x2, want_x) and torch.equal(l2, want_l)
    got = flow.forward(z, want_ll=True)
    ref = safe.forward(z, want_ll=True)
    for a, b in zip(got, ref):
        assert torch.equal(a, b)


def test_failing_inverse_checks_queued_back_to_back(dev, tuning):
    """Between the failed check and the host's next look at the pinned word nothing of the failed mode may come out either: with
    the flag set on the device, the bf16x6 pass behind every f16x3 launch re-evaluates the whole call."""
    import torch
    from gbnf_amd import native
    spec = _fail_spec("realnvp")
    z = _z(300, 21, 22, dev)
    want_x, want_l = native.NativeFlow(spec, math="bf16x6").inverse(z)
    tuning.tuning_set("check_tolerance_e9", 0)
    flow = native.NativeFlow(spec, math="default")
    outs = [flow.inverse(z) for _ in range(4)]                  # queued back to back: the host cannot have seen the flag for all
    torch.cuda.synchronize()
    for x, l in outs:
        assert torch.equal(x, want_x) and torch.equal(l, want_l)


def test_inverse_check_leaves_marked_rows_to_the_repair_pass(dev, tuning):
    """z rows beyond the fp16 range inside and outside the checked rows (17, 299): the check skips what the f16x3 launch marked,
    passes on the rest, counts nothing twice, and the call meets the x bar row by row against the exact-f32 handle."""
    import torch
    from gbnf_amd import native, synth
    spec = synth.synth_realnvp_spec(21, 105, 5, batch_norm=True, seed=4400)
    z = np.random.RandomState(4410).standard_normal((300, 21)).astype(np.float32)
    z[17] *= np.float32(1e6)
    z[299] *= np.float32(1e6)
    zd = torch.from_numpy(z).to(dev)
    xe = native.NativeFlow(spec, math="f32").inverse(zd)[0].cpu().numpy().astype(np.float64)
    assert np.isfinite(xe).all()
    plain = native.NativeFlow(spec, math="f16x3")
    native.saturation_count(reset=True)
    plain.inverse(zd)
    alone = native.saturation_count(reset=True)                 # what one f16x3 inverse launch counts on this input
    assert alone > 0
    flow = native.NativeFlow(spec, math="default")
    assert flow.info().math_mode == native.MATH["f16x3"]
    x, l = flow.inverse(zd)
    counted = native.saturation_count(reset=True)               # (synchronises)
    st = flow.numerics("inverse")
    print(f"INVGUARD marked worst {st.worst_rel_err:.3e} counted {counted} alone {alone}")
    assert st.checks == 1 and st.demoted == 0 and st.worst_rel_err <= st.tolerance
    assert counted == alone
    xs = x.cpu().numpy().astype(np.float64)
    assert np.isfinite(xs).all() and bool(torch.isfinite(l).all())
    de = _row_dev(xs, xe)
    print(f"INVGUARD marked rows vs f32 {de.max():.3e} (row {int(de.argmax())})")
    assert de.max() <= X_BAR, (int(de.argmax()), float(de.max()))


@pytest.mark.parametrize("size,L", [((3, 32, 32), 2), ((1, 28, 28), 2), ((3, 32, 32), 1)])
def test_image_inverse_check_passes_silently_and_repairs_when_it_fails(size, L, dev, tuning):
    """gbnf_image_flow_inverse: the first call checks 2 images on the exact-f32 sequence without touching x; with the tolerance at
    zero the failing call returns the exact-f32 handle's x for every image and the handle runs on exact f32 from then on."""
    import torch
    from gbnf_amd import native, synth
    sp = synth.synth_image_glow_spec(size, h=64, K=2, L=L, seed=5)
    n = 6
    flow = native.NativeImageFlow(sp)
    assert native.MATH_NAME[int(flow.numerics().math_mode)] == "f16x3"
    rng = np.random.RandomState(6)
    zd = torch.from_numpy((0.7 * rng.standard_normal((n,) + flow.z_shape)).astype(np.float32)).to(dev)
    shapes = flow.split_shapes()
    assert (len(shapes) == 0) == (L == 1)
    ed = [torch.from_numpy(rng.standard_normal((n,) + tuple(sh)).astype(np.float32)).to(dev) for sh in shapes] if L > 1 else None
    assert flow.inverse_check_counts() == {"data_checks": 0, "failed_checks": 0, "worst_rel_err": 0.0}
    x0 = flow.inverse(zd, ed, 0.9)                               # launch 0 of the direction: checked
    torch.cuda.synchronize()
    ck = flow.inverse_check_counts()
    print(f"INVGUARD image {size} L{L} worst {ck['worst_rel_err']:.3e}")
    assert ck["data_checks"] == 2 and ck["failed_checks"] == 0 and ck["worst_rel_err"] <= 2 * TOL
    x1 = flow.inverse(zd, ed, 0.9)                               # launch 1: not checked
    torch.cuda.synchronize()
    assert flow.inverse_check_counts()["data_checks"] == 2
    assert torch.equal(x0, x1)
    rc = flow.repair_counts()                                    # no forward ran: the forward counters have not moved
    assert rc["data_checks"] == 0 and rc["failed_checks"] == 0 and rc["marked_calls"] == 0
    assert not bool(flow.numerics().demoted)
    exact = native.NativeImageFlow(sp, math="f32")
    want = exact.inverse(zd, ed, 0.9)
    assert not torch.equal(x0, want)                             # the two arithmetic paths do differ in the last bits
    fresh = native.NativeImageFlow(sp)
    tuning.tuning_set("check_tolerance_e9", 0)
    x = fresh.inverse(zd, ed, 0.9)                               # checked, fails: every image re-evaluated in this call
    torch.cuda.synchronize()
    tuning.tuning_set("check_tolerance_e9", 2500)
    assert torch.equal(x, want)
    assert fresh.inverse_check_counts()["failed_checks"] >= 1 and fresh.repair_counts()["failed_checks"] == 0
    st = fresh.numerics()
    assert bool(st.demoted) and native.MATH_NAME[int(st.math_mode)] == "f32"
    xi, noise = synth.synth_image_batch(n, size, seed=9)
    xd, nd = torch.from_numpy(xi).to(dev), torch.from_numpy(noise).to(dev)
    assert torch.equal(fresh.forward(xd, nd)[0], exact.forward(xd, nd)[0])      # the forward direction follows the verdict


def test_module_numerics_status_by_direction(dev, tuning, golden_case):
    import torch
    from test_hip_module import _model_from_case
    g = golden_case("g2_glow_native_d43_h32_c3")
    m = _model_from_case(g, dev)
    keys = {"math_mode", "demoted", "checks", "worst_rel_err", "tolerance"}
    x = torch.from_numpy(g.x).to(dev)
    m.log_prob(x)
    assert set(m.numerics_status()) == keys and set(m.numerics_status(direction="forward")) == keys
    before = m.numerics_status(direction="inverse")
    assert set(before) == keys and before["checks"] == 0
    z = m(x=x, components=0)[0]
    m.component_inverse(z, 0)
    torch.cuda.synchronize()
    after = m.numerics_status(direction="inverse")
    assert after["checks"] == before["checks"] + 1 and after["demoted"] is False and after["worst_rel_err"] <= after["tolerance"]
    with pytest.raises(ValueError):
        m.numerics_status(direction="sideways")
