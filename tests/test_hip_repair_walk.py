"""GPU: the walking form of the bf16x6 repair launch (csrc/gbnf_flow_kernel_hx3.hip.h: a repair launch has at most 256 workgroups;
past that, each walks the work list with a stride of gridDim.x -- the one place where a workgroup runs the kernel body more than
once).  Range repair and the numerics guard's re-evaluation on launches past that grid, through the C ABI.

No tolerance of this file's own.  The references are the project's kernels bit for bit and the float64 oracle at the existing bars:
  bf    a math="bf16x6" handle on the same spec (run as one 8-wave workgroup per item, the form a repair launch has);
  bare  the f16x3 handle with tuning "repair" = 0: the rows it marks (NaN) are S, and S must be exactly the rows the test pushed out of
        the fp16 range (rows are independent of each other);
  the repaired call equals bf on S, bit for bit, is finite everywhere, and meets the oracle on S at 1e-5 for ll / ldj (BASELINE.json,
  conftest.rel_err) and 2e-5 max(1, |z|) for z.  Off S every row is bare's or bf's, bit for bit, and which of the two is pinned as
  well: a repair launch re-evaluates whole work items, so the unmarked rows that share an item with a marked one are bf's and the rows
  of every other item are bare's (_three_way).
The case lists live in tests/repair_walk_cases.py (checked on the host by tests/test_repair_walk_host.py).
"""
import numpy as np
import pytest

import repair_walk_cases as rw
from conftest import rel_err

pytestmark = pytest.mark.gpu

LL_RTOL = 1e-5            # ll, ldj, log|det| (tests/test_hip_parity.py, tests/test_hip_inverse.py ILD_BAR)
Z_BAR = 2e-5              # z and x, of max(1, |value|)
LSE_RTOL = 5e-6           # G == LSE(ll + log w) in float64 (tests/test_hip_baseline_configs.py)
KEYS = ("force_nt", "wg_pairs", "repair", "coop", "check_every", "check_tolerance_e9")


@pytest.fixture(scope="module")
def dev():
    import torch
    assert torch.cuda.is_available(), "GPU tests need the MI355X"
    return torch.device("cuda:0")


@pytest.fixture()
def tuning():
    from gbnf_amd import native
    saved = {k: native.tuning_get(k) for k in KEYS}

    def set_keys(**kw):
        for k, v in kw.items():
            assert k in saved
            native.tuning_set(k, v)
    try:
        yield set_keys
    finally:
        for k, v in saved.items():
            native.tuning_set(k, v)
        native.saturation_count(reset=True)


_FLOWS, _MIXTURES = {}, {}


def _flow(gid, math):
    """f16x3 / bf16x6 handles of a geometry: created once per process (explicit modes carry no guard state)."""
    from gbnf_amd import native
    if (gid, math) not in _FLOWS:
        _FLOWS[gid, math] = native.NativeFlow(rw.spec_of(gid), math=math)
    return _FLOWS[gid, math]


def _mixture(gid, math):
    from gbnf_amd import native
    if (gid, math) not in _MIXTURES:
        _MIXTURES[gid, math] = native.mixture_from_specs(rw.mixture_specs(gid), math=math)
    return _MIXTURES[gid, math][0]


def _to(dev, x):
    """A host batch (possibly one of the shared read-only ones) as a device tensor of its own."""
    import torch
    return torch.from_numpy(np.array(x)).to(dev)


def _nan_rows(t):
    """Rows of a (n,) or (n, d) tensor that hold a NaN."""
    import torch
    bad = torch.isnan(t)
    return torch.nonzero(bad if bad.dim() == 1 else bad.any(dim=1)).flatten()


def _same_rows(a, b):
    """Per row: are a and b the same bits?  (both finite where it matters: == is bit equality up to the sign of zero)"""
    same = a == b
    return same if same.dim() == 1 else same.all(dim=1)


def _three_way(tag, gots, bares, bfs, rows, n):
    """Every output of one call (tensors with the rows along dim 0): finite everywhere; the rows the bare launch marks are exactly
    `rows`; == bf on them, bit for bit.  A repair launch re-evaluates whole work items, so the unmarked rows of an item that holds a
    mark come back as bf's too, and the rows of every other item as bare's: that must hold, for all outputs alike, with an item of 64,
    128 or 256 rows (which of them is the variant's business).  Every row is accounted for, bit for bit, by one of the two references."""
    import torch
    dev = gots[0].device
    idx = torch.from_numpy(rows).to(dev)
    for got, bare, bf in zip(gots, bares, bfs):
        assert got.shape[0] == n and bool(torch.isfinite(got).all()), (tag, "a row was left unrepaired or came back non-finite")
        assert bool(torch.isfinite(bf).all()), tag                                   # precondition: bf16x6 needs no repair
        assert torch.equal(_nan_rows(bare), idx), (tag, "the rows the bare f16x3 launch marks are not the rows the test marked")
        if bare.dim() == 2:
            assert bool(torch.isnan(bare[idx]).all()), tag                            # a marked row is marked in every feature
        assert torch.equal(got[idx], bf[idx]), (tag, "marked rows differ from the bf16x6 handle's")
    fits = []
    row = torch.arange(n, device=dev)
    for rpi in rw.ROWS_PER_ITEM:
        holds_mark = torch.zeros(-(-n // rpi), dtype=torch.bool, device=dev)
        holds_mark[idx // rpi] = True
        redone = holds_mark[row // rpi]
        if all(bool(_same_rows(got, bf)[redone].all()) and bool(_same_rows(got, bare)[~redone].all())
               for got, bare, bf in zip(gots, bares, bfs)):
            fits.append(rpi)
    assert fits, (tag, "some row is neither the bf16x6 handle's (items that hold a mark) nor the bare f16x3 launch's (all others)")
    return fits


def _z_ok(z, z64):
    return bool((np.abs(z.astype(np.float64) - z64) <= Z_BAR * np.maximum(1.0, np.abs(z64))).all())


def _forward_references(tuning, gid, n, nt, pairs, pattern, dev, coop=-1):
    """(x marked on the device, x marked on the host, rows, bare (z, ldj, ll), bf (z, ldj, ll)) of a single-flow forward case; the
    preconditions are asserted on the way.  Leaves force_nt / wg_pairs / coop as the case wants them and repair = 1."""
    from gbnf_amd import native
    fast, safe = _flow(gid, "f16x3"), _flow(gid, "bf16x6")
    x, rows, xm = rw.forward_inputs(gid, n, pattern)
    xd, xmd = _to(dev, x), _to(dev, xm)
    tuning(force_nt=nt, wg_pairs=pairs, coop=coop, repair=1)
    native.saturation_count(reset=True)
    fast.forward(xd, want_ll=True)
    assert native.saturation_count() == 0, (gid, n, "the unmodified batch leaves the fp16 range")
    tuning(wg_pairs=0, coop=0)
    bf = safe.forward(xmd, want_ll=True)
    tuning(wg_pairs=pairs, coop=coop, repair=0)
    bare = fast.forward(xmd, want_ll=True)
    tuning(repair=1)
    native.saturation_count(reset=True)
    return xmd, xm, rows, bare, bf


def _forward_case(tuning, gid, n, nt, pairs, pattern, dev, coop=-1):
    import torch
    from gbnf_amd import native
    from oracle import gbnf_oracle as oracle
    tag = (gid, n, f"nt{nt}", f"pairs{pairs}", pattern, f"coop{coop}")
    xmd, xm, rows, bare, bf = _forward_references(tuning, gid, n, nt, pairs, pattern, dev, coop)
    got = _flow(gid, "f16x3").forward(xmd, want_ll=True)
    assert native.saturation_count(reset=True) > 0, tag
    fits = _three_way(tag, got, bare, bf, rows, n)
    sub = rw.oracle_rows(rows)
    spec = rw.spec_of(gid)
    z64, ldj64 = oracle.component_forward(spec, xm[sub], backend="numpy64")
    ll64 = oracle.component_log_prob(spec, xm[sub], backend="numpy64")
    idx = torch.from_numpy(sub).to(dev)
    z, ldj, ll = (t[idx].cpu().numpy() for t in got)
    print("WALK", *tag, f"rows per item {fits} S {rows.size} ll {rel_err(ll, ll64):.3e} ldj {rel_err(ldj, ldj64):.3e} "
          f"z {float(np.max(np.abs(z - z64) / np.maximum(1.0, np.abs(z64)))):.3e}")
    assert rel_err(ll, ll64) < LL_RTOL and rel_err(ldj, ldj64) < LL_RTOL, tag
    assert _z_ok(z, z64), tag
    return got


# ------------------------------------------------------------------ 3.1 forward, one flow
@pytest.mark.parametrize("pairs", [0, 1])
@pytest.mark.parametrize("nt", rw.FORCE_NT)
@pytest.mark.parametrize("n", rw.ROW_COUNTS)
def test_walking_repair_of_one_flow_on_the_geometry_of_the_repair_tests(n, nt, pairs, dev, tuning):
    """G1 over every row count: launches of exactly 256 items, of 257 and of >= 513 whatever the rows per item are."""
    for pattern in rw.PATTERNS:
        _forward_case(tuning, "G1", n, nt, pairs, pattern, dev)


@pytest.mark.parametrize("nt", rw.FORCE_NT)
@pytest.mark.parametrize("n", rw.SHORT_COUNTS)
@pytest.mark.parametrize("gid", [g for g in sorted(rw.GEOMETRIES) if g != "G1"])
def test_walking_repair_of_one_flow_on_every_kernel_structure(gid, n, nt, dev, tuning):
    """G2 .. G7: two nets per step, the heaviest stages, depth 2, ResidualNets, 28 hidden tiles, step tables read from the blob."""
    assert n in rw.GEOMETRIES[gid]["counts"]
    for pattern in rw.PATTERNS:
        _forward_case(tuning, gid, n, nt, -1, pattern, dev)


# ------------------------------------------------------------------ 3.2 each output alone: the probe's three branches
@pytest.mark.parametrize("nt", rw.FORCE_NT)
@pytest.mark.parametrize("gid", ["G1", "G3"])
def test_walking_repair_finds_the_marks_in_whichever_output_exists(gid, nt, dev, tuning):
    import torch
    n = 70001
    fast = _flow(gid, "f16x3")
    for pattern in rw.PATTERNS:
        xmd = _to(dev, rw.forward_inputs(gid, n, pattern)[2])
        tuning(force_nt=nt, repair=1)
        z, ldj, ll = fast.forward(xmd, want_ll=True)
        assert all(bool(torch.isfinite(t).all()) for t in (z, ldj, ll))
        only_z = fast.forward(xmd, want_ldj=False, want_ll=False)
        assert only_z[1] is None and only_z[2] is None and torch.equal(only_z[0], z), (gid, nt, pattern, "z alone")
        only_ldj = fast.forward(xmd, want_z=False, want_ll=False)
        assert only_ldj[0] is None and only_ldj[2] is None and torch.equal(only_ldj[1], ldj), (gid, nt, pattern, "ldj alone")
        only_ll = fast.forward(xmd, want_z=False, want_ldj=False, want_ll=True)
        assert only_ll[0] is None and only_ll[1] is None and torch.equal(only_ll[2], ll), (gid, nt, pattern, "ll alone")


# ------------------------------------------------------------------ 3.3 mixture and group launches
def _lse64(ll, rho):
    w = rho.astype(np.float64) / rho.astype(np.float64).sum()
    a = ll.astype(np.float64) + np.log(w)[:, None]
    m = a.max(axis=0)
    return m + np.log(np.exp(a - m).sum(axis=0))


@pytest.mark.parametrize("k", [0, 1, 2, 3])
@pytest.mark.parametrize("S", [2, 3])
@pytest.mark.parametrize("gid", ["G1", "G2"])
def test_walking_repair_of_group_launches(gid, S, k, dev, tuning):
    """C = 3 components x S batches in one launch, n C S = 16385 (1, 2, 4, 8): other marked rows in every batch, the last batch (and
    with it the end of the last component's run of items) marked densely."""
    import torch
    from gbnf_amd import native
    from oracle import gbnf_oracle as oracle
    C = 3
    n, rows, plain, marked = rw.group_inputs(gid, S, k, C)
    specs = rw.mixture_specs(gid)
    fast, safe = _mixture(gid, "f16x3"), _mixture(gid, "bf16x6")
    xs = [_to(dev, x) for x in plain]
    xms = [_to(dev, x) for x in marked]

    def group(mix, batches):
        out = torch.empty((C, S * n), dtype=torch.float32, device=dev)
        mix.prepared_group_log_prob(batches, out)(native._stream_ptr())
        return out

    for nt in rw.FORCE_NT:
        tag = (gid, f"S{S}", n, f"nt{nt}")
        tuning(force_nt=nt, wg_pairs=-1, repair=1)
        native.saturation_count(reset=True)
        group(fast, xs)
        assert native.saturation_count() == 0, tag
        tuning(wg_pairs=0)
        bf = group(safe, xms)
        tuning(wg_pairs=-1, repair=0)
        bare = group(fast, xms)
        tuning(repair=1)
        native.saturation_count(reset=True)
        got = group(fast, xms)
        assert native.saturation_count(reset=True) > 0, tag
        for b in range(S):                                      # column block by column block, the C components of a block together
            blk = slice(b * n, (b + 1) * n)
            _three_way(tag + (f"b{b}",), tuple(got[:, blk]), tuple(bare[:, blk]), tuple(bf[:, blk]), rows[b], n)
        for c in range(C):                                       # the oracle on marked rows of the first and the last batch
            for b in (0, S - 1):
                sub = rw.oracle_rows(rows[b])[::3]
                ll64 = oracle.component_log_prob(specs[c], marked[b][sub], backend="numpy64")
                ll = got[c, b * n:(b + 1) * n][torch.from_numpy(sub).to(dev)].cpu().numpy()
                assert rel_err(ll, ll64) < LL_RTOL, tag + (c, b, rel_err(ll, ll64))
        # the measured path: two of the three components and the mixture's log-sum-exp over the repaired table
        rho = oracle.rho_init(C)
        x_last = xms[S - 1]
        G, ll2 = fast.log_prob(x_last, torch.from_numpy(rho).to(dev), n_used=2)
        assert native.saturation_count(reset=True) > 0, tag
        assert torch.equal(ll2, got[:2, (S - 1) * n:]), tag       # the same rows in a launch of another shape: the same bits
        assert bool(torch.isfinite(G).all()), tag
        err = rel_err(G.cpu().numpy(), _lse64(ll2.cpu().numpy(), rho[:2]))
        print("WALK group", *tag, f"G vs LSE {err:.3e}")
        assert err < LSE_RTOL, tag


# ------------------------------------------------------------------ 3.4 the latency form in front of a walking repair
@pytest.mark.parametrize("gid", ["G1", "G3"])
def test_walking_repair_behind_the_latency_form(gid, dev, tuning):
    """tuning "coop" forced: the f16x3 launch is the cooperative kernel where the geometry builds that form (else the throughput
    kernel, which the other tests cover), its marks are read by the same walking bf16x6 launch."""
    import torch
    n, ran = 70001, 0
    plain = None
    for form in (1, 2, 3):
        got = _forward_case(tuning, gid, n, 0, -1, "marked", dev, coop=form)
        if plain is None:
            tuning(coop=0)
            plain = _flow(gid, "f16x3").forward(_to(dev, rw.forward_inputs(gid, n, "marked")[2]), want_ll=True)
        ran += int(not torch.equal(got[2], plain[2]))
    if gid == "G3":                # (csrc/variants.list: `coop 0 14 3 0 0`, all three forms)
        assert ran >= 1, "no cooperative form of this geometry ran"


# ------------------------------------------------------------------ 3.5 guard trips past the grid
def _default_mixture(gid, C):
    from gbnf_amd import native
    specs = rw.mixture_specs(gid)[:C] if C > 1 else [rw.spec_of(gid)]
    mix, flows = native.mixture_from_specs(specs, math="default")
    assert mix.numerics().math_mode == native.MATH["f16x3"], "the creation probe did not choose f16x3 for this geometry"
    return mix, flows


def _safe_mixture(gid, C):
    from gbnf_amd import native
    if C > 1:
        return _mixture(gid, "bf16x6")
    key = (gid + "/1", "bf16x6")
    if key not in _MIXTURES:
        _MIXTURES[key] = (native.NativeMixture([_flow(gid, "bf16x6")]), None)
    return _MIXTURES[key][0]


@pytest.mark.parametrize("n,C", [(70001, 1), (32769, 3)])
@pytest.mark.parametrize("gid", ["G1", "G2"])
def test_failed_check_re_evaluates_a_launch_past_the_repair_grid(gid, n, C, dev, tuning):
    """tolerance 0 => the first on-data check fails: the checked launch comes back as the bf16x6 results on ALL rows although its
    re-evaluation launch has 256 workgroups for more work items than that; single launch and two-batch group."""
    import torch
    from gbnf_amd import native
    d = rw.spec_of(gid)["d"]
    x, x2 = _to(dev, rw.batch(d, n, seed=200)), _to(dev, rw.batch(d, n, seed=201))
    safe = _safe_mixture(gid, C)
    for nt in rw.FORCE_NT:
        tuning(force_nt=nt, wg_pairs=0, check_tolerance_e9=2500)
        want, want2 = safe.component_log_prob(x), safe.component_log_prob(x2)
        tuning(wg_pairs=-1)
        fast = _mixture(gid, "f16x3").component_log_prob(x) if C > 1 else _flow(gid, "f16x3").forward(x, want_ll=True)[2][None]
        assert not torch.equal(fast, want)                                   # the two modes do differ in the last bits
        tuning(check_tolerance_e9=0)
        mix, flows = _default_mixture(gid, C)
        got = mix.component_log_prob(x)                                      # launch 0: checked, fails, re-evaluated on the device
        torch.cuda.synchronize()
        st = mix.numerics()
        assert st.checks == 1 and st.demoted == 1 and st.math_mode == native.MATH["bf16x6"], (gid, n, C, nt)
        assert torch.equal(got, want), (gid, n, C, nt)
        # the group form: two batches in one launch, twice the work items
        mix2, flows2 = _default_mixture(gid, C)
        table = torch.empty((C, 2 * n), dtype=torch.float32, device=dev)
        mix2.prepared_group_log_prob([x, x2], table)(native._stream_ptr())
        torch.cuda.synchronize()
        assert mix2.numerics().demoted == 1, (gid, n, C, nt)
        assert torch.equal(table[:, :n], want) and torch.equal(table[:, n:], want2), (gid, n, C, nt)
        if C == 1:                                                           # a single flow handle has a guard of its own: z and ldj too
            tuning(wg_pairs=0, check_tolerance_e9=2500)
            wz, wl, wll = _flow(gid, "bf16x6").forward(x, want_ll=True)
            tuning(wg_pairs=-1, check_tolerance_e9=0)
            flow = native.NativeFlow(rw.spec_of(gid), math="default")
            z, ldj, ll = flow.forward(x, want_ll=True)
            torch.cuda.synchronize()
            assert flow.numerics().demoted == 1, (gid, n, nt)
            assert torch.equal(z, wz) and torch.equal(ldj, wl) and torch.equal(ll, wll), (gid, n, nt)
        tuning(check_tolerance_e9=2500)


@pytest.mark.parametrize("gid", ["G1", "G2"])
def test_guard_flag_redoes_queued_launches_past_the_repair_grid(gid, dev, tuning):
    """Four calls queued before any synchronisation: the host cannot have seen the flag for all of them, so the walking bf16x6 launch
    behind each f16x3 launch re-evaluates the whole work list."""
    import torch
    from gbnf_amd import native
    n = 70001
    x = _to(dev, rw.batch(rw.spec_of(gid)["d"], n, seed=202))
    for nt in rw.FORCE_NT:
        tuning(force_nt=nt, wg_pairs=0, check_tolerance_e9=2500)
        want = _flow(gid, "bf16x6").forward(x, want_ll=True)
        tuning(wg_pairs=-1, check_tolerance_e9=0)
        flow = native.NativeFlow(rw.spec_of(gid), math="default")
        assert flow.numerics().math_mode == native.MATH["f16x3"]
        outs = [flow.forward(x, want_ll=True) for _ in range(4)]
        torch.cuda.synchronize()
        assert flow.numerics().demoted == 1
        for i, out in enumerate(outs):
            for a, b in zip(out, want):
                assert torch.equal(a, b), (gid, nt, i)


# ------------------------------------------------------------------ 3.6 the z -> x direction
@pytest.mark.parametrize("nt", rw.FORCE_NT)
@pytest.mark.parametrize("n", rw.SHORT_COUNTS)
@pytest.mark.parametrize("gid", rw.INVERSE_GEOMETRIES)
def test_walking_repair_backwards(gid, n, nt, dev, tuning):
    import torch
    from gbnf_amd import native
    from oracle import gbnf_oracle as oracle
    tag = (gid, n, f"nt{nt}", "inverse")
    fast, safe = _flow(gid, "f16x3"), _flow(gid, "bf16x6")
    z, rows, zm = rw.inverse_inputs(gid, n)
    zd, zmd = _to(dev, z), _to(dev, zm)
    tuning(force_nt=nt, wg_pairs=-1, repair=1)
    native.saturation_count(reset=True)
    fast.inverse(zd)
    assert native.saturation_count() == 0, tag
    tuning(wg_pairs=0)
    bf = safe.inverse(zmd)
    tuning(wg_pairs=-1, repair=0)
    bare = fast.inverse(zmd)
    tuning(repair=1)
    native.saturation_count(reset=True)
    got = fast.inverse(zmd)
    assert native.saturation_count(reset=True) > 0, tag
    fits = _three_way(tag, got, bare, bf, rows, n)
    x_only, none = fast.inverse(zmd, want_ldj=False)                       # the probe reads x where there is no log|det|
    assert none is None and torch.equal(x_only, got[0]), tag
    native.saturation_count(reset=True)
    sub = rw.oracle_rows(rows)
    x64, ild64 = oracle.component_inverse(rw.spec_of(gid), zm[sub], backend="numpy64")
    idx = torch.from_numpy(sub).to(dev)
    x, ild = got[0][idx].cpu().numpy(), got[1][idx].cpu().numpy()
    print("WALK", *tag, f"rows per item {fits} x {float(np.max(np.abs(x - x64) / np.maximum(1.0, np.abs(x64)))):.3e} ild {rel_err(ild, ild64):.3e}")
    assert _z_ok(x, x64), tag
    assert rel_err(ild, ild64) < LL_RTOL, tag


@pytest.mark.parametrize("gid", rw.INVERSE_GEOMETRIES)
def test_failed_inverse_check_re_evaluates_a_call_past_the_repair_grid(gid, dev, tuning):
    import torch
    from gbnf_amd import native
    n = 70001
    z = _to(dev, rw.batch(rw.spec_of(gid)["d"], n, seed=203))
    for nt in rw.FORCE_NT:
        tuning(force_nt=nt, wg_pairs=0, check_tolerance_e9=2500)
        want_x, want_l = _flow(gid, "bf16x6").inverse(z)
        tuning(wg_pairs=-1)
        assert not torch.equal(_flow(gid, "f16x3").inverse(z)[0], want_x)    # the two modes do differ in the last bits
        tuning(check_tolerance_e9=0)
        flow = native.NativeFlow(rw.spec_of(gid), math="default")
        assert flow.numerics("inverse").math_mode == native.MATH["f16x3"]
        x, l = flow.inverse(z)                                               # launch 0 of the direction: checked, fails, re-evaluated
        torch.cuda.synchronize()
        st = flow.numerics("inverse")
        assert st.checks == 1 and st.demoted == 1 and st.math_mode == native.MATH["bf16x6"], (gid, nt)
        assert torch.equal(x, want_x) and torch.equal(l, want_l), (gid, nt)
