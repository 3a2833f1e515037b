"""The z -> x direction (gbnf_flow_inverse) against the float64 oracle, over shapes, math modes and launch forms.

Every case: x = synth_batch(n, d, seed + 1), z = float32(oracle forward of x in float64), the device inverts that z and is
compared with oracle.component_inverse(spec, z, backend="numpy64") at the project's bars (test_hip_parity.py,
test_inverse_matches_oracle_and_round_trips):

    max|x - x64|     <= 2e-5 * max(1, max|x64|)
    max|ild - ild64| <= 1e-5 * max(1, max|ild64|)

The host part (not gpu) checks the case lists themselves: on every case the float32 oracle -- the reference's own arithmetic --
is within a third of each bar of the float64 oracle, so the rule "max(bar, 3 x the float32 oracle's deviation)" never exceeds
the bars and the GPU tests use the bars as they stand; the float64 inverse of the rounded z returns x; and z stays inside the
fp16 range, so no repair launch runs in the parity tests.  (Only the out-of-range test leaves that range, on purpose.)
"""
import ctypes as C
import functools

import numpy as np
import pytest

X_BAR = 2e-5
ILD_BAR = 1e-5
MODES = ("f32", "f16x3", "bf16x6", "default")
SPLIT = ("f16x3", "bf16x6")


# ------------------------------------------------------------------ the case lists (importable without a GPU)
def _spec(kind, d, h, K, act, extra, seed):
    from gbnf_amd import synth
    if kind == "glow":
        return synth.synth_glow_spec(d, h, K, act=act, seed=seed, **extra)
    return synth.synth_realnvp_spec(d, h, K, coupling_network=act, seed=seed, **extra)


def sweep_cases():
    """1a: the generator of test_hip_shapes._cases() with its own stream and seeds and with activations drawn per step / per net
    among the choices.  (kind, d, h, K, n, act, extra, seed)"""
    rng = np.random.RandomState(3030)
    cases = []
    for k in range(36):
        kind = "glow" if k % 3 else "realnvp"
        d = int(rng.choice([2, 3, 5, 6, 8, 13, 21, 32, 43, 50, 63, 64]))
        h = int(rng.choice([7, 16, 30, 33, 48, 64, 100, 105, 112, 129, 160, 200, 215, 240, 256]))
        K = int(rng.randint(1, 6))
        n = int(rng.choice([1, 15, 16, 17, 31, 33, 64, 100, 257, 1000]))
        act = str(rng.choice(["tanh", "relu", "random"]))
        if kind == "glow":
            extra = dict(coupling=str(rng.choice(["affine", "additive"])), permutation=str(rng.choice(["shuffle", "reverse"])))
        else:
            extra = dict(batch_norm=bool(rng.randint(2)), flip_init=int(rng.randint(2)))
            act = str(rng.choice(["tanh", "relu", "mixed", "random"]))
        if k % 4 == 3:                   # every fourth case: coupling_network_depth 0 or 2
            extra["depth"] = int(rng.choice([0, 2]))
        cases.append((kind, d, h, K, n, act, extra, 700 + k))
    return cases


# 1b: 13 .. 24 steps (per-step tables in LDS as one 8-wave workgroup, or read from the blob beside a pair of 4-wave workgroups) and
# more than 24 (always from the blob); RealNVP at odd d with flipped steps: the in-half width alternates from step to step
LONG_FLOWS = [("glow", 43, 64, 13), ("realnvp", 21, 64, 14), ("glow", 43, 215, 20), ("realnvp", 21, 105, 24),
              ("glow", 64, 64, 24), ("glow", 43, 64, 26), ("realnvp", 21, 64, 25), ("glow", 43, 215, 27)]
LONG_N = (333, 5000)       # 333: a ragged last tile for 16- and 32-sample waves; 5000: more than one workgroup per CU in flight


def long_cases():
    return [(kind, d, h, K, n, "tanh", dict(flip_init=1) if kind == "realnvp" else {}, 1700 + 10 * i)
            for i, (kind, d, h, K) in enumerate(LONG_FLOWS) for n in LONG_N]


# 1c: RealNVP ResidualNets (d, h, K, blocks), n = 300
RESIDUAL_NETS = [(21, 105, 4, 1), (21, 105, 4, 2), (8, 250, 3, 1), (21, 300, 3, 2), (21, 512, 3, 1)]


def residual_cases():
    return [("realnvp", d, h, K, 300, "residual", dict(depth=blocks), 2700 + 10 * i)
            for i, (d, h, K, blocks) in enumerate(RESIDUAL_NETS)]


# 1c: activations drawn per step (Glow) / per net (RealNVP): the components of test_hip_parity.test_activation_drawn_per_step
PER_STEP_GEOMETRIES = [("glow", 43, 64, 7), ("glow", 21, 300, 6), ("realnvp", 21, 105, 6), ("realnvp", 6, 30, 8)]


def per_step_specs(kind, d, h, K):
    """[(spec, created with per_step_activation?, seed of x)]: the three drawn components and one uniform component that is packed for
    the per-step-activation kernels all the same (GBNF_CREATE_PER_STEP_ACTIVATION)."""
    from gbnf_amd import synth
    kw = {"act": "random"} if kind == "glow" else {"coupling_network": "random"}
    specs = synth.synth_boosted_specs(kind, 3, d, h, K, seed=21, **kw)
    uniform = synth.synth_boosted_specs(kind, 1, d, h, K, seed=22)[0]
    return [(s, False, 3700 + c) for c, s in enumerate(specs)] + [(uniform, True, 3703)]


_REFERENCES = {}


def reference(key, spec, n, seed):
    """(z float32, x64, ild64) of a case: computed once per process under `key`, shared, never written to."""
    if key not in _REFERENCES:
        from gbnf_amd import synth
        from oracle import gbnf_oracle as oracle
        x = synth.synth_batch(n, spec["d"], seed + 1)
        z = np.ascontiguousarray(oracle.component_forward(spec, x, backend="numpy64")[0], dtype=np.float32)
        x64, ild64 = oracle.component_inverse(spec, z, backend="numpy64")
        for a in (z, x64, ild64):
            a.setflags(write=False)
        _REFERENCES[key] = (z, x64, ild64)
    return _REFERENCES[key]


def case_reference(case):
    """spec and reference of a (kind, d, h, K, n, act, extra, seed) case."""
    kind, d, h, K, n, act, extra, seed = case
    spec = _spec(kind, d, h, K, act, extra, seed)
    return (spec,) + reference(_case_id(case), spec, n, seed)


def all_reference_inputs():
    """Every (id, spec maker, n, seed) the GPU parity tests below run on."""
    out = []
    for name, cases in (("sweep", sweep_cases()), ("long", long_cases()), ("residual", residual_cases())):
        for k, case in enumerate(cases):
            out.append((f"{name}{k}-{_case_id(case)}", functools.partial(_spec, *case[:4], *case[5:]), case[4], case[7]))
    for kind, d, h, K in PER_STEP_GEOMETRIES:
        for c in range(4):
            out.append((f"perstep-{kind}-d{d}-h{h}-K{K}-c{c}", lambda g=(kind, d, h, K), c=c: per_step_specs(*g)[c][0], 200, 3700 + c))
    return out


def _case_id(case):
    kind, d, h, K, n, act, extra, seed = case
    return f"{kind}-d{d}-h{h}-K{K}-n{n}-{act}-s{seed}"


# ------------------------------------------------------------------ 1. host: the preconditions of every case
@pytest.mark.parametrize("name,make_spec,n,seed", all_reference_inputs(), ids=[e[0] for e in all_reference_inputs()])
def test_case_preconditions(name, make_spec, n, seed):
    """The bars are attainable by the reference's own float32 arithmetic on every listed case (a third of each bar), the rounded z
    inverts back to x, and z is inside the fp16 range."""
    from gbnf_amd import synth
    from oracle import gbnf_oracle as oracle
    spec = make_spec()
    z, x64, ild64 = reference(name, spec, n, seed)
    x = synth.synth_batch(n, spec["d"], seed + 1)
    x32, ild32 = oracle.component_inverse(spec, z.copy(), backend="torch")
    xs = max(1.0, float(np.abs(x64).max()))
    ls = max(1.0, float(np.abs(ild64).max()))
    dx = float(np.abs(x32.astype(np.float64) - x64).max()) / xs
    dl = float(np.abs(ild32.astype(np.float64) - ild64).max()) / ls
    back = float(np.abs(x64 - x).max()) / max(1.0, float(np.abs(x).max()))
    print(f"PRECOND {name} f32-oracle dx {dx:.3e} dild {dl:.3e} back {back:.3e} max|z| {np.abs(z).max():.3e}")
    assert dx <= X_BAR / 3.0, (name, dx)
    assert dl <= ILD_BAR / 3.0, (name, dl)
    assert back <= 1e-6, (name, back)
    assert float(np.abs(z).max()) < 65504.0, name


def test_case_lists_cover_what_they_are_for():
    """The sweep reaches the geometries the fixtures never run backwards: even d, the smallest d, d = 64, depth 0 / 2, additive
    coupling with a reverse permutation, flipped RealNVP steps at odd d, activations drawn per step, n at the tile edges."""
    cases = sweep_cases()
    assert len(cases) == 36 and len({c[7] for c in cases}) == 36
    ds = {c[1] for c in cases}
    assert any(d % 2 == 0 for d in ds) and ds & {2, 3, 5} and 64 in ds
    assert {c[6].get("depth") for c in cases} >= {0, 2}
    assert any(c[0] == "glow" and c[6]["coupling"] == "additive" and c[6]["permutation"] == "reverse" for c in cases)
    assert any(c[0] == "realnvp" and c[1] % 2 == 1 and c[3] >= 2 for c in cases)
    assert any(c[5] == "random" for c in cases if c[0] == "glow") and any(c[5] == "random" for c in cases if c[0] == "realnvp")
    assert {c[4] for c in cases} & {15, 16, 17, 31, 33}
    assert len(long_cases()) == 16 and len(residual_cases()) == 5


# ------------------------------------------------------------------ GPU
def _dev():
    import torch
    assert torch.cuda.is_available(), "GPU tests need the MI355X"
    return torch.device("cuda:0")


def _deviation(x, ild, x64, ild64):
    """(max|x - x64| / max(1, max|x64|), max|ild - ild64| / max(1, max|ild64|))"""
    xs = max(1.0, float(np.abs(x64).max()))
    ls = max(1.0, float(np.abs(ild64).max()))
    return (float(np.abs(x.cpu().numpy().astype(np.float64) - x64).max()) / xs,
            float(np.abs(ild.cpu().numpy().astype(np.float64) - ild64).max()) / ls)


def _check(tag, flow, zd, x64, ild64, also_without_ldj=False):
    """One inverse call against the oracle at the bars; the figures are printed before they are asserted."""
    import torch
    x, ild = flow.inverse(zd)
    torch.cuda.synchronize()
    assert bool(torch.isfinite(x).all()) and bool(torch.isfinite(ild).all()), tag
    dx, dl = _deviation(x, ild, x64, ild64)
    print("INVDEV", *tag, f"dx {dx:.3e} dild {dl:.3e}")
    assert dx <= X_BAR, (tag, dx)
    assert dl <= ILD_BAR, (tag, dl)
    if also_without_ldj:                      # the same handle, no log-determinant wanted: the same x, bit for bit
        x2, none = flow.inverse(zd, want_ldj=False)
        assert none is None and torch.equal(x2, x), tag
    return x, ild


class _Tuning:
    """Launch-policy knobs pinned for a block, restored behind it."""
    KEYS = ("force_nt", "wg_pairs", "coop")

    def __enter__(self):
        from gbnf_amd import native
        self.saved = {k: native.tuning_get(k) for k in self.KEYS}
        return self

    def set(self, **kw):
        from gbnf_amd import native
        for k, v in kw.items():
            native.tuning_set(k, v)

    def __exit__(self, *exc):
        from gbnf_amd import native
        for k, v in self.saved.items():
            native.tuning_set(k, v)
        return False


@pytest.mark.gpu
@pytest.mark.parametrize("case", sweep_cases(), ids=_case_id)
def test_random_shape_backwards_against_oracle(case):
    """1a: every math mode at the automatic launch policy, the split modes again on 32-sample waves."""
    import torch
    from gbnf_amd import native
    dev = _dev()
    spec, z, x64, ild64 = case_reference(case)
    zd = torch.from_numpy(z.copy()).to(dev)
    with _Tuning() as t:
        for math in MODES:
            flow = native.NativeFlow(spec, math=math)
            for nt in ((0, 2) if math in SPLIT else (0,)):
                t.set(force_nt=nt)
                _check(("sweep", math, f"nt{nt}", _case_id(case)), flow, zd, x64, ild64, also_without_ldj=True)
            t.set(force_nt=0)
            flow.close()


@pytest.mark.gpu
@pytest.mark.parametrize("kind,d,h,K", LONG_FLOWS)
def test_long_flows_backwards_on_every_launch_form(kind, d, h, K):
    """1b: 16- / 32-sample waves x a pair of 4-wave workgroups / one 8-wave workgroup, step tables in LDS or read from the blob."""
    import torch
    from gbnf_amd import native
    dev = _dev()
    small, large = [c for c in long_cases() if c[:4] == (kind, d, h, K)]
    assert (small[4], large[4]) == LONG_N
    spec, z, x64, ild64 = case_reference(small)
    _, zl, xl64, ildl64 = case_reference(large)
    zd, zld = torch.from_numpy(z.copy()).to(dev), torch.from_numpy(zl.copy()).to(dev)
    name = f"{kind}-d{d}-h{h}-K{K}"
    with _Tuning() as t:
        for math in SPLIT:
            flow = native.NativeFlow(spec, math=math)
            for nt in (1, 2):
                for pairs in (0, 1):
                    t.set(force_nt=nt, wg_pairs=pairs)
                    _check(("long", math, f"nt{nt}-pairs{pairs}", name), flow, zd, x64, ild64)
            t.set(force_nt=0, wg_pairs=-1)
            _check(("long", math, "auto-n5000", name), flow, zld, xl64, ildl64)
            flow.close()
        flow = native.NativeFlow(spec, math="f32")
        _check(("long", "f32", "auto", name), flow, zd, x64, ild64)
        flow.close()


def residual_modes(h, blocks):
    """The math modes include/gbnf.h states for a RealNVP ResidualNet component (LIMITS of gbnf_flow_create): one or two blocks run on
    the split kernels at every width 1 <= h <= 512, and the exact-f32 kernel takes ResidualNets of <= 2 blocks to h = 512."""
    assert 1 <= h <= 512 and blocks in (1, 2)
    return set(MODES)


@pytest.mark.gpu
@pytest.mark.parametrize("case", residual_cases(), ids=_case_id)
def test_residual_nets_backwards_against_oracle(case):
    """1c: ResidualNets of one and two blocks, narrow and wide, every math mode the handle exists in, 16- and 32-sample waves."""
    import torch
    from gbnf_amd import native
    dev = _dev()
    kind, d, h, K, n, act, extra, seed = case
    spec, z, x64, ild64 = case_reference(case)
    zd = torch.from_numpy(z.copy()).to(dev)
    stated = residual_modes(h, extra["depth"])
    with _Tuning() as t:
        for math in MODES:
            try:
                flow = native.NativeFlow(spec, math=math)
            except native.GbnfError as e:        # a refusal is GBNF_ERR_UNSUPPORTED, and only where the header states no such mode
                assert math not in stated and "error -2:" in str(e), (math, str(e))
                continue
            assert math in stated, math
            for nt in (1, 2):
                t.set(force_nt=nt)
                _check(("residual", math, f"nt{nt}", _case_id(case)), flow, zd, x64, ild64)
            t.set(force_nt=0)
            flow.close()


@pytest.mark.gpu
@pytest.mark.parametrize("kind,d,h,K", PER_STEP_GEOMETRIES)
def test_per_step_activations_backwards_against_oracle(kind, d, h, K):
    """1c: the per-step-activation kernel variants, x and the log-determinant."""
    import torch
    from gbnf_amd import native
    dev = _dev()
    for c, (spec, flag, seed) in enumerate(per_step_specs(kind, d, h, K)):
        assert seed == 3700 + c
        z, x64, ild64 = reference(f"perstep-{kind}-d{d}-h{h}-K{K}-c{c}", spec, 200, seed)
        zd = torch.from_numpy(z.copy()).to(dev)
        for math in (("f32", "f16x3") if h <= 256 else ("f16x3",)):       # hidden widths above 256 with drawn activations: split kernels
            flow = native.NativeFlow(spec, math=math, per_step_activation=flag)
            _check(("perstep", math, "flag" if flag else "drawn", f"{kind}-d{d}-h{h}-K{K}-c{c}"), flow, zd, x64, ild64)
            flow.close()


# ------------------------------------------------------------------ 1d. edges of the direction
SENTINEL = 0x7FC0BEEF      # a quiet NaN with a payload, as int32


@pytest.mark.gpu
@pytest.mark.parametrize("math", ["f32", "f16x3", "bf16x6"])
@pytest.mark.parametrize("kind", ["glow", "realnvp"])
def test_inverse_writes_nothing_beyond_n(kind, math):
    """gbnf_flow_inverse through the C ABI into buffers 64 rows longer than n: rows at and beyond n keep their bits, with and without
    the log-determinant output, on 16- and 32-sample waves; the rows below n meet the bars."""
    import torch
    from gbnf_amd import native, synth
    dev = _dev()
    L = native.lib()
    d = 43 if kind == "glow" else 21
    spec = synth.synth_glow_spec(d, 64, 3, seed=4100) if kind == "glow" else synth.synth_realnvp_spec(d, 64, 3, flip_init=1, seed=4101)
    flow = native.NativeFlow(spec, math=math)
    with _Tuning() as t:
        for n in (1, 17, 33, 65, 257):
            z, x64, ild64 = reference(f"canary-{kind}-n{n}", spec, n, 4200 + n)
            zd = torch.from_numpy(z.copy()).to(dev)
            for nt in (1, 2):
                t.set(force_nt=nt)
                for with_ldj in (True, False):
                    xbuf = torch.full((n + 64, d), SENTINEL, dtype=torch.int32, device=dev)
                    lbuf = torch.full((n + 64,), SENTINEL, dtype=torch.int32, device=dev)
                    rc = L.gbnf_flow_inverse(flow.handle, C.c_void_p(zd.data_ptr()), n, C.c_void_p(xbuf.data_ptr()),
                                             C.c_void_p(lbuf.data_ptr()) if with_ldj else C.c_void_p(0), native._stream_ptr())
                    assert rc == 0, L.gbnf_last_error()
                    torch.cuda.synchronize()
                    tag = (kind, math, n, nt, with_ldj)
                    assert bool((xbuf[n:] == SENTINEL).all()), tag
                    assert bool((lbuf[n if with_ldj else 0:] == SENTINEL).all()), tag
                    ild = lbuf[:n].view(torch.float32) if with_ldj else torch.from_numpy(ild64.copy())
                    dx, dl = _deviation(xbuf[:n].view(torch.float32), ild, x64, ild64)
                    assert dx <= X_BAR and dl <= ILD_BAR, (tag, dx, dl)
    flow.close()


@pytest.mark.gpu
@pytest.mark.parametrize("math", SPLIT)
@pytest.mark.parametrize("kind,d,h", [("glow", 43, 215), ("realnvp", 21, 105)])
def test_inverse_is_deterministic_and_tile_independent(kind, d, h, math):
    """With the launch form pinned, a row's x and log-determinant do not depend on the rows around it, nor on the run."""
    import torch
    from gbnf_amd import native, synth
    dev = _dev()
    spec = synth.synth_glow_spec(d, h, 5, seed=4300) if kind == "glow" else synth.synth_realnvp_spec(d, h, 5, batch_norm=True, seed=4301)
    z, x64, ild64 = reference(f"tiles-{kind}", spec, 1000, 4310)
    zd = torch.from_numpy(z.copy()).to(dev)
    head = zd[:100].contiguous()
    flow = native.NativeFlow(spec, math=math)
    with _Tuning() as t:
        for nt in (1, 2):
            for pairs in (0, 1):
                t.set(force_nt=nt, wg_pairs=pairs)
                xa, la = _check(("tiles", math, f"nt{nt}-pairs{pairs}", f"{kind}-d{d}-h{h}"), flow, zd, x64, ild64)
                xb, lb = flow.inverse(zd)
                xh, lh = flow.inverse(head)
                assert torch.equal(xa, xb) and torch.equal(la, lb), (nt, pairs)
                assert torch.equal(xh, xa[:100]) and torch.equal(lh, la[:100]), (nt, pairs)
    flow.close()


def _row_dev(x, ref):
    """per row: max|x - ref| / max(1, max|ref|) over the row's features"""
    return np.abs(x - ref).max(axis=1) / np.maximum(1.0, np.abs(ref).max(axis=1))


@pytest.mark.gpu
@pytest.mark.parametrize("kind", ["realnvp", "glow_additive"])
def test_out_of_range_rows_backwards_are_repaired(kind):
    """z rows beyond the fp16 range: marked by the f16x3 launch and re-evaluated by the bf16x6 launch behind it, backwards as forwards
    (every value involved is finite).  Each row is held to the x bar on its own scale: against the exact-f32 kernel, and against the
    float64 oracle where that is finite.  bf16x6 handles need no repair."""
    import torch
    from gbnf_amd import native, synth
    from oracle import gbnf_oracle as oracle
    dev = _dev()
    if kind == "realnvp":
        spec = synth.synth_realnvp_spec(21, 105, 5, batch_norm=True, seed=4400)
    else:
        spec = synth.synth_glow_spec(8, 64, 3, coupling="additive", seed=4401)
    d = spec["d"]
    z = np.random.RandomState(4410).standard_normal((300, d)).astype(np.float32)
    z[17] *= np.float32(1e6)
    z[299] *= np.float32(1e6)
    zd = torch.from_numpy(z.copy()).to(dev)
    xe = native.NativeFlow(spec, math="f32").inverse(zd)[0].cpu().numpy().astype(np.float64)
    assert np.isfinite(xe).all()
    with np.errstate(all="ignore"):
        x64 = oracle.component_inverse(spec, z, backend="numpy64")[0]
    fin = np.isfinite(x64).all(axis=1)
    assert fin[[0, 16, 18, 298]].all()

    def judge(tag, x):
        x = x.cpu().numpy().astype(np.float64)
        assert np.isfinite(x).all(), tag
        de = _row_dev(x, xe)
        do = _row_dev(x[fin], x64[fin])
        print("INVDEV range", *tag, f"rows vs f32 {de.max():.3e} (row {int(de.argmax())}) vs oracle {do.max():.3e}")
        assert de.max() <= X_BAR, (tag, int(de.argmax()), float(de.max()))
        assert do.max() <= X_BAR, (tag, float(do.max()))

    with _Tuning() as t:
        for math in ("default", "f16x3"):
            flow = native.NativeFlow(spec, math=math)
            assert flow.info().math_mode == native.MATH["f16x3"]
            for nt in (1, 2):
                t.set(force_nt=nt)
                native.saturation_count(reset=True)
                x, _ = flow.inverse(zd)
                assert native.saturation_count(reset=True) > 0, (math, nt)
                judge((kind, math, f"nt{nt}"), x)
            flow.close()
        flow = native.NativeFlow(spec, math="bf16x6")
        for nt in (1, 2):
            t.set(force_nt=nt)
            native.saturation_count(reset=True)
            x, _ = flow.inverse(zd)
            assert native.saturation_count(reset=True) == 0, nt
            judge((kind, "bf16x6", f"nt{nt}"), x)
        flow.close()
