"""CPU: the host layer both model families share -- ``boosted_base.BoostedMixtureBase`` (constructor order, ``_n_used`` and its two
defaults, the component draw, the loader cycle, the rho loop, the un-normalised recursion, the ``fit_weights`` skeleton) and the one
calling idiom of ``native`` (size queries, workspaces, handle life time, the trainers' shared base).  Tiny modules on the CPU; nothing
here computes on a device."""
import ctypes as C
import hashlib
import itertools
import json
import os

import numpy as np
import pytest
import torch

import test_image_boost_host as boost_host
from conftest import GOLDEN_DIR
from gbnf_amd import BoostedFlow, native
from test_host_module import make_args

SEED = 20
RECORDING = os.path.join(GOLDEN_DIR, "boosted_base_state_dicts.json")
CPU = torch.device("cpu")


def tabular_model(kind="glow", **extra):
    args = make_args(kind=kind, d=4, h=8, K=2, C=3)
    args.rho_iters, args.rho_lr = 40, 0.05
    for k, v in extra.items():
        setattr(args, k, v)
    return BoostedFlow(args)


def image_model(**extra):
    return BoostedFlow(boost_host.image_args((1, 4, 4), 8, 2, 2, CPU, C_=3, permutation="shuffle", rho_iters=40, **extra))


MODELS = {"tabular_glow": lambda: tabular_model("glow"), "tabular_realnvp": lambda: tabular_model("realnvp"), "image_glow": image_model}
FAMILIES = {"tabular": tabular_model, "image": image_model}


def state_digest(model):
    """The key order of ``state_dict()`` and a SHA-256 of every tensor's bytes."""
    sd = model.state_dict()
    return {"keys": list(sd), "sha256": {k: hashlib.sha256(v.detach().cpu().contiguous().numpy().tobytes()).hexdigest() for k, v in sd.items()}}


# ---------------------------------------------------------------------------------------------------------------- the modules
def test_the_two_modules_share_the_base_and_nothing_else():
    from gbnf_amd import boosted_base, image_glow
    import gbnf_amd
    t, i = tabular_model(), image_model()
    assert type(t) is BoostedFlow and type(i) is image_glow.BoostedImageFlow
    assert isinstance(t, boosted_base.BoostedMixtureBase) and isinstance(i, boosted_base.BoostedMixtureBase)
    assert not isinstance(i, BoostedFlow)
    assert not hasattr(gbnf_amd, "BoostedMixtureBase")
    for name in ("increment_component", "_sample_component", "_n_used", "_require_device", "_log_w", "_rho_in_place", "_cycle", "_rho_loop",
                 "_mixture_recursion", "_fit_weights_over", "_eval_sums", "_score_result", "_check_component", "_apply"):
        assert name not in vars(BoostedFlow) and name not in vars(image_glow.BoostedImageFlow), f"{name} is written twice again"


@pytest.mark.parametrize("name", sorted(MODELS))
def test_same_seed_same_model(name):
    """The constructor draws in the order it always did: base_dist_mean first, then the components."""
    want = json.load(open(RECORDING))
    torch.manual_seed(want["seed"])
    got = state_digest(MODELS[name]())
    assert got["keys"] == want[name]["keys"]
    assert got["keys"][:3] == ["base_dist_mean", "base_dist_var", "rho"]
    assert got["sha256"] == want[name]["sha256"]


# Which default ``n_used=None`` takes at every public method: "trained" = the components trained so far (component + 1, all of them
# once all_trained), "all" = num_components whatever has been trained.  The image module's evaluation-path methods take "all".
N_USED_DEFAULT = {
    "tabular": {"sample": "trained", "numerics_status": "trained", "mixture_training_step": "trained", "component_log_prob": "trained",
                "log_prob": "trained", "evaluate": "trained", "fit_weights": "trained", "score": "trained", "responsibilities": "trained"},
    "image": {"sample": "trained", "evaluate": "trained", "fit_weights": "trained", "numerics_status": "all",
              "component_log_prob": "all", "log_prob": "all", "graphed_log_prob": "all", "score": "all", "responsibilities": "all",
              "component_class_log_prob": "all", "class_log_prob": "all"},
}


class _Asked(Exception):
    pass


def _call(m, family, method):
    x = torch.zeros((2, 4) if family == "tabular" else (2, 1, 4, 4))
    if method in ("evaluate", "fit_weights"):
        return getattr(m, method)([(x, None)])
    if method == "sample":
        return m.sample(2)
    if method == "numerics_status":
        return m.numerics_status()
    if method == "graphed_log_prob":
        return m.graphed_log_prob(2)
    if method == "mixture_training_step":
        return m.mixture_training_step(x, lr=0.1)
    return getattr(m, method)(x)


@pytest.mark.parametrize("family,method", [(f, k) for f in sorted(N_USED_DEFAULT) for k in sorted(N_USED_DEFAULT[f])])
def test_every_call_site_asks_n_used_with_its_default(family, method):
    m = FAMILIES[family]() if not method.endswith("class_log_prob") else image_model(y_condition=True, y_classes=3)
    asked = []

    def spy(n_used, default="trained"):
        asked.append((n_used, default))
        raise _Asked()

    m._n_used = spy
    m._require_device = lambda t: None           # (the tabular module looks at the device first)
    with pytest.raises(_Asked):
        _call(m, family, method)
    assert asked == [(None, N_USED_DEFAULT[family][method])]


@pytest.mark.parametrize("family", sorted(FAMILIES))
def test_n_used_defaults_and_range(family):
    m = FAMILIES[family]()
    assert m.num_components == 3
    assert (m._n_used(None), m._n_used(None, "trained"), m._n_used(None, "all")) == (1, 1, 3)
    m.increment_component()
    assert (m.component, m._n_used(None), m._n_used(None, "all")) == (1, 2, 3)
    m.increment_component()
    m.increment_component()
    assert m.all_trained and m.component == 0
    assert (m._n_used(None), m._n_used(None, "all")) == (3, 3)
    assert m._n_used(2) == 2 and m._n_used(2, "all") == 2 and m._n_used(np.int64(3)) == 3
    for bad in (0, 4):
        for default in ("trained", "all"):
            with pytest.raises(ValueError, match=rf"n_used={bad} outside \[1, 3\]"):
                m._n_used(bad, default)
    with pytest.raises(ValueError):
        m._n_used(None, "some")


@pytest.mark.parametrize("method", ["numerics_status", "component_log_prob", "log_prob", "graphed_log_prob", "class_log_prob",
                                    "component_class_log_prob"])
def test_out_of_range_n_used_is_refused_before_device_work(method):
    """The image sites that checked no range: a ValueError now, where an IndexError on flows[c] or a torch error came out."""
    m = image_model(y_condition=True, y_classes=3) if "class" in method else image_model()
    x = torch.zeros(2, 1, 4, 4)
    calls = {"numerics_status": lambda n: m.numerics_status(n), "graphed_log_prob": lambda n: m.graphed_log_prob(2, n)}
    call = calls.get(method) or (lambda n: getattr(m, method)(x, n))
    for bad in (0, 4):
        with pytest.raises(ValueError, match=rf"n_used={bad} outside \[1, 3\]"):
            call(bad)


def test_sample_component_draws_alike_in_both_modules():
    t, i = tabular_model(), image_model()
    assert torch.equal(t.rho, i.rho)
    for m in (t, i):
        m.component = 2
        assert m._sample_component("c") == 2
        with pytest.raises(ValueError, match="z_k can only be sampled from .*'new', 'fixed'"):
            m._sample_component("2:c")
    for form, allowed in (("1:c", {0, 1, 2}), ("1:c-1", {0, 1}), ("-c", {0, 1})):
        draws = []
        for m in (t, i):
            torch.manual_seed(5)
            draws.append([m._sample_component(form) for _ in range(12)])
        assert draws[0] == draws[1] and set(draws[0]) <= allowed
        assert len(set(draws[0])) > 1, "twelve draws hit one component: the draw does not look at rho"
    for m in (t, i):                                    # "1:c" reaches every component once all are trained
        m.component, m.all_trained = 0, True
        torch.manual_seed(5)
        assert max(m._sample_component("1:c") for _ in range(40)) == 2


def test_cycle_restarts_the_loader():
    m = tabular_model()
    loader = [("b0", 0), ("b1", 1)]
    assert [b[0] for b in itertools.islice(m._cycle(loader), 5)] == ["b0", "b1", "b0", "b1", "b0"]
    assert list(m._cycle([])) == []


def _run_rho_loop(m, difs):
    """``_rho_loop`` on scripted statistics: -> the (batch, step size) of every call."""
    calls = []

    def step_fn(x, y, step_size):
        calls.append((x, step_size))
        return torch.tensor([0.0, 0.0, 0.0, difs[len(calls) - 1]])

    version = m.rho._version
    m._rho_loop([("b0", None), ("b1", None)], step_fn)
    assert m.rho._version == version + len(calls)       # one increment_version([rho]) per iteration
    return calls


@pytest.mark.parametrize("family", sorted(FAMILIES))
def test_rho_loop_stop_rule_and_step_sizes(family):
    tol, min_iters = boost_host.TOLERANCE, boost_host.MIN_ITERS
    m = FAMILIES[family]()
    iters, lr = m.args.rho_iters, m.args.rho_lr
    assert iters == 40
    small, large = tol / 2, 2 * tol
    # small from the first iteration on: the reference cannot stop before batch_id = min_iters + 1
    calls = _run_rho_loop(m, [small] * iters)
    assert len(calls) == min_iters + 2
    # the first later iteration whose dif is below the tolerance (dif == tolerance does not stop)
    calls = _run_rho_loop(m, [large] * 20 + [tol] + [small] * iters)
    assert len(calls) == 22
    # never below: rho_iters iterations
    calls = _run_rho_loop(m, [large] * iters)
    assert len(calls) == iters
    assert [s for _, s in calls] == [lr / (0.05 * k + 1) for k in range(iters)]
    assert [b for b, _ in calls] == ["b0", "b1"] * (iters // 2)
    m.args.rho_iters = 5                                 # fewer than min_iters: all of them
    assert len(_run_rho_loop(m, [small] * 5)) == 5


@pytest.mark.parametrize("family", sorted(FAMILIES))
def test_mixture_recursion_against_float64(family):
    """The un-normalised recursion on a (3, 7) table against ``fixed_ll64`` of tests/test_image_boost_host.py, at that file's tolerance
    for the quantity (1e-15 absolute on float64 inputs of magnitude <= 2: 4 ulp), and on the float32 the modules run in."""
    m = FAMILIES[family]()
    rng = np.random.default_rng(3)
    ll = -rng.random((3, 7))
    rho = np.array([1.0, 0.5, 0.25])
    for dtype, atol in ((torch.float64, 1e-15), (torch.float32, 8 * 2.0 ** -24 * 2.0)):     # f32: 8 roundings of values below 2
        m.rho = torch.tensor(rho, dtype=dtype)
        table = torch.tensor(ll, dtype=dtype)
        ref = table.double().numpy()
        for component in (0, 1, 2):
            m.component = component
            new_ll, fixed_ll, full_ll = m._mixture_recursion(table[: component + 1].unbind(0))
            assert new_ll.dtype == dtype and new_ll.shape == (7,)
            zero = np.zeros(7)
            assert np.array_equal(new_ll.numpy(), ref[component] if component else zero)
            assert np.allclose(full_ll.double().numpy(), boost_host.fixed_ll64(ref, rho, component + 1), rtol=0, atol=atol)
            want_fixed = boost_host.fixed_ll64(ref, rho, component) if component else zero
            assert np.allclose(fixed_ll.double().numpy(), want_fixed, rtol=0, atol=atol)
    m.component = 2                                      # a generator is consumed once, column by column
    assert len(m._mixture_recursion(t for t in table.unbind(0))) == 3


class _Dataset(list):
    pass


class _Loader(list):
    """A list of batches, with a ``dataset`` of ``rows`` entries when given."""

    def __init__(self, batches, rows=None):
        super().__init__(batches)
        if rows is not None:
            self.dataset = _Dataset(range(rows))


@pytest.mark.parametrize("family", sorted(FAMILIES))
def test_fit_weights_skeleton(family, monkeypatch):
    m = FAMILIES[family]()
    m._require_device = lambda t: None
    seen = {}

    def on_table(table, rho, n_used, max_iters, tol, write):
        seen.update(table=table.clone(), rho=rho, args=(n_used, max_iters, tol, write))
        return "report"

    monkeypatch.setattr(native, "fit_weights_on_table", on_table)
    hook_calls = []

    def batch_table(x, y, table, filled):
        """Row c of a batch's piece: the batch's first column + 10 c."""
        hook_calls.append((x.shape[0], y, None if table is None else tuple(table.shape), filled))
        piece = torch.stack([x[:, 0] + 10.0 * c for c in range(2)])
        if table is None:
            return piece
        table[:, filled:filled + x.shape[0]].copy_(piece)

    rows = [torch.arange(0.0, 3.0), torch.arange(3.0, 3.0), torch.arange(3.0, 5.0)]          # 3 rows, an empty batch, 2 rows
    batches = [(r.view(-1, 1).repeat(1, 4).double(), k) for k, r in enumerate(rows)]
    want = torch.stack([torch.arange(0.0, 5.0), torch.arange(0.0, 5.0) + 10.0])
    # with a dataset: one table of len(dataset) columns, every batch at its offset
    assert m._fit_weights_over(_Loader(batches, rows=5), 2, batch_table, 7, 1e-3, False) == "report"
    assert hook_calls == [(3, 0, (2, 5), 0), (2, 2, (2, 5), 3)]
    assert seen["table"].shape == (2, 5) and torch.equal(seen["table"], want) and seen["table"].dtype == torch.float32
    assert seen["rho"] is m.rho and seen["args"] == (2, 7, 1e-3, False)
    # without one: the pieces, concatenated
    del hook_calls[:]
    m._fit_weights_over(_Loader(batches), 2, batch_table, 7, 1e-3, True)
    assert hook_calls == [(3, 0, None, 0), (2, 2, None, 3)]
    assert torch.equal(seen["table"], want) and seen["args"] == (2, 7, 1e-3, True)
    # a dataset that undercounts: the table grows, nothing is lost
    m._fit_weights_over(_Loader(batches, rows=2), 2, batch_table, 7, 1e-3, False)
    assert torch.equal(seen["table"], want)
    for empty in (_Loader([]), _Loader([batches[1]]), _Loader([], rows=4)):
        with pytest.raises(ValueError, match="fit_weights: the loader yielded no rows"):
            m._fit_weights_over(empty, 2, batch_table, 7, 1e-3, False)
    with pytest.raises(ValueError, match=rf"fit_weights handles up to {native.WEIGHTS_MAX_COMPONENTS} components"):
        m._fit_weights_over(_Loader(batches), native.WEIGHTS_MAX_COMPONENTS + 1, batch_table, 7, 1e-3, False)
    with pytest.raises(ValueError, match=r"n_used=4 outside \[1, 3\]"):          # (the range is the public method's check)
        m.fit_weights(_Loader(batches), n_used=4)
    m.rho = m.rho.double()
    with pytest.raises(ValueError, match="fit_weights reads .* self.rho in place: it must be contiguous float32"):
        m._fit_weights_over(_Loader(batches), 2, batch_table, 7, 1e-3, False)


def test_small_shared_helpers():
    t, i = tabular_model(), image_model()
    for m in (t, i):
        with pytest.raises(native.GbnfError, match="x must live on the MI355X"):
            m._require_device(torch.zeros(2))
        with pytest.raises(native.GbnfError):
            m._require_device(None)
        rho = m.rho[:2].double()
        assert torch.equal(m._log_w(2), torch.log(m.rho[:2] / m.rho[:2].sum())) and m._log_w(2).dtype == torch.float32
        assert abs(float(torch.exp(m._log_w(2)).sum()) - 1.0) < 1e-6 and rho.numel() == 2
        assert m._rho_in_place("a call writes") is m.rho
        assert m._check_component(np.int64(2)) == 2
        for bad in (-1, 3):
            with pytest.raises(ValueError, match=rf"c={bad} is no component of this model \(0 .. 2\)"):
                m._check_component(bad)
        g, G, r = torch.zeros(2, 4), torch.ones(2), torch.zeros(3, 2)
        assert m._score_result(g, G, r, False, False) is g
        out = m._score_result(g, G, r, True, True)
        assert out[0] is g and out[1] is G and out[2].shape == (2, 3)
        assert m._score_result(g, G, r, False, True)[1].shape == (2, 3) and m._score_result(g, G, None, True, False)[1] is G
        with pytest.raises(ValueError, match="evaluate: the loader yielded no rows"):
            m._eval_sums(None)
        with pytest.raises(ValueError, match="evaluate: the loader yielded no rows"):
            m._eval_sums(torch.zeros(native.EVAL_STATE_DOUBLES, dtype=torch.float64))
        state = torch.arange(1.0, native.EVAL_STATE_DOUBLES + 1.0, dtype=torch.float64)
        sums = m._eval_sums(state)
        assert sums == {name: float(k + 1) for name, k in native.EVAL_STATE.items()}
        # .to() drops every cache the class lists
        for name in m._CACHES:
            m.__dict__[name] = {"stale": 1}
        m.to(CPU)
        m.float()
        assert not any(name in m.__dict__ for name in m._CACHES) and m._CACHES
    t.__dict__["_key_cache"] = {"stale": 1}
    t.load_state_dict(t.state_dict())
    assert "_key_cache" not in t.__dict__


# ---------------------------------------------------------------------------------------------------------------- native
class _FakeLib:
    """Size queries that write through the byref they get last, and destroy calls that are counted."""

    def __init__(self):
        self.queries, self.destroyed = [], []

    def gbnf_trainer_workspace_bytes(self, handle, n, out):
        self.queries.append(("gbnf_trainer_workspace_bytes", handle, n, type(out).__name__))
        out._obj.value = 4096 + n
        return 0

    def gbnf_failing_bytes(self, out):
        return -1

    def gbnf_last_error(self):
        return b"refused"

    def __getattr__(self, name):
        if name.endswith("_destroy"):
            return lambda handle: self.destroyed.append((name, handle.value))
        raise AttributeError(name)


@pytest.fixture
def fake(monkeypatch):
    lib = _FakeLib()
    monkeypatch.setattr(native, "lib", lambda: lib)
    return lib


def test_query_i64_passes_a_byref_last_and_asks_every_time(fake):
    h = C.c_void_p(1)
    assert native._query_i64(fake.gbnf_trainer_workspace_bytes, h, 8) == 4104
    assert native._query_i64(fake.gbnf_trainer_workspace_bytes, h, 9) == 4105
    assert isinstance(native._query_i64(fake.gbnf_trainer_workspace_bytes, h, 8), int)
    assert fake.queries == [("gbnf_trainer_workspace_bytes", h, n, "CArgObject") for n in (8, 9, 8)]
    with pytest.raises(native.GbnfError, match="refused"):
        native._query_i64(fake.gbnf_failing_bytes)


def test_ptr_and_arrays():
    t = torch.zeros(4)
    assert native._ptr(None).value is None and native._ptr(t).value == t.data_ptr()
    arr = native._addr_array([t, None, t[2:]])
    assert list(arr) == [t.data_ptr(), None, t.data_ptr() + 8] and isinstance(arr, C.Array)

    class H:
        def __init__(self, v):
            self.handle = C.c_void_p(v)

    arr = native._handle_array([H(3), H(5)])
    assert list(arr) == [3, 5] and arr._type_ is C.c_void_p


def test_shape_checks(monkeypatch):
    monkeypatch.setattr(native, "_require_device_f32", lambda t, name: t)
    x = torch.zeros(2, 1, 4, 4)
    assert native._check_noise(None, x) is None and native._check_noise(torch.ones(2, 1, 4, 4), x) is None
    with pytest.raises(native.GbnfError, match="^noise must have the shape of x$"):
        native._check_noise(torch.ones(2, 1, 4, 3), x)
    assert native._check_log_w(torch.zeros(3), 3) is None
    for bad in (torch.zeros(2), torch.zeros(3, 1)):
        with pytest.raises(native.GbnfError, match=r"^log_w must be \(3,\), got"):
            native._check_log_w(bad, 3)
    monkeypatch.undo()
    with pytest.raises(native.GbnfError, match="noise must be a tensor on the MI355X"):
        native._check_noise(torch.ones(2, 1, 4, 4), x)                  # (a host tensor: the device check runs first)
    with pytest.raises(native.GbnfError, match="log_w must be a tensor on the MI355X"):
        native._check_log_w(torch.zeros(3), 3)


class _DeviceTensor(torch.Tensor):
    """A host tensor that says it lives on the device (for the checks that only ask)."""
    is_cuda = property(lambda self: True)


def test_workspace_arg():
    asked = []

    def nbytes():
        asked.append(1)
        return 10

    ws = native._workspace_arg(None, nbytes, CPU)
    assert asked == [1] and ws.dtype == torch.float32 and ws.numel() == 3 and ws.device == CPU
    given = torch.zeros(5).as_subclass(_DeviceTensor)
    assert native._workspace_arg(given, nbytes, CPU) is given and asked == [1], "the size was asked for although a workspace was passed"
    assert native._check_workspace(given) is given
    for bad in (torch.zeros(4, 2).as_subclass(_DeviceTensor).t(), "a string", torch.zeros(5)):     # strided; no tensor; a host tensor
        for check in (lambda w: native._workspace_arg(w, nbytes, CPU), native._check_workspace):
            with pytest.raises(native.GbnfError, match="^workspace must be a contiguous device tensor$"):
                check(bad)
    assert asked == [1]


def test_grown_keeps_a_buffer_that_is_large_enough():
    a = native._grown(None, 10, CPU)
    assert a.numel() == 3 and a.dtype == torch.float32
    assert native._grown(a, 12, CPU) is a and native._grown(a, 4, CPU) is a
    b = native._grown(a, 13, CPU)
    assert b is not a and b.numel() == 4
    d = native._grown(None, 10, CPU, torch.float64)
    assert d.numel() == 2 and d.dtype == torch.float64 and native._grown(d, 16, CPU, torch.float64) is d
    assert native._grown(a, 4, torch.device("meta")).device.type == "meta"        # another device: a new buffer


@pytest.mark.parametrize("cls,symbol", [("NativeFlow", "gbnf_flow_destroy"), ("NativeImageFlow", "gbnf_image_flow_destroy"),
                                        ("NativeTrainer", "gbnf_trainer_destroy"), ("NativeImageTrainer", "gbnf_image_trainer_destroy"),
                                        ("NativeMixture", "gbnf_mixture_destroy")])
def test_handle_close_is_idempotent_and_del_is_silent(fake, cls, symbol):
    cls = getattr(native, cls)
    assert issubclass(cls, native._Handle) and cls._destroy == symbol
    obj = cls.__new__(cls)
    obj.handle = C.c_void_p(7)
    obj.close()
    obj.close()
    assert fake.destroyed == [(symbol, 7)] and obj.handle is None
    obj.__del__()
    bare = cls.__new__(cls)                      # no attribute at all, then a null handle: nothing to destroy, nothing raised
    bare.close()
    bare.__del__()
    bare.handle = None
    bare.__del__()
    assert fake.destroyed == [(symbol, 7)]


def test_del_swallows_a_failing_destroy(monkeypatch):
    def broken():
        raise native.GbnfError("no library")

    monkeypatch.setattr(native, "lib", broken)
    obj = native.NativeFlow.__new__(native.NativeFlow)
    obj.handle = C.c_void_p(7)
    obj.__del__()
    obj.handle = None


def test_the_trainers_share_their_base():
    tb = native._TrainerBase
    assert issubclass(native.NativeTrainer, tb) and issubclass(native.NativeImageTrainer, tb) and issubclass(tb, native._Handle)
    assert native.NativeImageTrainer._hyper is native.NativeTrainer._hyper is tb._hyper
    for name in ("key", "deterministic", "_hyper", "apply_update"):
        assert name not in vars(native.NativeTrainer) and name not in vars(native.NativeImageTrainer), f"{name} is written twice again"
    assert (native.NativeTrainer._update_floats, native.NativeImageTrainer._update_floats) == ("grad_floats", "step_grad_floats")

    class State:
        kind, step = "sgd", 4

    h = tb._hyper(None, State(), lr=0.5, betas=(0.8, 0.9), bn_momentum=0.25)
    assert (h.kind, h.step, h.lr, h.beta1, h.bn_momentum) == (native.OPT_KIND["sgd"], 5, 0.5, np.float32(0.8), 0.25)
