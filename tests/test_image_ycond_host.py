"""Host: the class-conditional image path without a GPU -- the new symbols in header, binding and library; the yardstick
(tests/image_ycond_oracle.py) against the reference's own class-conditional component (fixtures g22), against its closed forms and
against finite differences; the module's construction, names, spec round trip and refusals."""
import argparse
import math
import os
import pickle
import re

import numpy as np
import pytest
import torch

import image_grad_oracle as igo
import image_ycond_oracle as iyo

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
NEW_SYMBOLS = ("gbnf_image_flow_set_ycond", "gbnf_image_flow_y_classes", "gbnf_image_flow_forward_y", "gbnf_image_flow_prior_y",
               "gbnf_image_trainer_bind_ycond", "gbnf_image_trainer_y_classes", "gbnf_image_trainer_nll_step_y",
               "gbnf_image_boosted_step_workspace_bytes_y", "gbnf_image_boosted_nll_step_y")


def test_new_symbols_in_header_binding_and_library():
    from gbnf_amd import native
    hdr = open(os.path.join(ROOT, "include", "gbnf.h")).read()
    for name in NEW_SYMBOLS:
        assert re.search(r"\bint\s+%s\s*\(" % name, hdr), f"{name} is not declared in include/gbnf.h"
        assert name in native.ABI_SYMBOLS, f"{name} is not in native.ABI_SYMBOLS"
    assert re.search(r"#define\s+GBNF_ABI_VERSION\s+4\b", hdr)
    L = native.lib()
    for name in NEW_SYMBOLS:
        assert hasattr(L, name), f"{name} is not exported by libgbnf_hip.so"
        assert getattr(L, name).argtypes is not None, f"{name} has no argtypes"
    assert L.gbnf_version() == 4
    for attr in ("bind_ycond", "YCOND_KEYS"):
        assert hasattr(native.NativeImageTrainer, attr)
    for attr in ("set_ycond", "prior_y"):
        assert hasattr(native.NativeImageFlow, attr)


# ---- the yardstick ------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("name", iyo.G22)
def test_yardstick_matches_the_reference(name):
    """float64 yardstick against the reference's f32 CPU autograd of bpd + 0.01 cross_entropy at component level (fixtures g22): nll
    1e-6 relative, logits and class loss 1e-5, each gradient 1e-5 of its tensor's largest entry (the bars g21 is held to)."""
    cfg, data = iyo.g22_load(name)
    m = iyo.g22_module(cfg, data, torch.device("cpu"))
    k = 1.0 / (math.log(2.0) * float(np.prod(cfg["input_size"])))
    out, grads = iyo.module_yardstick(m.flows[0], data["x"], data["noise"], data["y"], k=k, y_weight=cfg["y_weight"])
    assert abs(out["nll"] - float(data["nll"])) <= 1e-6 * abs(out["nll"])
    assert abs(out["loss_classes"] - float(data["loss_classes"])) <= 1e-5 * abs(float(data["loss_classes"]))
    assert abs(out["total"] - float(data["total"])) <= 1e-5 * abs(float(data["total"]))
    lg = data["y_logits"]
    assert np.abs(out["y_logits"].numpy() - lg).max() <= 1e-5 * float(np.abs(lg).max())
    Cz = data["z"].shape[1]
    for key, mine in (("z_mu", out["z_mu"]), ("z_var", out["z_var"])):
        ref = data[key]
        assert ref.shape == data["z"].shape
        assert np.abs(mine.numpy().reshape(-1, Cz, 1, 1) - ref).max() <= 1e-6 * max(1.0, float(np.abs(ref).max())), key
    assert np.abs(out["z"].numpy() - data["z"]).max() <= 1e-5 * float(np.abs(data["z"]).max())
    ref = {k_[len("grad."):]: data[k_] for k_ in data.files if k_.startswith("grad.")}
    assert set(grads) == set(ref)
    assert all(nm in ref for nm in iyo.YCOND_NAMES.values())
    for k_, b in ref.items():
        a = grads[k_].reshape(b.shape)
        assert np.abs(a - b).max() <= 1e-5 * float(np.abs(b).max()), (k_, float(np.abs(a - b).max()), float(np.abs(b).max()))


def test_fixture_cases_are_what_the_issue_lists():
    cfgs = {name: iyo.g22_load(name) for name in iyo.G22}
    a, b, c = (cfgs[n] for n in iyo.G22)
    assert (a[0]["Y"], a[0]["N"], a[0]["LU"], a[0]["coupling"], a[0]["learn_top"]) == (10, 3, False, "affine", True)
    assert (b[0]["Y"], b[0]["LU"]) == (10, True)
    assert (c[0]["Y"], c[0]["N"], c[0]["coupling"], c[0]["permutation"], c[0]["learn_top"], c[0]["depth"]) == (3, 5, "additive", "shuffle", False, 2)
    y = c[1]["y"]
    t = np.argmax(y, axis=1)
    assert len(set(t.tolist())) < len(t), "a class repeats"
    soft = [i for i in range(len(y)) if not np.isin(y[i], (0.0, 1.0)).all()]
    assert len(soft) == 1 and np.sort(y[soft[0]])[-1] > np.sort(y[soft[0]])[-2], "one soft row, no tie"


@pytest.mark.parametrize("name", sorted(iyo.YC_CASES))
def test_cases_are_clear_of_the_kink_margin(name):
    sp, x, noise, _ = iyo.make_case(name)
    rows = igo.kink_report(sp, x, noise)
    assert rows and [inside for inside, _ in rows] == [0] * len(rows)


@pytest.mark.parametrize("name,k,yw", [("g22", 0.0056, 0.01), ("S70", 1.0, 0.5), ("S1", 1.0, 0.01)])
def test_closed_forms_match_autograd(name, k, yw):
    """The numpy closed forms of the new gradients against the yardstick's own autograd, to float64 rounding."""
    sp, x, noise, y = iyo.make_case(name)
    out, g = iyo.yardstick(sp, x, noise, y, k=k, y_weight=yw)
    top = None if sp["learn_top"] is None else (sp["learn_top"]["b"], sp["learn_top"]["logs"])
    cf = iyo.np_ycond(out["z"].numpy(), out["ldj"].numpy(), top, sp["ycond"], y, k=k, y_weight=yw)
    close = lambda a, b, what: np.testing.assert_allclose(a, b, rtol=1e-9, atol=1e-12 * max(1.0, float(np.abs(b).max())), err_msg=what)
    close(cf["ll"], out["ll"].numpy(), "ll")
    close(cf["y_logits"], out["y_logits"].numpy(), "y_logits")
    assert abs(cf["nll"] - out["nll"]) <= 1e-12 * abs(out["nll"]) and abs(cf["loss_classes"] - out["loss_classes"]) <= 1e-12
    assert cf["correct"] == int(out["correct"])
    for key in iyo.YCOND_KEYS:
        close(cf[key], g[("ycond", key)], key)
    if top is not None:
        close(cf["top_b"], g[("learn_top", "b")], "top_b")
        close(cf["top_logs"], g[("learn_top", "logs")], "top_logs")
        assert np.abs(g[("learn_top", "w")]).max() == 0.0
    # the seed: autograd of total with respect to z and ldj
    P = iyo.leaf_params(sp)
    o = iyo.forward(sp, P, x, noise, y)
    o["z"].retain_grad(); o["ldj"].retain_grad()
    (k * o["nll_i"].mean() + yw * o["ce_i"].mean()).backward()
    close(cf["g_z"], o["z"].grad.numpy(), "g_z")
    close(cf["g_ldj"], o["ldj"].grad.numpy(), "g_ldj")


def test_yardstick_gradients_match_finite_differences():
    sp, x, noise, y = iyo.make_case("S70")
    k, yw = 0.7, 0.3
    _, g = iyo.yardstick(sp, x, noise, y, k=k, y_weight=yw)
    rng = np.random.RandomState(3)
    paths = [("ycond", key) for key in iyo.YCOND_KEYS] + [("learn_top", "b"), ("learn_top", "logs")]
    for path in paths:
        idx = tuple(int(rng.randint(0, d)) for d in g[path].shape)
        vals = []
        for sgn in (1.0, -1.0):
            P = iyo.leaf_params(sp)
            with torch.no_grad():
                P[path][idx] += sgn * 1e-6
                o = iyo.forward(sp, P, x, noise, y)
                vals.append(float(k * o["nll_i"].mean() + yw * o["ce_i"].mean()))
        fd = (vals[0] - vals[1]) / 2e-6
        assert abs(fd - g[path][idx]) <= 1e-5 * max(1.0, abs(fd)), (path, fd, g[path][idx])


def test_ll_moves_with_y_and_ties_take_the_lowest_index():
    sp, x, noise, y = iyo.make_case("g22")
    with torch.no_grad():
        a = iyo.forward(sp, iyo.leaf_params(sp), x, noise, y)["ll"].numpy()
        b = iyo.forward(sp, iyo.leaf_params(sp), x, noise, np.roll(y, 1, axis=1))["ll"].numpy()
    assert np.abs(a - b).min() > 1e-3
    assert iyo.target(np.array([[0.5, 0.5, 0.0], [0.0, 1.0, 1.0]])).tolist() == [0, 1]


# ---- synth, spec, module ----------------------------------------------------------------------------------------------------------
def test_synth_is_unchanged_without_classes():
    from gbnf_amd import synth
    kw = dict(input_size=(1, 16, 16), h=32, K=2, L=2, seed=3)
    a, b, c = synth.synth_image_glow_spec(**kw), synth.synth_image_glow_spec(y_classes=0, **kw), synth.synth_image_glow_spec(y_classes=10, **kw)
    assert "ycond" not in a and pickle.dumps(a) == pickle.dumps(b)
    yc = c.pop("ycond")
    assert pickle.dumps(a) == pickle.dumps(c), "the rest of a spec does not depend on the conditioning"
    Cz = 8
    assert {k: v.shape for k, v in yc.items()} == {"cond_w": (2 * Cz, 10), "cond_b": (2 * Cz,), "cond_logs": (2 * Cz,),
                                                    "class_w": (10, Cz), "class_b": (10,), "class_logs": (10,)}
    assert all(v.dtype == np.float32 and np.abs(v).min() > 0 for v in yc.values()), "LinearZeros at zero would test nothing"


def _args(y_condition=True, Y=10, **kw):
    base = dict(num_flows=2, z_size=256, density_evaluation=True, device=torch.device("cpu"), cuda=False, component_type="glow",
                num_components=1, rho_init="decreasing", learn_top=True, y_classes=Y, y_condition=y_condition, sample_size=4,
                input_size=[1, 16, 16], h_size=32, num_blocks=2, actnorm_scale=1.0, flow_permutation="invconv", flow_coupling="affine",
                LU_decomposed=False, num_dequant_blocks=0, coupling_network="tanh", coupling_network_depth=1, batch_norm=False)
    base.update(kw)
    return argparse.Namespace(**base)


def test_construction_names_and_state_dict():
    """ImageGlow(y_condition=True) builds project_ycond / project_class as LinearZeros under the reference's names: the parameter names
    equal a fixture's state-dict keys and the fixture loads."""
    from gbnf_amd import BoostedFlow, image_glow
    m = BoostedFlow(_args())
    glow = m.flows[0]
    assert glow.y_condition and isinstance(glow.project_ycond, image_glow.LinearZeros) and isinstance(glow.project_class, image_glow.LinearZeros)
    assert tuple(glow.project_ycond.linear.weight.shape) == (16, 10) and tuple(glow.project_class.linear.weight.shape) == (10, 8)
    assert all(float(p.abs().max()) == 0.0 for p in list(glow.project_ycond.parameters()) + list(glow.project_class.parameters()))
    cfg, data = iyo.g22_load(iyo.G22[0])
    keys = {k[len("param."):] for k in data.files if k.startswith("param.")}
    assert set(glow.state_dict().keys()) == keys
    assert {n for n, _ in glow.named_parameters()} == {k[len("grad."):] for k in data.files if k.startswith("grad.")}
    for name in iyo.G22:
        cfg, data = iyo.g22_load(name)
        g = iyo.g22_module(cfg, data, torch.device("cpu")).flows[0]
        for key, nm in iyo.YCOND_NAMES.items():
            assert np.array_equal(g.state_dict()[nm].numpy(), data["param." + nm]) and np.abs(data["param." + nm]).max() > 0
    # an unconditional model has none of this
    plain = BoostedFlow(_args(y_condition=False, Y=0)).flows[0]
    assert not plain.y_condition and not hasattr(plain, "project_ycond")
    with pytest.raises(NotImplementedError):
        BoostedFlow(_args(Y=257))


def test_spec_round_trip():
    from gbnf_amd import BoostedFlow, image_glow
    cfg, data = iyo.g22_load(iyo.G22[0])
    glow = iyo.g22_module(cfg, data, torch.device("cpu")).flows[0]
    sp = image_glow.image_spec_from_glow_module(glow)
    assert set(sp["ycond"]) == set(iyo.YCOND_KEYS)
    for key, nm in iyo.YCOND_NAMES.items():
        assert np.array_equal(sp["ycond"][key], data["param." + nm])
    other = BoostedFlow(_args()).flows[0]
    image_glow.load_image_spec(other, sp)
    back = image_glow.image_spec_from_glow_module(other)
    for key in iyo.YCOND_KEYS:
        assert np.array_equal(back["ycond"][key], sp["ycond"][key])
    assert np.array_equal(back["learn_top"]["b"], sp["learn_top"]["b"])
    # an unconditional module's spec has no entry, and the two kinds do not mix
    plain = BoostedFlow(_args(y_condition=False, Y=0)).flows[0]
    with pytest.raises(ValueError):
        image_glow.load_image_spec(plain, sp)
    plain.set_actnorm_init()
    assert "ycond" not in image_glow.image_spec_from_glow_module(plain)


def test_y_onehot_none_is_refused():
    from gbnf_amd import BoostedFlow
    m = BoostedFlow(_args())
    with pytest.raises(ValueError, match="y_onehot"):
        m._y(0, None)
    for call in (lambda: m.update_rho([]), lambda: m.graphed_log_prob(4)):
        m.component, m.all_trained, m.args.rho_iters = 0, True, 3
        with pytest.raises(NotImplementedError, match="class-conditional"):
            call()
    # an unconditional model ignores the argument, as before
    plain = BoostedFlow(_args(y_condition=False, Y=0))
    assert plain._y(0, None) is None and plain._y(0, torch.zeros(2, 3)) is None


def test_tabular_y_condition_is_still_refused():
    from gbnf_amd import BoostedFlow
    a = _args(input_size=[21], z_size=21, num_blocks=1)
    with pytest.raises(NotImplementedError):
        BoostedFlow(a)
