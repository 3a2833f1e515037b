"""Host: the all-class density table without a GPU -- the new symbols in header, binding and library; the geometry the cases claim;
the numpy closed forms (tests/image_class_table_cases.py) against the float64 yardstick; the g23 fixture (the reference's own component
under every class) against the yardstick; the module's new methods on an unconditional model and the old refusals."""
import os
import re

import numpy as np
import pytest
import torch

import image_class_table_cases as ict
import image_ycond_oracle as iyo
from test_hip_image_train import LL_RTOL
from test_image_ycond_host import _args

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
NEW_SYMBOLS = {"gbnf_image_flow_forward_classes": 11, "gbnf_class_posterior": 8, "gbnf_image_mixture_rho_step_y": 13}


def test_new_symbols_in_header_binding_and_library():
    import ctypes as C
    from gbnf_amd import native
    hdr = open(os.path.join(ROOT, "include", "gbnf.h")).read()
    L = native.lib()
    for name, n_args in NEW_SYMBOLS.items():
        decl = re.search(r"\bint\s+%s\s*\(([^;]*)\)\s*;" % name, hdr)
        assert decl, f"{name} is not declared in include/gbnf.h"
        assert len(decl.group(1).split(",")) == n_args
        assert name in native.ABI_SYMBOLS, f"{name} is not in native.ABI_SYMBOLS"
        assert hasattr(L, name), f"{name} is not exported by libgbnf_hip.so"
        fn = getattr(L, name)
        assert fn.argtypes is not None and len(fn.argtypes) == n_args and fn.restype is C.c_int
    # the y call is the plain one with one more pointer behind noise; the float is the step size in both
    plain, with_y = L.gbnf_image_mixture_rho_step.argtypes, L.gbnf_image_mixture_rho_step_y.argtypes
    assert list(with_y) == list(plain[:4]) + [C.c_void_p] + list(plain[4:])
    assert L.gbnf_class_posterior.argtypes[2:4] == [C.c_int64, C.c_int32]
    assert L.gbnf_image_flow_forward_classes.argtypes[3] is C.c_int64 and L.gbnf_image_flow_forward_classes.argtypes[9] is C.c_int64
    for attr in ("forward_classes", "rho_step"):
        assert hasattr(native.NativeImageFlow, attr)
    assert callable(native.class_posterior)


def test_case_geometry():
    assert set(ict.CASES) == set(iyo.YC_CASES) | {"W"}
    assert ict.geometry("W") == (2, 70, 4, 256)                  # a 16x16 map: four strides of a wave; 70 classes: past 64, ragged
    assert ict.geometry("G") == (2, 256, 64, 4)                  # the widest top latent and the most classes the handle takes
    assert ict.geometry("g22") == (3, 10, 8, 16)
    assert ict.geometry("S1")[:2] == (1, 1) and ict.geometry("S70")[0] == 70
    assert len(ict.CASES["D"][1]) == 3 and ict.CASES["D"][1]["L"] == 3
    for name in ict.CASES:
        sp, x, noise = ict.make_case(name)
        n, Y, Cz, _ = ict.geometry(name)
        assert x.shape[0] == n and np.asarray(sp["ycond"]["cond_w"]).shape == (2 * Cz, Y), name


def test_closed_forms_against_the_yardstick():
    """np_table on the yardstick's z and ldj with the priors of np_prior equals the per-class forwards (g22: 10 of them); the handle's
    float32 top prior moves it by less than the bar; np_posterior and np_mixture against torch."""
    sp, x, noise, out = ict.yardstick("g22")
    assert out["table"].shape == (3, 10)
    closed = ict.np_table(out["z"], out["ldj"], ict.class_priors(sp))
    assert np.abs(closed - out["table"]).max() <= 1e-12 * np.abs(out["table"]).max()
    packed = ict.np_table(out["z"], out["ldj"], ict.class_priors(sp, ict.handle_top_h(sp)))
    assert 0.0 < np.abs(packed - out["table"]).max() <= 0.01 * LL_RTOL * np.abs(out["table"]).max()
    # the row under the case's own labels is image_ycond_oracle's ll
    _, _, _, y = iyo.make_case("g22")
    with torch.no_grad():
        ll = iyo.forward(sp, iyo.leaf_params(sp), x, noise, y)["ll"].numpy()
    assert np.array_equal(out["table"][np.arange(3), iyo.target(y)], ll)
    rng = np.random.RandomState(0)
    t = rng.randn(4, 7) * 1e3
    t[1, 2] = -np.inf
    t[3] = -np.inf
    prior = rng.dirichlet(np.ones(7))
    for lp in (None, np.log(prior)):
        lpx, post = ict.np_posterior(t, lp)
        a = torch.from_numpy(t) + torch.from_numpy(np.full(7, -np.log(7.0)) if lp is None else lp)
        want = torch.logsumexp(a, dim=1).numpy()
        assert np.allclose(lpx[:3], want[:3], rtol=1e-14, atol=0) and lpx[3] == -np.inf == want[3]
        assert np.isnan(post[3]).all() and post[1, 2] == -np.inf
        assert np.abs(np.exp(post[:3]).sum(axis=1) - 1.0).max() <= 1e-12
    tabs = rng.randn(3, 5, 2) * 10
    rho = np.array([1.0, 0.5, 0.25])
    G = ict.np_mixture(tabs, rho)
    r1, r2 = 0.5 / 1.5, 0.25 / 1.75
    want = np.log((1 - r2) * ((1 - r1) * np.exp(tabs[0]) + r1 * np.exp(tabs[1])) + r2 * np.exp(tabs[2]))
    assert np.allclose(G, want, rtol=1e-12, atol=0)


def test_the_large_case_restates_the_prior():
    """G (256 classes) takes the numpy route: on three of its classes it equals the per-class forward."""
    sp, x, noise, out = ict.yardstick("G")
    assert out["table"].shape == (2, 256) and np.isfinite(out["table"]).all()
    P = iyo.leaf_params(sp)
    eye = np.eye(256, dtype=np.float32)
    with torch.no_grad():
        for k in (0, 64, 255):
            ll = iyo.forward(sp, P, x, noise, np.repeat(eye[k:k + 1], 2, axis=0))["ll"].numpy()
            assert np.abs(out["table"][:, k] - ll).max() <= 1e-12 * np.abs(ll).max()
    assert np.abs(out["table"][:, 0] - out["table"][:, 1]).min() > 0.0        # the class moves the density


def test_g23_fixture_against_the_yardstick():
    """The reference's own component under every class (float32 CPU) against the float64 yardstick on the same parameters: LL_RTOL."""
    ref = ict.g23_load()
    cfg, data = iyo.g22_load(iyo.G22[0])
    assert ref.shape == (data["x"].shape[0], cfg["Y"]) and np.isfinite(ref).all()
    from gbnf_amd import image_glow
    glow = iyo.g22_module(cfg, data, torch.device("cpu")).flows[0]
    sp = image_glow.image_spec_from_glow_module(glow)
    P = iyo.leaf_params(sp)
    eye = np.eye(cfg["Y"], dtype=np.float32)
    n = ref.shape[0]
    with torch.no_grad():
        mine = np.stack([iyo.forward(sp, P, data["x"], data["noise"], np.repeat(eye[k:k + 1], n, axis=0))["ll"].numpy()
                         for k in range(cfg["Y"])], axis=1)
    err = float((np.abs(mine - ref) / np.abs(ref)).max())
    print(f"g23 against the yardstick: {err:.3e}")
    assert err < LL_RTOL
    t = iyo.target(data["y"])
    assert abs(float(-ref[np.arange(n), t].mean()) - float(data["nll"])) <= 1e-6 * abs(float(data["nll"]))
    assert np.abs(ref[:, 0] - ref[:, 1]).min() > 0.0


def test_new_methods_need_a_conditional_model():
    from gbnf_amd import BoostedFlow
    plain = BoostedFlow(_args(y_condition=False, Y=0))
    x = torch.zeros(2, 1, 16, 16)
    for call in (lambda: plain.component_class_log_prob(x), lambda: plain.class_log_prob(x), lambda: plain.marginal_log_prob(x),
                 lambda: plain.class_posterior(x), lambda: plain.predict(x), lambda: plain.update_rho([], labels=True),
                 lambda: plain.graphed_log_prob(4, labels=True)):
        with pytest.raises(ValueError, match="class-conditional"):
            call()


def test_old_refusals_hold_without_the_keyword():
    from gbnf_amd import BoostedFlow
    m = BoostedFlow(_args())
    m.component, m.all_trained, m.args.rho_iters = 0, True, 3
    for call in (lambda: m.update_rho([]), lambda: m.graphed_log_prob(4), lambda: m.update_rho([], labels=False),
                 lambda: m.graphed_log_prob(4, labels=False)):
        with pytest.raises(NotImplementedError, match="class-conditional"):
            call()
    x = torch.zeros(2, 1, 16, 16)
    for call in (lambda: m.log_prob(x), lambda: m.component_log_prob(x)):
        with pytest.raises(ValueError, match="y_onehot"):
            call()
