"""CPU: boosting for image components (csrc/gbnf_image_boost.hip, BoostedImageFlow.update_rho / permutation_state) as far as it goes
without a device -- exports, argument validation, the float64 numpy replay of the ``update_rho`` loop that tests/test_hip_image_boost.py
compares the module with, and the checkpoint round trip of the shuffles and ActNorm flags."""
import argparse
import ctypes as C
import os
import re

import numpy as np

from gbnf_amd import native

REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
IMAGE_BOOST_SYMBOLS = ("gbnf_image_rho_step_workspace_bytes", "gbnf_image_mixture_rho_step",
                       "gbnf_image_boosted_step_workspace_bytes", "gbnf_image_boosted_nll_step")
TOLERANCE, MIN_ITERS = 0.001, 10        # models/boosted_flow.py:158-160


def fixed_ll64(ll, rho, component):
    """models/boosted_flow.py:124-137 in float64 on a (component + 1, n) table: the un-normalised recursion up to component - 1."""
    ll = np.asarray(ll, dtype=np.float64)
    rho = np.asarray(rho, dtype=np.float64)
    fixed = ll[0]
    with np.errstate(invalid="ignore", divide="ignore"):
        for c in range(1, component):
            fixed = np.logaddexp(np.log(1.0 - rho[c]) + fixed, np.log(rho[c]) + ll[c])
    return fixed


def grad64(ll, rho, component):
    """grad = mean(fixed_ll - new_ll), :184."""
    return float(np.mean(fixed_ll64(ll, rho, component) - np.asarray(ll, dtype=np.float64)[component]))


def replay_update_rho(tables, rho0, component, rho_lr, rho_iters):
    """The loop of models/boosted_flow.py:141-207 (approximate branch) in float64.  ``tables``: one (component + 1, n) log-likelihood
    table per batch of the loader, in loader order (the loop starts the loader again when it runs out).
    -> dict(rho = the final rho[component], iters, grads, steps, difs: one entry per iteration)."""
    rho = np.asarray(rho0, dtype=np.float64).copy()
    prev = float(rho[component])
    out = {"grads": [], "steps": [], "difs": [], "rhos": []}
    for batch_id in range(rho_iters):
        g = grad64(tables[batch_id % len(tables)], rho, component)
        step = rho_lr / (0.05 * batch_id + 1)
        new = min(max(prev - step * g, 0.01), 100.0)
        dif = abs(prev - new)
        prev = rho[component] = new
        for key, v in (("grads", g), ("steps", step), ("difs", dif), ("rhos", new)):
            out[key].append(v)
        if batch_id > MIN_ITERS and (batch_id > rho_iters or dif < TOLERANCE):
            break
    out["rho"], out["iters"] = prev, len(out["grads"])
    return out


def image_args(input_size, h, K, L, dev, C_=1, permutation="invconv", depth=1, **extra):
    """The reference's argument namespace for a boosted image Glow of C_ components."""
    ns = argparse.Namespace(
        num_flows=K, z_size=int(np.prod(input_size)), density_evaluation=True, device=dev, cuda=str(dev) != "cpu", component_type="glow",
        num_components=C_, rho_init="decreasing", learn_top=True, y_classes=0, y_condition=False, sample_size=4,
        input_size=list(input_size), h_size=h, num_blocks=L, actnorm_scale=1.0, flow_permutation=permutation, flow_coupling="affine",
        LU_decomposed=False, num_dequant_blocks=0, coupling_network="tanh", coupling_network_depth=depth, batch_norm=False,
        boosted=True, rho_iters=12, rho_lr=0.05)
    for k, v in extra.items():
        setattr(ns, k, v)
    return ns


def test_new_symbols_are_declared_bound_and_exported():
    text = open(os.path.join(REPO, "include", "gbnf.h")).read()
    text = re.sub(r"/\*.*?\*/", "", text, flags=re.S)
    declared = set(re.findall(r"\b(gbnf_[a-z_]+)\s*\(", text))
    L = native.lib()
    for name in IMAGE_BOOST_SYMBOLS:
        assert name in declared, f"{name} is not declared in include/gbnf.h"
        assert name in native.ABI_SYMBOLS
        assert hasattr(L, name), f"{name} missing from libgbnf_hip.so"
    assert L.gbnf_version() == 4


def test_entry_points_refuse_null_arguments_without_a_device():
    L = native.lib()
    nb = C.c_int64(-7)
    buf = (C.c_float * 64)()          # host memory: a refused call never touches it
    p = C.cast(buf, C.c_void_p)
    null_entry = (C.c_void_p * 2)(None, None)
    calls = [
        ("rho workspace, null flows", lambda: L.gbnf_image_rho_step_workspace_bytes(None, 2, 16, C.byref(nb))),
        ("rho workspace, null entry", lambda: L.gbnf_image_rho_step_workspace_bytes(null_entry, 2, 16, C.byref(nb))),
        ("rho workspace, null bytes", lambda: L.gbnf_image_rho_step_workspace_bytes(null_entry, 2, 16, None)),
        ("rho workspace, n = 0", lambda: L.gbnf_image_rho_step_workspace_bytes(null_entry, 2, 0, C.byref(nb))),
        ("rho step, all null", lambda: L.gbnf_image_mixture_rho_step(None, 1, None, None, 16, None, 0.1, None, None, None, 0, None)),
        ("rho step, null flows", lambda: L.gbnf_image_mixture_rho_step(None, 1, p, None, 16, p, 0.1, p, p, p, 256, None)),
        ("rho step, null entry", lambda: L.gbnf_image_mixture_rho_step(null_entry, 1, p, None, 16, p, 0.1, p, p, p, 256, None)),
        ("rho step, component 0", lambda: L.gbnf_image_mixture_rho_step(null_entry, 0, p, None, 16, p, 0.1, p, p, p, 256, None)),
        ("rho step, n = 0", lambda: L.gbnf_image_mixture_rho_step(null_entry, 1, p, None, 0, p, 0.1, p, p, p, 256, None)),
        ("boosted workspace", lambda: L.gbnf_image_boosted_step_workspace_bytes(None, None, 16, C.byref(nb))),
        ("boosted step", lambda: L.gbnf_image_boosted_nll_step(None, -10.0, None, None, None, 16, 1.0, None, None, None, None, None, None, 0,
                                                               None)),
        ("boosted step, null trainer", lambda: L.gbnf_image_boosted_nll_step(None, -10.0, None, p, None, 16, 1.0, p, None, None, None, p, p,
                                                                             256, None)),
    ]
    for what, call in calls:
        assert call() == -1, f"{what}: accepted"
        assert L.gbnf_last_error(), f"{what}: no message"
    assert nb.value == -7 and not any(buf)


def test_replay_on_a_hand_made_table():
    """The replay against a table whose recursion is exact: equal components, so fixed_ll = ll_0 + log(1) whatever rho[1] is."""
    ll = np.array([[-3.0, -5.0], [-3.0, -5.0], [-4.0, -7.0]])
    rho0 = [1.0, 0.5, 0.25]
    assert np.allclose(fixed_ll64(ll, rho0, 2), ll[0], rtol=0, atol=1e-15)
    assert abs(grad64(ll, rho0, 2) - 1.5) < 1e-15
    assert abs(grad64(ll, rho0, 1) - 0.0) < 1e-15          # component 1: fixed_ll = ll_0, new_ll = ll_1
    r = replay_update_rho([ll], rho0, 2, rho_lr=0.01, rho_iters=40)
    # constant gradient 1.5: rho falls by 0.015 / (0.05 k + 1) per iteration until the clamp or the stop rule
    want = 0.25
    for k in range(r["iters"]):
        want = min(max(want - 0.01 / (0.05 * k + 1) * 1.5, 0.01), 100.0)
    assert abs(r["rho"] - want) < 1e-15
    assert r["iters"] > MIN_ITERS + 1 and (r["difs"][-1] < TOLERANCE or r["iters"] == 40)
    assert all(d >= TOLERANCE for d in r["difs"][MIN_ITERS + 1:-1])
    r = replay_update_rho([ll], rho0, 2, rho_lr=1e6, rho_iters=12)
    assert r["rho"] == 0.01 and r["iters"] == 12
    assert np.isnan(grad64(ll + np.array([[0.0], [1.0], [0.0]]), [1.0, 1.5, 0.25], 2))


def test_checkpoint_keeps_the_shuffles_of_an_image_model(tmp_path):
    """checkpoint.save / load of a 2-component shuffle model: the second model, built under another seed, ends up with the first
    one's Permute2d.indices and ActNorm flags (without the side-car it keeps its own random shuffles)."""
    import torch
    from gbnf_amd import BoostedFlow, checkpoint, image_glow
    dev = torch.device("cpu")
    args = image_args((2, 8, 12), 16, 2, 2, dev, C_=2, permutation="shuffle")
    torch.manual_seed(11)
    a = BoostedFlow(args)
    assert isinstance(a, image_glow.BoostedImageFlow)
    a.flows[0].set_actnorm_init()                 # component 0 initialised, component 1 not
    a.component = 1
    torch.manual_seed(12)
    b = BoostedFlow(args)

    def perms(m):
        return [p.indices.clone() for f in m.flows for p in f.modules() if isinstance(p, image_glow.Permute2d)]

    def flags(m):
        return [bool(n.inited) for f in m.flows for n in f._actnorms()]

    pa, pb = perms(a), perms(b)
    assert len(pa) == 2 * 2 * 2 and any(not torch.equal(u, v) for u, v in zip(pa, pb)), "the two seeds drew the same shuffles"
    assert flags(a) != flags(b)
    path = str(tmp_path / "model_c1.pt")
    checkpoint.save(a, None, path)
    checkpoint.load(b, None, path, args, verbose=False)
    assert all(torch.equal(u, v) for u, v in zip(pa, perms(b)))
    assert flags(b) == flags(a) and any(flags(b)) and not all(flags(b))
    assert b.component == 1 and b.all_trained is False
    assert all(torch.equal(u, v) for (_, u), (_, v) in zip(a.state_dict().items(), b.state_dict().items()))
    assert b._handles == {} and b._trainers == {}
