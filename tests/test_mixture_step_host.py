"""CPU: the joint mixture step's yardstick (tests/mixture_step_oracle.py) checked against central differences of its own loss and
the reference's own gradient; the two new symbols; the refusals that return before a device is touched."""
import copy
import ctypes
import os
import re

import numpy as np
import pytest

from conftest import GRADS_CASES, REPO, load_grads_case
from gbnf_amd import native
from oracle import gbnf_oracle as oracle
import mixture_step_oracle as mso

NEW_SYMBOLS = ("gbnf_mixture_step_workspace_bytes", "gbnf_mixture_nll_step")
G_RTOL = 2e-4          # tests/test_hip_train.py's bar on the g10 fixtures
GBNF_ERR_INVALID = -1


def test_new_symbols_are_declared_bound_and_exported():
    text = open(os.path.join(REPO, "include", "gbnf.h")).read()
    text = re.sub(r"/\*.*?\*/", "", text, flags=re.S)
    declared = set(re.findall(r"\b(gbnf_[a-z_]+)\s*\(", text))
    assert os.path.exists(native.LIB_PATH), "build the library first: python __graft_entry__.py"
    lib = ctypes.CDLL(native.LIB_PATH)
    for name in NEW_SYMBOLS:
        assert name in declared, f"{name} is not declared in include/gbnf.h"
        assert name in native.ABI_SYMBOLS, f"{name} is not in native.ABI_SYMBOLS"
        assert hasattr(lib, name), f"{name} missing from libgbnf_hip.so"
    assert lib.gbnf_version() == 4
    assert len(native.lib().gbnf_mixture_nll_step.argtypes) == 15
    assert len(native.lib().gbnf_mixture_step_workspace_bytes.argtypes) == 4


# ---- the yardstick against central differences of its own loss -------------------------------------------------------------------
def _probe_sites(spec):
    """[(label, getter of the array inside a spec)] -- ActNorm logs, first, hidden and last Linear weight of step 0's net."""
    layers = spec["steps"][0]["net"]["layers"]
    assert len(layers) >= 3
    sites = [("actnorm logs", lambda sp: ("an_logs", None))]
    for label, j in (("first layer", 0), ("hidden layer", 1), ("last layer", len(layers) - 1)):
        sites.append((label + " weight", lambda sp, j=j: ("layer", j)))
    return sites


def _perturbed(specs, c, site, index, delta):
    """A deep copy of specs with one entry of component c's step-0 tensor moved by delta (the tensor becomes float64)."""
    out = copy.deepcopy(list(specs))
    st = out[c]["steps"][0]
    if site[0] == "an_logs":
        a = np.asarray(st["an_logs"], dtype=np.float64).copy()
        a[index] += delta
        st["an_logs"] = a
    else:
        w, b = st["net"]["layers"][site[1]]
        w = np.asarray(w, dtype=np.float64).copy()
        w[index] += delta
        st["net"]["layers"][site[1]] = (w, b)
    return out


def _grad_of_site(spec, grads, site):
    """The yardstick's gradient of the tensor a site names (param_arrays order: [an_bias, an_logs, w0, b0, w1, b1, ...] per step)."""
    return np.asarray(grads[1] if site[0] == "an_logs" else grads[2 + 2 * site[1]], dtype=np.float64)


def test_gradients_equal_central_differences_of_the_mixture_nll(golden_case):
    """g6_glow_d43_h64_c3_rho (tanh nets, no kinks), float64, h = 1e-6: per component the largest entry of the ActNorm logs and of the
    first, hidden and last Linear weight of step 0.  Bar: 1e-5 of the largest probed entry.  Also sum_c rbar_c = 1 to 1e-14."""
    g = golden_case("g6_glow_d43_h64_c3_rho")
    specs = g.specs[: g.n_used]
    assert specs[0]["kind"] == "glow" and len(specs) == 3
    nll, G, r, rbar, grads = mso.step64(specs, g.rho, g.x)
    assert abs(nll - mso.nll64(specs, g.rho, g.x)) <= 1e-14 * abs(nll)
    assert abs(float(rbar.sum()) - 1.0) <= 1e-14
    print(f"nll {nll:.6f}, rbar {np.array2string(rbar, precision=3)}")
    h = 1e-6
    probes = []
    for c, sp in enumerate(specs):
        for label, site_of in _probe_sites(sp):
            site = site_of(sp)
            ga = _grad_of_site(sp, grads[c], site)
            index = np.unravel_index(int(np.abs(ga).argmax()), ga.shape)
            fd = (mso.nll64(_perturbed(specs, c, site, index, +h), g.rho, g.x)
                  - mso.nll64(_perturbed(specs, c, site, index, -h), g.rho, g.x)) / (2 * h)
            probes.append((c, label, float(ga[index]), fd))
    scale = max(abs(p[2]) for p in probes)
    for c, label, mine, fd in probes:
        print(f"component {c} {label}: step64 {mine:+.7e}  central difference {fd:+.7e}  |d| / max {abs(mine - fd) / scale:.1e}")
    assert len(probes) >= 4 * len(specs)
    for c, label, mine, fd in probes:
        assert abs(mine - fd) <= 1e-5 * scale, (c, label, mine, fd)


def test_given_responsibilities_scale_the_gradient_linearly(golden_case):
    """step64(r=...) judges a backward on the r it is handed: doubling r_c doubles component c's gradient, the loss stays."""
    g = golden_case("g5_glow_d6_h30_c2")
    specs = g.specs[: g.n_used]
    nll, G, r, rbar, grads = mso.step64(specs, g.rho, g.x)
    nll2, _, r2, rbar2, grads2 = mso.step64(specs, g.rho, g.x, r=2.0 * r)
    assert nll2 == nll and np.array_equal(r2, 2.0 * r) and np.allclose(rbar2, 2.0 * rbar, rtol=1e-15)
    for c in range(len(specs)):
        a, b = mso.flat64(specs[c], grads[c]), mso.flat64(specs[c], grads2[c])
        assert np.abs(b - 2.0 * a).max() <= 1e-12 * np.abs(a).max()


@pytest.mark.parametrize("name", GRADS_CASES)
def test_lone_component_is_the_references_gradient(name):
    """g10: for C = 1 (r = 1) the yardstick is the reference's own nll.backward(), at the existing G_RTOL per tensor."""
    cfg, spec, x, nll, flat, g_x = load_grads_case(name)
    nll_mine, G, r, rbar, grads = mso.step64([spec], [1.0], x)
    assert np.array_equal(r, np.ones_like(r)) and rbar[0] == 1.0
    assert abs(nll_mine - nll) <= 1e-5 * abs(nll)
    mine = mso.flat64(spec, grads[0])
    assert mine.shape == np.asarray(flat).shape
    off = 0
    for a in oracle.param_arrays(spec):
        size = spec["d"] if a is None else int(np.size(a))
        ref = np.asarray(flat[off:off + size], dtype=np.float64)
        err = float(np.abs(mine[off:off + size] - ref).max())
        assert err <= G_RTOL * max(float(np.abs(ref).max()), 1e-3), (name, off, err)
        off += size


# ---- refusals that return before a device is touched (null and shape arguments) ----------------------------------------------------
def _rc(fn, *args):
    rc = fn(*args)
    msg = native.lib().gbnf_last_error().decode(errors="replace")
    return rc, msg


def test_error_code_is_the_headers():
    text = open(os.path.join(REPO, "include", "gbnf.h")).read()
    m = re.search(r"GBNF_ERR_INVALID\s*=\s*(-?\d+)", text)
    assert m is not None and int(m.group(1)) == GBNF_ERR_INVALID
    m = re.search(r"#define\s+GBNF_WEIGHTS_MAX_COMPONENTS\s+(\d+)", text)
    assert m is not None and int(m.group(1)) == native.WEIGHTS_MAX_COMPONENTS


def test_mixture_nll_step_refuses_bad_arguments():
    L = native.lib()
    one = ctypes.c_void_p(16)          # (never dereferenced: every call below is refused on its arguments)
    vp2 = ctypes.c_void_p * 2
    none_arr, ones = vp2(None, None), vp2(16, 16)
    hypers = (native._OptHyper * 2)()
    for h in hypers:
        h.kind, h.step, h.lr = 1, 1, 1e-3
    good = dict(trainers=none_arr, C=2, log_w=one, x=one, n=4, grads=ones, m=ones, v=ones, hypers=hypers, stats=one, G=None, r=None,
                ws=one, wsb=1 << 20)

    def call(**kw):
        a = {**good, **kw}
        return _rc(L.gbnf_mixture_nll_step, a["trainers"], a["C"], a["log_w"], a["x"], a["n"], a["grads"], a["m"], a["v"], a["hypers"],
                   a["stats"], a["G"], a["r"], a["ws"], a["wsb"], None)

    for kw in (dict(trainers=None), dict(grads=None), dict(m=None), dict(v=None), dict(hypers=None), dict(log_w=None), dict(x=None),
               dict(stats=None), dict(ws=None), dict(C=0), dict(C=native.WEIGHTS_MAX_COMPONENTS + 1), dict(n=0), dict(n=-1),
               dict()):          # (the last: both entries of `trainers` are null)
        rc, msg = call(**kw)
        assert rc == GBNF_ERR_INVALID and "gbnf_mixture_nll_step" in msg, (kw, msg)
    assert "trainers[0] is null" in call()[1]
    same = vp2(16, 16)                 # one (fake, never dereferenced) handle twice
    rc, msg = call(trainers=same)
    assert rc == GBNF_ERR_INVALID and "same trainer" in msg


def test_mixture_step_workspace_bytes_refuses_bad_arguments():
    L = native.lib()
    none_arr = (ctypes.c_void_p * 2)(None, None)
    nb = ctypes.c_int64(-1)
    for args in ((None, 2, 4, ctypes.byref(nb)), (none_arr, 2, 4, None), (none_arr, 0, 4, ctypes.byref(nb)),
                 (none_arr, native.WEIGHTS_MAX_COMPONENTS + 1, 4, ctypes.byref(nb)), (none_arr, 2, 0, ctypes.byref(nb)),
                 (none_arr, 2, 4, ctypes.byref(nb))):
        rc, msg = _rc(L.gbnf_mixture_step_workspace_bytes, *args)
        assert rc == GBNF_ERR_INVALID and "gbnf_mixture_step_workspace_bytes" in msg and nb.value == -1, (args, msg)


def test_python_binding_refuses_host_tensors_and_wrong_lengths():
    import torch
    with pytest.raises(native.GbnfError):
        native.mixture_nll_step([], [], torch.zeros(1), torch.zeros(4, 3), lr=1e-3)
    with pytest.raises(native.GbnfError):
        native.mixture_nll_step([object()], [object()], torch.zeros(1), torch.zeros(4, 3), lr=1e-3)
    with pytest.raises(native.GbnfError):
        native.mixture_step_workspace_bytes([object()], 4)

    class _Open(native.NativeTrainer):           # an "open" trainer that never reaches the library: the argument checks come first
        def __init__(self):
            self.handle, self.d, self.grad_floats = ctypes.c_void_p(16), 3, 8

        def __del__(self):
            pass

    tr = _Open()
    st = native.OptState.__new__(native.OptState)
    st.kind, st.step, st.grad_floats, st.exp_avg, st.exp_avg_sq = "sgd", 0, 8, None, None
    host = ([tr], [st], torch.zeros(1), torch.zeros(4, 3))
    for kw, args in ((dict(lr=1e-3), ([tr], [st, st]) + host[2:]),          # states of the wrong length
                     (dict(lr=[1e-3, 1e-3]), host),                         # lr of the wrong length
                     (dict(lr=[]), host),
                     (dict(lr=1e-3), host)):                                # x (and log_w) on the host
        with pytest.raises(native.GbnfError):
            native.mixture_nll_step(*args, **kw)
