"""CPU: the tabular score's yardstick (tests/score_oracle.py) checked against itself, the oracle's recursion and the reference's own
gradient; the new symbols; the refusals of the three calls that return before they touch a device."""
import ctypes
import os
import re

import numpy as np
import pytest

from conftest import GRADS_CASES, REPO, load_grads_case
from gbnf_amd import native
from oracle import gbnf_oracle as oracle
import score_oracle

NEW_SYMBOLS = ("gbnf_trainer_backward_x_workspace_bytes", "gbnf_trainer_backward_x", "gbnf_score_seed",
               "gbnf_mixture_score_workspace_bytes", "gbnf_mixture_score")
G_RTOL = 2e-4          # tests/test_hip_train.py's bar on the g10 fixtures


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


@pytest.mark.parametrize("name", ["g6_glow_d43_h64_c3_rho", "g1_toy_realnvp_c2", "g4_realnvp_d21_h105_c8"])
def test_closed_form_equals_the_recursion(name, golden_case):
    """G = LSE_c(log(rho_c / sum rho) + ll_c) against oracle.mixture_log_prob's prefix-normalised recursion, float64.  Bar: 1e-12."""
    g = golden_case(name)
    specs = g.specs[: g.n_used]
    _, G, r, ll = score_oracle.score64(specs, g.rho, g.x, base=g.base)
    ll_ref, G_ref = oracle.mixture_log_prob(g.specs, g.rho, g.x, n_used=g.n_used, backend="numpy64", base=g.base)
    err_ll, err_G = float(np.abs(ll - ll_ref).max()), float(np.abs(G - G_ref).max())
    print(f"{name}: |ll - ll_ref| = {err_ll:.2e}, |G - recursion| = {err_G:.2e}")
    assert err_ll <= 1e-12 and err_G <= 1e-12
    assert np.abs(r.sum(axis=0) - 1.0).max() <= 1e-14


@pytest.mark.parametrize("name", ["g6_glow_d43_h64_c3_rho", "g1_toy_realnvp_c2"])
def test_score_equals_central_differences_of_its_own_log_density(name, golden_case):
    """float64, h = 1e-5, the first 4 rows: tanh nets (no kinks) and the toy fixture with its base.  Bar: 1e-7 of the largest entry."""
    g = golden_case(name)
    specs = g.specs[: g.n_used]
    x = np.asarray(g.x[:4], dtype=np.float64)
    g_x, _, _, _ = score_oracle.score64(specs, g.rho, x, base=g.base)
    h = 1e-5
    fd = np.zeros_like(x)
    for j in range(x.shape[1]):
        xp, xm = x.copy(), x.copy()
        xp[:, j] += h
        xm[:, j] -= h
        Gp = score_oracle.score64(specs, g.rho, xp, base=g.base)[1]
        Gm = score_oracle.score64(specs, g.rho, xm, base=g.base)[1]
        fd[:, j] = (Gp - Gm) / (2 * h)
    err = float(np.abs(g_x - fd).max() / np.abs(fd).max())
    print(f"{name}: |score64 - central differences| / max = {err:.2e}")
    assert err <= 1e-7


@pytest.mark.parametrize("name", GRADS_CASES)
def test_lone_component_score_is_the_references_gradient(name):
    """g10: the reference's nll.backward() gave g_x = d mean(-ll) / dx, so the score of the lone component is -N g_x."""
    cfg, spec, x, nll, flat, g_x = load_grads_case(name)
    s64 = score_oracle.score64([spec], [1.0], x)[0]
    ref = -x.shape[0] * np.asarray(g_x, dtype=np.float64)
    err = float(np.abs(s64 - ref).max() / np.abs(ref).max())
    print(f"{name}: |score64 + N g_x| / max = {err:.2e}")
    assert err <= G_RTOL


# ---- refusals that return before a device is touched (null and shape arguments)
def _rc(fn, *args):
    rc = fn(*args)
    msg = native.lib().gbnf_last_error().decode(errors="replace")
    return rc, msg


GBNF_ERR_INVALID = -1


def test_error_codes_are_the_headers():
    text = open(os.path.join(REPO, "include", "gbnf.h")).read()
    m = re.search(r"GBNF_ERR_INVALID\s*=\s*(-?\d+)", text)
    assert m is not None and int(m.group(1)) == GBNF_ERR_INVALID


def test_backward_x_refuses_null_arguments():
    L = native.lib()
    one = ctypes.c_void_p(16)          # (never dereferenced: every call below is refused on its arguments)
    nb = ctypes.c_int64(-1)
    rc, msg = _rc(L.gbnf_trainer_backward_x, None, one, 4, None, None, None, one, 0, one, 1 << 20, None)
    assert rc == GBNF_ERR_INVALID and "trainer is null" in msg
    rc, msg = _rc(L.gbnf_trainer_backward_x_workspace_bytes, None, 4, ctypes.byref(nb))
    assert rc == GBNF_ERR_INVALID and nb.value == -1


def test_score_seed_refuses_bad_arguments():
    L = native.lib()
    one = ctypes.c_void_p(16)
    for args in ((None, None, None, None, 4, 3, one, one, None, None),        # z
                 (one, None, None, None, 4, 3, None, one, None, None),        # g_z
                 (one, None, None, None, 4, 3, one, None, None, None),        # g_ldj
                 (one, None, None, None, -1, 3, one, one, None, None),        # n < 0
                 (one, None, None, None, 4, 0, one, one, None, None),         # d < 1
                 (one, one, None, None, 4, 3, one, one, None, None),          # mean without std
                 (one, None, one, None, 4, 3, one, one, None, None)):         # std without mean
        rc, msg = _rc(L.gbnf_score_seed, *args)
        assert rc == GBNF_ERR_INVALID and "gbnf_score_seed" in msg, (args, msg)
    assert L.gbnf_score_seed(one, None, None, None, 0, 3, one, one, None, None) == 0          # n == 0: nothing to do


def test_mixture_score_refuses_bad_arguments():
    L = native.lib()
    one = ctypes.c_void_p(16)
    none_arr = (ctypes.c_void_p * 2)(None, None)
    nb = ctypes.c_int64(-1)
    good = dict(trainers=none_arr, C=2, log_w=one, mean=None, std=None, ll=None, x=one, n=4, g_x=one, G=one, r=None, ws=one, wsb=1 << 20)

    def call(**kw):
        a = {**good, **kw}
        return _rc(L.gbnf_mixture_score, a["trainers"], a["C"], a["log_w"], a["mean"], a["std"], a["ll"], a["x"], a["n"], a["g_x"], a["G"],
                   a["r"], a["ws"], a["wsb"], None)

    for kw in (dict(trainers=None), dict(log_w=None), dict(x=None), dict(g_x=None), dict(G=None), dict(ws=None), dict(C=0), dict(n=-1),
               dict(mean=one), dict(std=one), dict()):          # (the last: both entries of `trainers` are null)
        rc, msg = call(**kw)
        assert rc == GBNF_ERR_INVALID and "gbnf_mixture_score" in msg, (kw, msg)
    assert "trainers[0] is null" in call()[1]
    for args in ((None, 2, 4, ctypes.byref(nb)), (none_arr, 2, 4, None), (none_arr, 0, 4, ctypes.byref(nb)), (none_arr, 2, -1, ctypes.byref(nb)),
                 (none_arr, 2, 4, ctypes.byref(nb))):
        rc, msg = _rc(L.gbnf_mixture_score_workspace_bytes, *args)
        assert rc == GBNF_ERR_INVALID and nb.value == -1, (args, msg)


def test_python_binding_refuses_host_tensors_and_wrong_shapes():
    import torch
    with pytest.raises(native.GbnfError):
        native.score_seed(torch.zeros(4, 3))                       # not on the device
    with pytest.raises(native.GbnfError):
        native.mixture_score([], torch.zeros(1), torch.zeros(4, 3))
    with pytest.raises(native.GbnfError):
        native.mixture_score_workspace_bytes([object()], 4)
