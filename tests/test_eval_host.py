"""CPU: the validation pass's ABI (gbnf_eval_accumulate and the calls around it) as far as it goes without a device -- header and
binding, the workspace size, every refusal that returns before a launch -- and the float64 yardstick of the GPU tests
(tests/eval_oracle.py) tied to the reference: its recursion against the G the reference itself wrote into the g2 / g3 / g4 fixtures,
its class loss against torch.nn.functional.cross_entropy in float64."""
import ctypes as C
import os
import re

import numpy as np
import pytest

import eval_oracle as eo
from conftest import REPO

EVAL_SYMBOLS = ("gbnf_eval_workspace_bytes", "gbnf_eval_accumulate", "gbnf_eval_accumulate_class_loss", "gbnf_mixture_evaluate",
                "gbnf_image_mixture_evaluate_workspace_bytes", "gbnf_image_mixture_evaluate", "gbnf_image_mixture_evaluate_y")
FIXTURES = ("g2_glow_native_d43_h32_c3", "g3_glow_d43_h215_c8", "g4_realnvp_d21_h105_c8", "g4_realnvp_d21_h105_c2_mixed",
            "g4_realnvp_d21_h105_c2_relu_nobn")


def _lib():
    from gbnf_amd import native
    return native.lib()


def test_header_and_binding_agree():
    from gbnf_amd import native
    text = open(os.path.join(REPO, "include", "gbnf.h")).read()
    code = re.sub(r"/\*.*?\*/", "", text, flags=re.S)
    L = _lib()
    for name in EVAL_SYMBOLS:
        assert re.search(r"\b%s\s*\(" % name, code), f"{name} is not declared in include/gbnf.h"
        assert name in native.ABI_SYMBOLS
        fn = getattr(L, name)
        assert fn.argtypes is not None and fn.restype is C.c_int, name
        decl = re.search(r"\b%s\s*\(([^;]*)\);" % name, code).group(1)
        assert len(fn.argtypes) == decl.count(",") + 1, f"{name}: {len(fn.argtypes)} argtypes for `{decl}`"
    assert int(re.search(r"#define\s+GBNF_EVAL_STATE_DOUBLES\s+(\d+)", text).group(1)) == native.EVAL_STATE_DOUBLES == eo.STATE_DOUBLES
    assert sorted(native.EVAL_STATE.values()) == list(range(13))
    assert L.gbnf_version() == 4


def test_workspace_bytes():
    from gbnf_amd import native
    L = _lib()
    nb = C.c_int64(-1)
    sizes = []
    for n in (0, 1, 1024, 1 << 20, 1 << 33):
        assert L.gbnf_eval_workspace_bytes(n, C.byref(nb)) == 0
        sizes.append(nb.value)
        # five sums per workgroup of the largest grid, in 256-byte steps
        assert nb.value >= 5 * 8 * native.EVAL_MAX_PARTIALS and nb.value % 256 == 0 and nb.value <= 1 << 20
    assert sizes == sorted(sizes)
    assert L.gbnf_eval_workspace_bytes(-1, C.byref(nb)) == -1 and L.gbnf_last_error()
    assert L.gbnf_eval_workspace_bytes(4, None) == -1


def test_refusals_before_any_device_call():
    """Every argument check of the calls returns before the device is touched: host addresses stand in for device buffers."""
    L = _lib()
    n = 8
    ll = np.zeros((3, n), dtype=np.float32)
    rho = np.ones(3, dtype=np.float32)
    state = np.full(16, 7.0)
    nb = C.c_int64()
    assert L.gbnf_eval_workspace_bytes(n, C.byref(nb)) == 0
    ws = np.zeros(nb.value // 8, dtype=np.float64)
    p = lambda a: None if a is None else C.c_void_p(a.ctypes.data)

    def acc(ll_=ll, stride=n, n_used=3, n_=n, rho_=rho, component=1, state_=state, ws_=ws, nbytes=nb.value):
        return L.gbnf_eval_accumulate(p(ll_), stride, n_used, n_, p(rho_), component, None, p(state_), p(ws_), nbytes, None)

    bad = {"null ll": dict(ll_=None), "null rho": dict(rho_=None), "null state": dict(state_=None), "null workspace": dict(ws_=None),
           "n < 0": dict(n_=-1), "n_used = 0": dict(n_used=0), "component = n_used": dict(component=3), "component < 0": dict(component=-1),
           "stride < n": dict(stride=n - 1), "short workspace": dict(nbytes=nb.value - 8)}
    for what, kw in bad.items():
        assert acc(**kw) == -1, f"accumulate, {what}: accepted"
        assert L.gbnf_last_error(), what
    assert acc(n_=0, stride=0) == 0, "n = 0 adds nothing and needs no device"

    y = np.zeros((n, 10), dtype=np.float32)

    def cls(lg=y, y_=y, n_=n, Y=10, rho_=rho, n_used=3, c=0, state_=state, ws_=ws, nbytes=nb.value):
        return L.gbnf_eval_accumulate_class_loss(p(lg), p(y_), n_, Y, p(rho_), n_used, c, p(state_), p(ws_), nbytes, None)

    bad = {"null logits": dict(lg=None), "null y": dict(y_=None), "null rho": dict(rho_=None), "null state": dict(state_=None),
           "null workspace": dict(ws_=None), "n < 0": dict(n_=-1), "Y = 0": dict(Y=0), "Y = 257": dict(Y=257), "n_used = 0": dict(n_used=0),
           "c = n_used": dict(c=3), "c < 0": dict(c=-1), "short workspace": dict(nbytes=nb.value - 8)}
    for what, kw in bad.items():
        assert cls(**kw) == -1, f"class loss, {what}: accepted"
        assert L.gbnf_last_error(), what
    assert cls(n_=0) == 0

    x = np.zeros((n, 4), dtype=np.float32)
    assert L.gbnf_mixture_evaluate(None, p(x), n, 3, 1, p(rho), p(ll), None, p(state), p(ws), nb.value, None) == -1
    handles = (C.c_void_p * 2)(None, None)
    img = lambda f, x_, st: L.gbnf_image_mixture_evaluate(f, 2, 0, p(x_), None, n, p(rho), p(ll), None, p(st), p(ws), 1 << 30, None)
    assert img(None, x, state) == -1 and img(handles, None, state) == -1 and img(handles, x, None) == -1
    assert img(handles, x, state) == -1, "a null entry of flows"
    assert L.gbnf_image_mixture_evaluate_y(handles, 2, 0, p(x), None, None, n, p(rho), p(ll), None, p(state), p(ws), 1 << 30, None) == -1
    assert L.gbnf_image_mixture_evaluate_workspace_bytes(handles, 2, n, C.byref(nb)) == -1
    assert L.gbnf_image_mixture_evaluate_workspace_bytes(None, 2, n, C.byref(nb)) == -1
    assert (state == 7.0).all()


@pytest.mark.parametrize("name", FIXTURES)
def test_the_yardstick_reproduces_the_reference(name, golden_case):
    """The recursion of eval_oracle on the fixture's ll and rho is the G the reference wrote, and nll / g_nll / ratio are the means of
    density_experiment.py:581-588 formed directly from the fixture's arrays."""
    g = golden_case(name)
    ll, rho, n_used = g.ll[:g.n_used], g.rho, g.n_used
    G = eo.mixture_G(ll, rho)
    rel = np.abs(G - g.G.astype(np.float64)) / np.abs(g.G.astype(np.float64))
    print(f"{name}: worst relative difference of G {rel.max():.3e}")
    assert rel.max() <= 1e-6
    G32 = eo.mixture_G(ll, rho, dtype=np.float32)
    assert G32.dtype == np.float32 and (np.abs(G32 - g.G) <= 1e-6 * np.abs(g.G)).all()
    for component in (0, n_used - 1):
        s = eo.state_of([ll[:, :100], ll[:, 100:]], rho, component)
        n = ll.shape[1]
        assert s[0] == n and s[1] == 2 and s[9] == 0 and (s[13:] == 0).all()
        got = {"nll": -s[2] / n, "g_nll": -s[3] / n, "ratio": s[4] / n}
        # directly from the fixture: the reference's own G, its own ll of the component
        want = eo.summary(g.G, g.ll[component])
        scale = np.abs(ll).max()
        for key in want:
            assert abs(got[key] - want[key]) <= 1e-6 * scale, (key, got[key], want[key])
        # ... and from the yardstick's own G the two statements are the same numbers
        own = eo.summary(G, ll[component])
        for key in own:
            assert abs(got[key] - own[key]) <= 1e-12 * scale, (key, got[key], own[key])
        assert abs(-s[6] / 2 - 0.5 * (np.mean(-G[:100]) + np.mean(-G[100:]))) <= 1e-12 * scale
        E = (eo.weights(rho, n_used)[:, None] * ll.astype(np.float64)).sum(axis=0)
        assert abs(s[5] - E.sum()) <= 1e-12 * scale * n
    first = eo.summary(G, ll[0], first_pass_component_zero=True)
    assert first["g_nll"] == first["nll"] and first["ratio"] == 0.0


def test_the_class_loss_yardstick_is_cross_entropy():
    """eval_oracle.cross_entropy against F.cross_entropy(y_logits, argmax(y)) in float64 on the CPU: one-hot rows, soft rows, rows with
    ties in y (torch.argmax and the yardstick both take the first of the largest) and ties in the logits."""
    import torch
    import torch.nn.functional as F
    rng = np.random.default_rng(5)
    for n, Y in ((1, 1), (1, 10), (33, 10), (33, 256), (7, 3)):
        logits = (rng.standard_normal((n, Y)) * 3).astype(np.float32)
        y = np.zeros((n, Y), dtype=np.float32)
        y[np.arange(n), rng.integers(0, Y, n)] = 1.0
        if n > 4 and Y > 2:
            y[1] = rng.random(Y)                         # a soft row
            y[2] = 0.0                                   # all tied: the first entry
            y[3, :] = 0.0
            y[3, [Y - 1, 1]] = 0.5                       # two tied maxima: the first of them
            logits[4, :] = logits[4, 0]                  # tied logits: prediction 0
        ce, label, pred = eo.cross_entropy(logits, y)
        t = torch.from_numpy(logits).double()
        target = torch.argmax(torch.from_numpy(y), dim=1)
        want = F.cross_entropy(t, target, reduction="none").numpy()
        assert (label == target.numpy()).all()
        assert (pred == torch.argmax(t, dim=1).numpy()).all()
        assert np.abs(ce - want).max() <= 1e-13 * max(1.0, np.abs(want).max()), (n, Y, np.abs(ce - want).max())
        if n > 4 and Y > 2:
            assert label[2] == 0 and label[3] == 1 and pred[4] == 0
        rho = np.array([1.0, 0.5, 0.25], dtype=np.float32)
        got = eo.class_state(logits, y, rho, 3, 1)
        w = 0.5 / 1.75
        mean = float(F.cross_entropy(t, target, reduction="mean"))
        assert abs(got[1] - w * mean) <= 1e-13 * max(1.0, mean) and abs(got[0] - w * mean * n) <= 1e-13 * max(1.0, mean) * n
        assert got[2] == w * float((torch.argmax(t, dim=1) == target).sum())
