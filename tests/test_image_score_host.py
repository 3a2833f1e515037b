"""Host: the image score's symbols in header, binding and library; the numpy restatement of the library's last adjoint against
torch autograd in float64; the mixture models' kink margins and responsibilities on the yardstick; the g24 fixtures (the reference's
own input gradient) against the yardstick."""
import ctypes
import os
import re

import numpy as np
import pytest
import torch

import image_grad_oracle as igo
import image_score_cases as isc

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
# symbol -> parameters of its declaration in include/gbnf.h
NEW_SYMBOLS = {"gbnf_image_trainer_backward_x": 13, "gbnf_image_score_seed": 10, "gbnf_mixture_responsibilities": 7,
               "gbnf_image_mixture_score_workspace_bytes": 4, "gbnf_image_mixture_score": 13}


def test_new_symbols_in_header_binding_and_library():
    from gbnf_amd import native
    hdr = re.sub(r"/\*.*?\*/", "", open(os.path.join(ROOT, "include", "gbnf.h")).read(), flags=re.S)
    assert "#define GBNF_ABI_VERSION 4" in hdr
    L = native.lib()                        # dlopen + symbol binding only; touches no device
    for name, n_params in NEW_SYMBOLS.items():
        m = re.search(r"\bint\s+%s\s*\(([^)]*)\)\s*;" % name, hdr)
        assert m, f"{name} is not declared in include/gbnf.h"
        assert len(m.group(1).split(",")) == n_params, name
        assert name in native.ABI_SYMBOLS, f"{name} is not in native.ABI_SYMBOLS"
        fn = getattr(L, name)
        assert fn.restype is ctypes.c_int and len(fn.argtypes) == n_params, name
    # a pointer is a pointer, a count is a count: the declared C types against the ctypes ones, in order
    kinds = {"int64_t": ctypes.c_int64, "int32_t": ctypes.c_int32}
    for name in NEW_SYMBOLS:
        params = re.search(r"\bint\s+%s\s*\(([^)]*)\)\s*;" % name, hdr).group(1).split(",")
        for decl, ct in zip(params, getattr(L, name).argtypes):
            decl = " ".join(decl.split())
            if "*" in decl:
                assert ct is ctypes.c_void_p or issubclass(ct, ctypes._Pointer), (name, decl, ct)
            else:
                assert ct is kinds[decl.split()[0]], (name, decl, ct)
    for attr in ("score_seed", "mixture_responsibilities", "image_mixture_score"):
        assert callable(getattr(native, attr))
    assert callable(native.NativeImageTrainer.backward_x)


@pytest.mark.parametrize("size,with_noise", [((2, 8, 12), True), ((1, 28, 20), True), ((3, 6, 4), False)])
def test_pre_adjoint_restatement_against_autograd(size, with_noise):
    """g_x = (g_logit + g_ldj (2v - 1)) / (v (1 - v)) * bounds * 255 / 256 and the un-squeeze, against float64 autograd of the
    yardstick's own head (dequantise, logit, its log-det, the first squeeze)."""
    rng = np.random.RandomState(5)
    n, bounds = 3, 0.9
    C, H, W = size
    x = rng.randint(0, 256, size=(n,) + size).astype(np.float64) / 255.0
    noise = rng.uniform(size=x.shape) if with_noise else None
    g_sq = rng.standard_normal((n, 4 * C, H // 2, W // 2))
    g_ldj = rng.standard_normal(n)
    xl = torch.tensor(x, requires_grad=True)
    u = (255.0 * xl + (torch.tensor(noise) if with_noise else 0.0)) / 256.0
    v = ((u * 2.0 - 1.0) * bounds + 1.0) / 2.0
    logit = torch.log(v) - torch.log(1.0 - v)
    sp = torch.nn.functional.softplus
    ld = (sp(logit) + sp(-logit)).flatten(1).sum(-1)
    ((igo._squeeze(logit) * torch.tensor(g_sq)).sum() + (ld * torch.tensor(g_ldj)).sum()).backward()
    got = isc.pre_adjoint_numpy(x, noise, g_sq, g_ldj, bounds)
    assert np.abs(got - xl.grad.numpy()).max() <= 1e-12 * np.abs(xl.grad.numpy()).max()


@pytest.mark.parametrize("name", sorted(isc.MIX_MODELS))
def test_mixture_models_are_clear_of_kinks_and_one_hot_rows(name):
    specs, log_w, x, noise = isc.mixture_case(name)
    assert len(specs) == 3 and np.all(np.diff(log_w) < 0)          # rho decreasing
    for sp in specs:
        rows = igo.kink_report(sp, x, noise)
        assert rows and [inside for inside, _ in rows] == [0] * len(rows)
    y = isc.mixture_yardstick(specs, log_w, x, noise)
    print(name, "largest responsibility per row", y["r"].max(axis=0))
    assert np.all(y["r"].max(axis=0) <= isc.R_MAX)
    # the autograd gradient of sum G is sum_c r_c grad ll_c: the identity the library's one call rests on
    comp = [isc.component_yardstick(sp, x, noise)[1] for sp in specs]
    mix = sum(y["r"][c].reshape(-1, 1, 1, 1) * comp[c] for c in range(len(specs)))
    assert np.abs(mix - y["gx"]).max() <= 1e-10 * np.abs(y["gx"]).max()


@pytest.mark.parametrize("name", igo.G21)
def test_fixture_matches_the_yardstick(name):
    """The reference's own f32 CPU autograd d sum(ll) / dx (fixtures g24) against the float64 yardstick with x a leaf: 1e-5 of the
    largest entry, the bar of the g21 parameter gradients."""
    cfg, data = igo.g21_load(name)
    g24 = np.load(os.path.join(ROOT, "tests", "golden", "image_score", name.replace("g21_image_grads", "g24_image_score") + ".npz"))
    from gbnf_amd import image_glow
    m = igo.g21_module(cfg, data, torch.device("cpu"))
    sp = image_glow.image_spec_from_glow_module(m.flows[0])
    ll, gx = isc.component_yardstick(sp, data["x"], data["noise"])
    assert g24["gx"].shape == data["x"].shape
    err = float(np.abs(gx - g24["gx"]).max()) / float(np.abs(gx).max())
    print(f"{name}: fixture against the yardstick {err:.3e} of 1e-5")
    assert err <= 1e-5
    assert np.abs(ll - g24["ll"]).max() <= 1e-5 * np.abs(ll).max()
