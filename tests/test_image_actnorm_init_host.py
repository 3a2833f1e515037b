"""CPU: the host side of the one-pass ActNorm2d initialisation (gbnf_image_trainer_actnorm_init): ABI names, ctypes signatures, the
skip vector, the default of initialize_actnorms, and the margin that gives the GPU test's bar its meaning."""
import ctypes as C
import inspect
import os
import re

import numpy as np
import pytest

import image_actnorm_init_cases as cases
from conftest import REPO

NAMES = ("gbnf_image_trainer_actnorm_count", "gbnf_image_trainer_actnorm_init_workspace_bytes", "gbnf_image_trainer_actnorm_init")


def test_names_are_declared_bound_and_exported():
    from gbnf_amd import native
    text = re.sub(r"/\*.*?\*/", "", open(os.path.join(REPO, "include", "gbnf.h")).read(), flags=re.S)
    declared = set(re.findall(r"\b(gbnf_[a-z_]+)\s*\(", text))
    assert "#define GBNF_ABI_VERSION 4" in text
    lib = C.CDLL(native.LIB_PATH)
    for name in NAMES:
        assert name in declared and name in native.ABI_SYMBOLS and hasattr(lib, name), name


def test_ctypes_signatures():
    from gbnf_amd import native
    L = native.lib()                                        # dlopen + binding only: touches no device
    vp, i32, i64 = C.c_void_p, C.c_int32, C.c_int64
    assert L.gbnf_image_trainer_actnorm_count.argtypes == [vp, C.POINTER(i32)]
    assert L.gbnf_image_trainer_actnorm_init_workspace_bytes.argtypes == [vp, i64, C.POINTER(i64)]
    assert L.gbnf_image_trainer_actnorm_init.argtypes == [vp, vp, vp, i64, C.c_float, vp, vp, i64, vp]
    for name in NAMES:
        assert getattr(L, name).restype is C.c_int


@pytest.mark.parametrize("name", list(cases.CASES))
def test_float32_oracle_stays_inside_the_margin(name):
    """The GPU test holds an exact-f32 implementation to 1e-5 of the float64 oracle.  That bar means something only while float32
    arithmetic itself lands well inside it on these shapes: the float32 oracle within 1e-6 on every layer (measured: <= 3e-7)."""
    _, ref64 = cases.oracle_init(name, "float64")
    _, ref32 = cases.oracle_init(name, "float32")
    w = cases.worst(ref32, ref64)
    print(f"{name}: float32 oracle against float64 {w:.3e} of {cases.MARGIN}")
    assert w <= cases.MARGIN
    assert max(float(np.abs(l).max()) for _, l in ref64) < 10.0          # logs of order one: the bar is absolute, in effect


def test_cases_are_zeroed_and_counted():
    for name, (size, n, kw) in cases.CASES.items():
        spec, x, noise = cases.make(name)
        acts = cases.spec_actnorms(spec)
        depth = kw.get("depth", 1)
        assert len(acts) == kw["L"] * kw["K"] * (2 + depth)               # a step's own + one per Conv2d of its net
        assert all(not np.any(b) and not np.any(l) for b, l in acts)
        assert x.shape == (n,) + size == noise.shape


def test_skip_flags_follow_the_inited_flags_in_module_order():
    import argparse
    import torch
    from gbnf_amd import BoostedFlow, image_glow
    args = argparse.Namespace(
        num_flows=2, z_size=1 * 8 * 8, density_evaluation=True, device=torch.device("cpu"), cuda=False, component_type="glow",
        num_components=1, rho_init="decreasing", learn_top=True, y_classes=0, y_condition=False, sample_size=4, input_size=[1, 8, 8],
        h_size=8, num_blocks=1, actnorm_scale=1.0, flow_permutation="invconv", flow_coupling="affine", LU_decomposed=False,
        num_dequant_blocks=0, coupling_network="tanh", coupling_network_depth=1, batch_norm=False)
    m = BoostedFlow(args)
    glow = m.flows[0]
    acts = glow._actnorms()
    assert len(acts) == 2 * 3
    # module order: a FlowStep's own ActNorm2d, then the ones of its coupling net, step by step
    steps = [l for l in glow.flow.layers if isinstance(l, image_glow.FlowStep)]
    expect = []
    for st in steps:
        expect.append(st.actnorm)
        expect += [c.actnorm for c in st.block.network if isinstance(c, image_glow.Conv2d)]
    assert all(a is b for a, b in zip(acts, expect))
    assert image_glow.actnorm_skip_flags(glow) == [False] * 6
    for i in (1, 2, 5):
        acts[i].inited = True
    assert image_glow.actnorm_skip_flags(glow) == [False, True, True, False, False, True]


def test_fused_is_off_by_default():
    from gbnf_amd import image_glow, native
    sig = inspect.signature(image_glow.BoostedImageFlow.initialize_actnorms)
    assert sig.parameters["fused"].default is False
    assert list(sig.parameters)[:4] == ["self", "x", "components", "noise"]
    sig = inspect.signature(native.NativeImageTrainer.actnorm_init)
    assert sig.parameters["scale"].default == 1.0 and sig.parameters["skip"].default is None
    assert inspect.signature(image_glow.BoostedImageFlow._native_trainer).parameters["allow_uninit"].default is False
