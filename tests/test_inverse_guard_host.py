"""CPU: the interface of the z -> x numerics guard -- the header declares its two entry points, native.py binds them, the built
library exports them, the ABI version has not moved, and a bad `direction` is refused before any device is touched."""
import argparse
import ctypes
import os
import re

import pytest
import torch

from conftest import REPO
from gbnf_amd import native

NEW_SYMBOLS = ("gbnf_flow_numerics_inverse", "gbnf_image_flow_inverse_check_counts")


def _header():
    text = open(os.path.join(REPO, "include", "gbnf.h")).read()
    return text, re.sub(r"/\*.*?\*/", "", text, flags=re.S)


def test_header_declares_and_native_binds_the_inverse_guard_entry_points():
    _, code = _header()
    flat = " ".join(code.split())
    assert "int gbnf_flow_numerics_inverse(const gbnf_flow* flow, gbnf_numerics_status* out);" in flat
    assert ("int gbnf_image_flow_inverse_check_counts(const gbnf_image_flow* flow, int64_t* data_checks, int64_t* failed_checks, "
            "float* worst_rel_err);") in flat
    for name in NEW_SYMBOLS:
        assert name in native.ABI_SYMBOLS


def test_library_exports_the_inverse_guard_entry_points_at_abi_4():
    assert os.path.exists(native.LIB_PATH), "build the library first: python __graft_entry__.py"
    raw = ctypes.CDLL(native.LIB_PATH)
    for name in NEW_SYMBOLS:
        assert hasattr(raw, name), f"{name} missing from libgbnf_hip.so"
    L = native.lib()                                  # dlopen + argtypes only; touches no device
    assert L.gbnf_flow_numerics_inverse.argtypes[1]._type_ is native.NumericsStatus
    assert len(L.gbnf_image_flow_inverse_check_counts.argtypes) == 4
    text, _ = _header()
    assert re.search(r"#define\s+GBNF_ABI_VERSION\s+4\b", text)
    assert L.gbnf_version() == 4
    # null handles are refused with GBNF_ERR_INVALID, no device involved
    st = native.NumericsStatus()
    assert L.gbnf_flow_numerics_inverse(None, ctypes.byref(st)) == -1
    assert L.gbnf_image_flow_inverse_check_counts(None, None, None, None) == -1


def test_a_bad_direction_is_refused_without_a_device():
    from gbnf_amd.boosted_flow import BoostedFlow
    from gbnf_amd.image_glow import BoostedImageFlow
    with pytest.raises(ValueError):
        native.check_direction("sideways")
    assert native.check_direction("forward") == "forward" and native.check_direction("inverse") == "inverse"
    args = argparse.Namespace(
        num_flows=3, z_size=7, density_evaluation=True, device=torch.device("cpu"), cuda=False, component_type="glow",
        num_components=2, rho_init="decreasing", learn_top=False, y_classes=0, y_condition=False, sample_size=4, input_size=[7],
        h_size=12, num_blocks=1, actnorm_scale=1.0, flow_permutation="shuffle", flow_coupling="affine", LU_decomposed=False,
        num_dequant_blocks=0, coupling_network="tanh", coupling_network_depth=1, batch_norm=True)
    m = BoostedFlow(args)
    with pytest.raises(ValueError):
        m.numerics_status(direction="sideways")
    with pytest.raises(ValueError):
        BoostedImageFlow.numerics_status(object(), direction="sideways")      # refused before the module is looked at
