"""CPU: the host side of the trainer's math modes -- which bf16x6 training sweeps the build compiles (csrc/variants.list `safe`
lines), how the drop-in module picks the mode (args.train_math, env GBNF_TRAIN_MATH), what the binding accepts.  No device work."""
import argparse
import os
import sys

import pytest
import torch

from conftest import REPO
from gbnf_amd import native
from gbnf_amd.boosted_flow import BoostedFlow

CSRC = os.path.join(REPO, "gradient-boosted-normalizing-flows_amd", "csrc")

# (kind, ht, ot, act_a, act_b, depth): the geometries a range-safe trainer must find -- the generic supersets of Glow and RealNVP with
# the activation per step at depths 0, 1, 2 (h <= 256), the one-block ResidualNet (h <= 256) and the two BASELINE geometries
REQUIRED = [(0, 16, 4, 3, 3, 0), (0, 16, 4, 3, 3, 1), (0, 16, 4, 3, 3, 2), (1, 16, 2, 3, 3, 0), (1, 16, 2, 3, 3, 1), (1, 16, 2, 3, 3, 2),
            (1, 16, 2, 2, 2, 2), (0, 14, 3, 0, 0, 1), (1, 7, 1, 0, 0, 1)]


def _variants():
    sys.path.insert(0, CSRC)
    import build
    return build.read_variants()


@pytest.mark.parametrize("key", REQUIRED)
def test_build_lists_the_bf16x6_training_sweeps(key):
    kind, ht, ot, a, b, depth = key
    v = _variants()
    for nt in (1, 2):
        assert ("hx3t", kind, ht, ot, nt, a, b, 1, depth) in v, f"no bf16x6 forward sweep (NT = {nt}) for {key}"
    assert ("hx3b", kind, ht, ot, a, b, depth, 1) in v, f"no bf16x6 backward sweep for {key}"
    # ... next to the f16x3 sweeps and the evaluation kernels of the same geometry (the `hx3` line the `safe` line names)
    assert ("hx3t", kind, ht, ot, 1, a, b, 0, depth) in v and ("hx3b", kind, ht, ot, a, b, depth) in v
    assert ("hx3", kind, ht, ot, 1, a, b, 1, depth) in v


def test_safe_sweeps_are_built_for_listed_lines_only():
    v = _variants()
    safe_b = [t for t in v if t[0] == "hx3b" and len(t) == 8]
    safe_t = [t for t in v if t[0] == "hx3t" and t[7] == 1]
    assert len(safe_b) == len(REQUIRED) and len(safe_t) == 2 * len(REQUIRED)
    assert all(t[-1] == 1 for t in safe_b)
    assert len({str(t) for t in v}) == len(v)            # object names stay unique


def _args(**kw):
    ns = argparse.Namespace(
        num_flows=3, z_size=7, density_evaluation=True, device=torch.device("cpu"), cuda=False, component_type="glow",
        num_components=2, rho_init="decreasing", learn_top=False, y_classes=0, y_condition=False, sample_size=4, input_size=[7],
        h_size=12, num_blocks=1, actnorm_scale=1.0, flow_permutation="shuffle", flow_coupling="affine", LU_decomposed=False,
        num_dequant_blocks=0, coupling_network="tanh", coupling_network_depth=1, batch_norm=True)
    for k, val in kw.items():
        setattr(ns, k, val)
    return ns


def test_train_math_defaults_to_the_saturating_trainer(monkeypatch):
    monkeypatch.delenv("GBNF_TRAIN_MATH", raising=False)
    assert BoostedFlow(_args()).train_math == "f16x3"
    assert BoostedFlow(_args(train_math=None)).train_math == "f16x3"


@pytest.mark.parametrize("value", ["f16x3", "bf16x6", "repair"])
def test_train_math_argument_is_taken(monkeypatch, value):
    monkeypatch.setenv("GBNF_TRAIN_MATH", "f16x3" if value != "f16x3" else "bf16x6")      # the argument wins over the environment
    assert BoostedFlow(_args(train_math=value)).train_math == value


def test_train_math_environment_is_honoured(monkeypatch):
    monkeypatch.setenv("GBNF_TRAIN_MATH", "bf16x6")
    assert BoostedFlow(_args()).train_math == "bf16x6"
    monkeypatch.setenv("GBNF_TRAIN_MATH", "f64")
    with pytest.raises(ValueError, match="train_math"):
        BoostedFlow(_args())


@pytest.mark.parametrize("value", ["f32", "default", "BF16X6", "fast", 3])
def test_unknown_train_math_raises_at_construction(monkeypatch, value):
    monkeypatch.delenv("GBNF_TRAIN_MATH", raising=False)
    with pytest.raises(ValueError, match="train_math"):
        BoostedFlow(_args(train_math=value))


def test_binding_names_the_three_modes_and_refuses_the_rest():
    assert native.NativeTrainer.TRAIN_MATH == {"f16x3": native.MATH["f16x3"], "bf16x6": native.MATH["bf16x6"],
                                               "repair": native.MATH["default"]}
    for bad in ("f32", "default", None):
        with pytest.raises(native.GbnfError, match="math"):        # checked before the spec is looked at, before any device work
            native.NativeTrainer({}, math=bad)
    assert {"gbnf_trainer_create_mode", "gbnf_trainer_repair_count"} <= set(native.ABI_SYMBOLS)


def test_a_safe_line_must_name_a_training_hx3_line(tmp_path, monkeypatch):
    """csrc/build.py refuses a `safe` line without an `hx3` line of the same geometry that builds training sweeps."""
    sys.path.insert(0, CSRC)
    import build
    text = open(os.path.join(CSRC, "variants.list")).read()
    for extra in ("safe 0 5 3 0 0", "safe 1 24 2 2 2 4"):        # no such hx3 line; an `eval` line
        (tmp_path / "variants.list").write_text(text + "\n" + extra + "\n")
        monkeypatch.setattr(build, "HERE", str(tmp_path))
        with pytest.raises(ValueError, match="names no `hx3` line"):
            build.read_variants()
