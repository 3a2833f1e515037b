"""CPU: the fused training step's part of the C ABI -- declared in include/gbnf.h, listed and bound in native.py, exported by the
library (no compute calls)."""
import ctypes
import os
import re

from conftest import REPO
from gbnf_amd import native

NEW_SYMBOLS = ("gbnf_trainer_apply_update", "gbnf_trainer_step_workspace_bytes", "gbnf_trainer_nll_step")


def _header():
    return re.sub(r"/\*.*?\*/", "", open(os.path.join(REPO, "include", "gbnf.h")).read(), flags=re.S)


def test_header_declares_and_binding_lists_the_step_symbols():
    declared = set(re.findall(r"\b(gbnf_[a-z_]+)\s*\(", _header()))
    for name in NEW_SYMBOLS:
        assert name in declared, f"{name} is not declared in include/gbnf.h"
        assert name in native.ABI_SYMBOLS, f"{name} is not in native.ABI_SYMBOLS"
    assert "#define GBNF_ABI_VERSION 4" in _header()


def test_opt_hyper_mirror_matches_the_header():
    assert ctypes.sizeof(native._OptHyper) == 48
    # field order and types as declared (LP64): two int32, one int64, eight floats
    body = re.search(r"typedef struct gbnf_opt_hyper \{(.*?)\} gbnf_opt_hyper;", _header(), flags=re.S).group(1)
    declared = []
    for typ, names in re.findall(r"\b(int32_t|int64_t|float)\s+([a-z0-9_,\s]+);", body):
        declared += [(n.strip(), typ) for n in names.split(",")]
    ctype = {"int32_t": ctypes.c_int32, "int64_t": ctypes.c_int64, "float": ctypes.c_float}
    assert [(n, ctype[t]) for n, t in declared] == list(native._OptHyper._fields_)
    assert native._OptHyper.step.offset == 8 and native._OptHyper.lr.offset == 16 and native._OptHyper.bn_momentum.offset == 40
    enum = re.search(r"enum \{ GBNF_OPT_SGD = (\d+), GBNF_OPT_ADAMW = (\d+) \};", _header())
    assert native.OPT_KIND == {"sgd": int(enum.group(1)), "adamw": int(enum.group(2))}


def test_library_exports_and_binds_the_step_symbols():
    assert os.path.exists(native.LIB_PATH), "build the library first: python __graft_entry__.py"
    raw = ctypes.CDLL(native.LIB_PATH)
    for name in NEW_SYMBOLS:
        assert hasattr(raw, name), f"{name} missing from libgbnf_hip.so"
    L = native.lib()                       # dlopen + symbol binding only; touches no device
    assert len(L.gbnf_trainer_apply_update.argtypes) == 7
    assert len(L.gbnf_trainer_step_workspace_bytes.argtypes) == 3
    assert len(L.gbnf_trainer_nll_step.argtypes) == 13
