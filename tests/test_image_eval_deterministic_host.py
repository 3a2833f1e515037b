"""CPU: the host side of the image evaluation handles' deterministic mode -- the header, the binding and the built library agree on
the two new entry points, the module-level flag (``args.image_eval_deterministic`` / env GBNF_IMAGE_EVAL_DETERMINISTIC) parses and
refuses a wrong value, none of the three determinism flags reads another, ``native.NativeImageFlow.deterministic`` goes through the
library (mocked) and ``BoostedImageFlow.native_flow`` applies the module's flag to cached handles.  The GPU side is
tests/test_hip_image_eval_deterministic.py."""
import argparse
import ctypes as C
import os
import re

import pytest

from conftest import REPO
from gbnf_amd import native
from gbnf_amd.boosted_flow import deterministic_from, image_deterministic_from, image_eval_deterministic_from

NEW = ("gbnf_image_flow_set_deterministic", "gbnf_image_flow_get_deterministic")
VAR = "GBNF_IMAGE_EVAL_DETERMINISTIC"


def _header():
    return open(os.path.join(REPO, "include", "gbnf.h")).read()


def test_header_binding_and_library_have_the_entry_points():
    text = re.sub(r"/\*.*?\*/", "", _header(), flags=re.S)
    declared = set(re.findall(r"\b(gbnf_[a-z_]+)\s*\(", text))
    for name in NEW:
        assert name in declared and name in native.ABI_SYMBOLS
    assert declared == set(native.ABI_SYMBOLS)
    assert re.search(r"#define\s+GBNF_ABI_VERSION\s+4\b", _header())
    lib = C.CDLL(native.LIB_PATH)
    for name in NEW:
        assert hasattr(lib, name)


def test_header_no_longer_excludes_the_evaluation_handles():
    text = _header()
    assert "the evaluation path has no such mode" not in text
    assert "whose kernels keep their atomics" not in text
    # ... and says what a captured graph does with a later switch, next to the declaration
    at = text.index("int gbnf_image_flow_set_deterministic")
    assert "captured graph" in text[max(0, at - 3000):at]


def test_flag_from_args_and_environment():
    ns = argparse.Namespace
    assert image_eval_deterministic_from(ns(), env={}) is False
    assert image_eval_deterministic_from(ns(image_eval_deterministic=None), env={VAR: "1"}) is True
    assert image_eval_deterministic_from(ns(), env={VAR: "0"}) is False
    assert image_eval_deterministic_from(ns(), env={VAR: ""}) is False
    assert image_eval_deterministic_from(ns(image_eval_deterministic=True), env={VAR: "0"}) is True       # args win
    assert image_eval_deterministic_from(ns(image_eval_deterministic=False), env={VAR: "1"}) is False
    for bad in ("yes", "true", "2", " 1"):
        with pytest.raises(ValueError, match=VAR):
            image_eval_deterministic_from(ns(), env={VAR: bad})
    for bad in ("1", 2, 0.5):
        with pytest.raises(ValueError):
            image_eval_deterministic_from(ns(image_eval_deterministic=bad), env={})


def test_flag_reads_the_process_environment(monkeypatch):
    monkeypatch.setenv(VAR, "1")
    assert image_eval_deterministic_from(argparse.Namespace()) is True
    monkeypatch.setenv(VAR, "maybe")
    with pytest.raises(ValueError, match=VAR):
        image_eval_deterministic_from(argparse.Namespace())
    monkeypatch.delenv(VAR)
    assert image_eval_deterministic_from(argparse.Namespace()) is False


def test_the_three_flags_do_not_read_each_other():
    ns = argparse.Namespace
    others = {"GBNF_DETERMINISTIC": "1", "GBNF_IMAGE_DETERMINISTIC": "1"}
    assert image_eval_deterministic_from(ns(deterministic=True, image_deterministic=True), env=others) is False
    assert deterministic_from(ns(image_eval_deterministic=True), env={VAR: "1"}) is False
    assert image_deterministic_from(ns(image_eval_deterministic=True), env={VAR: "1"}) is False
    assert image_deterministic_from(ns(deterministic=True), env={"GBNF_DETERMINISTIC": "1"}) is False        # (as before)
    assert deterministic_from(ns(image_deterministic=True), env={"GBNF_IMAGE_DETERMINISTIC": "1"}) is False
    with pytest.raises(ValueError, match=VAR):
        image_eval_deterministic_from(ns(), env={VAR: "on"})
    with pytest.raises(ValueError, match="GBNF_IMAGE_DETERMINISTIC"):      # (the other two flags' behaviour is unchanged)
        image_deterministic_from(ns(), env={"GBNF_IMAGE_DETERMINISTIC": "on", VAR: "1"})
    with pytest.raises(ValueError, match="GBNF_DETERMINISTIC"):
        deterministic_from(ns(), env={"GBNF_DETERMINISTIC": "on", VAR: "1"})
    # a wrong value of one flag's variable does not disturb the others
    assert deterministic_from(ns(), env={VAR: "on"}) is False and image_deterministic_from(ns(), env={VAR: "on"}) is False


class _FakeLib:
    """Stands in for the library behind a NativeImageFlow: keeps the flag, reports a larger workspace while it is on."""
    SMALL, LARGE = 4096, 16384

    def __init__(self):
        self.on = 0
        self.calls = []

    def gbnf_image_flow_set_deterministic(self, handle, on):
        self.calls.append(("set", int(on)))
        self.on = int(on)
        return 0

    def gbnf_image_flow_get_deterministic(self, handle, out):
        out._obj.value = self.on
        return 0

    def gbnf_image_flow_workspace_bytes(self, handle, n, out):
        self.calls.append(("workspace", self.on))
        out._obj.value = self.LARGE if self.on else self.SMALL
        return 0


def _fake_flow(monkeypatch):
    fake = _FakeLib()
    monkeypatch.setattr(native, "lib", lambda: fake)
    flow = native.NativeImageFlow.__new__(native.NativeImageFlow)
    flow.handle = C.c_void_p(1)
    flow._ws = None
    return fake, flow


def test_the_property_goes_through_the_library(monkeypatch):
    fake, flow = _fake_flow(monkeypatch)
    assert flow.deterministic is False
    flow.deterministic = True
    assert fake.on == 1 and flow.deterministic is True
    flow.deterministic = 0
    assert fake.on == 0 and flow.deterministic is False
    assert [c for c in fake.calls if c[0] == "set"] == [("set", 1), ("set", 0)]
    flow.handle = None          # (nothing to destroy)


def test_the_workspace_size_is_asked_in_the_current_mode(monkeypatch):
    """The cached workspace is re-sized after a switch: every size comes from the library, in the mode the handle has then."""
    fake, flow = _fake_flow(monkeypatch)
    assert flow.workspace_bytes(9) == fake.SMALL
    flow.deterministic = True
    assert flow.workspace_bytes(9) == fake.LARGE
    flow.deterministic = False
    assert flow.workspace_bytes(9) == fake.SMALL
    assert [c for c in fake.calls if c[0] == "workspace"] == [("workspace", 0), ("workspace", 1), ("workspace", 0)]
    flow.handle = None


def test_native_flow_applies_the_module_flag_to_cached_handles():
    """BoostedImageFlow.native_flow sets the handle's mode from ``image_eval_deterministic`` -- also on a handle cached before the
    flag changed -- and does not touch the library while handle and flag agree."""
    from gbnf_amd import image_glow

    class Handle:
        def __init__(self):
            self.sets = []

        @property
        def deterministic(self):
            return bool(self.sets and self.sets[-1])

        @deterministic.setter
        def deterministic(self, on):
            self.sets.append(bool(on))

    class Module:
        native_flow = image_glow.BoostedImageFlow.native_flow
        flows = [object()]

        def _component_tensors(self, c):
            return [], [], [], []

    m = Module()
    handle = Handle()
    m._handles = {0: ((), handle)}          # (the key of a component without tensors)
    m.image_eval_deterministic = False
    assert m.native_flow(0) is handle and handle.sets == []
    m.image_eval_deterministic = True
    assert m.native_flow(0) is handle and handle.sets == [True]
    assert m.native_flow(0) is handle and handle.sets == [True]
    m.image_eval_deterministic = False
    assert m.native_flow(0) is handle and handle.sets == [True, False]


def test_the_module_reads_the_flag_and_the_tool_has_the_switch():
    src = open(os.path.join(REPO, "gradient-boosted-normalizing-flows_amd", "image_glow.py")).read()
    assert "self.image_eval_deterministic = image_eval_deterministic_from(args)" in src
    tool = open(os.path.join(REPO, "tools", "bench_image.py")).read()
    assert "--eval-deterministic" in tool
