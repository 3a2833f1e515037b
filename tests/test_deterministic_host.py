"""CPU: the host side of deterministic training mode -- the header and the binding agree on the new entry points, the module-level
flag (``args.deterministic`` / env GBNF_DETERMINISTIC) parses and refuses a wrong value, and every workspace helper of
``native.NativeTrainer`` asks the library for the size again after the mode is switched (the library calls are mocked)."""
import argparse
import ctypes as C
import os
import re

import pytest

from conftest import REPO
from gbnf_amd import native
from gbnf_amd.boosted_flow import deterministic_from

NEW = ("gbnf_trainer_set_deterministic", "gbnf_trainer_get_deterministic")


def test_header_and_binding_have_the_entry_points():
    text = open(os.path.join(REPO, "include", "gbnf.h")).read()
    text = re.sub(r"/\*.*?\*/", "", text, flags=re.S)
    declared = set(re.findall(r"\b(gbnf_[a-z_]+)\s*\(", text))
    for name in NEW:
        assert name in declared and name in native.ABI_SYMBOLS
    assert declared == set(native.ABI_SYMBOLS)
    assert re.search(r"#define\s+GBNF_ABI_VERSION\s+4\b", open(os.path.join(REPO, "include", "gbnf.h")).read())


def test_library_exports_them():
    lib = C.CDLL(native.LIB_PATH)
    for name in NEW:
        assert hasattr(lib, name)


def test_flag_from_args_and_environment():
    ns = argparse.Namespace
    assert deterministic_from(ns(), env={}) is False
    assert deterministic_from(ns(deterministic=None), env={"GBNF_DETERMINISTIC": "1"}) is True
    assert deterministic_from(ns(), env={"GBNF_DETERMINISTIC": "0"}) is False
    assert deterministic_from(ns(), env={"GBNF_DETERMINISTIC": ""}) is False
    assert deterministic_from(ns(deterministic=True), env={"GBNF_DETERMINISTIC": "0"}) is True       # args win
    assert deterministic_from(ns(deterministic=False), env={"GBNF_DETERMINISTIC": "1"}) is False
    for bad in ("yes", "true", "2", " 1"):
        with pytest.raises(ValueError):
            deterministic_from(ns(), env={"GBNF_DETERMINISTIC": bad})
    for bad in ("1", 2, 0.5):
        with pytest.raises(ValueError):
            deterministic_from(ns(deterministic=bad), env={})


def test_flag_reads_the_process_environment(monkeypatch):
    monkeypatch.setenv("GBNF_DETERMINISTIC", "1")
    assert deterministic_from(argparse.Namespace()) is True
    monkeypatch.setenv("GBNF_DETERMINISTIC", "maybe")
    with pytest.raises(ValueError):
        deterministic_from(argparse.Namespace())
    monkeypatch.delenv("GBNF_DETERMINISTIC")
    assert deterministic_from(argparse.Namespace()) is False


class _FakeLib:
    """Stands in for the library behind a NativeTrainer: reports a larger size while the mode is on, records every size query and the
    workspace (address, bytes) every compute call was handed."""
    SMALL, LARGE = 4096, 16384

    def __init__(self):
        self.on = 0
        self.queries = []
        self.calls = []

    def gbnf_trainer_set_deterministic(self, handle, on):
        self.on = int(on)
        return 0

    def gbnf_trainer_get_deterministic(self, handle, out):
        out._obj.value = self.on
        return 0

    def _size(self, name, out):
        self.queries.append((name, self.on))
        out._obj.value = self.LARGE if self.on else self.SMALL
        return 0

    def gbnf_trainer_workspace_bytes(self, handle, n, out):
        return self._size("backward", out)

    def gbnf_trainer_step_workspace_bytes(self, handle, n, out):
        return self._size("nll_step", out)

    def gbnf_boosted_step_workspace_bytes(self, mixture, n_fixed, handle, n, out):
        return self._size("boosted_nll_step", out)

    # (the workspace pointer and its size: arguments 8, 9 of gbnf_trainer_backward, 10, 11 of gbnf_trainer_nll_step, 14, 15 of
    #  gbnf_boosted_nll_step -- include/gbnf.h)
    def gbnf_trainer_backward(self, *a):
        self.calls.append(("backward", a[8].value, a[9]))
        return 0

    def gbnf_trainer_nll_step(self, *a):
        self.calls.append(("nll_step", a[10].value, a[11]))
        return 0

    def gbnf_boosted_nll_step(self, *a):
        self.calls.append(("boosted_nll_step", a[14].value, a[15]))
        return 0


class _State:
    """The part of native.OptState the step helpers use."""
    kind, step = "adamw", 0

    def __init__(self, floats):
        import torch
        self.exp_avg, self.exp_avg_sq = torch.zeros(floats), torch.zeros(floats)

    def check(self, trainer):
        pass


class _Mixture:
    handle = C.c_void_p(2)


def _fake_trainer(monkeypatch):
    """A NativeTrainer of d = 3 with one 6-float parameter, on host tensors, in front of the fake library."""
    import torch
    fake = _FakeLib()
    monkeypatch.setattr(native, "lib", lambda: fake)
    monkeypatch.setattr(native, "_require_device_f32", lambda t, name: t)
    monkeypatch.setattr(native, "_stream_ptr", lambda: None)
    tr = native.NativeTrainer.__new__(native.NativeTrainer)
    tr.handle = C.c_void_p(1)
    tr.d, tr.grad_floats = 3, 6
    tr.params, tr._sizes = [torch.zeros(2, 3)], [6]
    tr._ws = tr._step_ws = tr._boost_ws = None
    tr.device = torch.device("cpu")
    tr._deterministic = False
    return fake, tr


def test_the_property_goes_through_the_library(monkeypatch):
    fake, tr = _fake_trainer(monkeypatch)
    assert tr.deterministic is False
    tr.deterministic = True
    assert fake.on == 1 and tr.deterministic is True and tr._deterministic is True
    tr.deterministic = False
    assert fake.on == 0 and tr.deterministic is False and tr._deterministic is False
    tr.handle = None          # (nothing to destroy)


@pytest.mark.parametrize("helper", ["backward", "nll_step", "boosted_nll_step"])
def test_workspace_helpers_requery_after_a_switch(monkeypatch, helper):
    """Off -> on -> off: every call asks the library for the size under the mode then in force, the call after the switch gets a new,
    larger workspace (never the cached small one), and the large one is kept when the mode goes off again."""
    import torch
    fake, tr = _fake_trainer(monkeypatch)
    x = torch.zeros(8, 3)

    def call():
        if helper == "backward":
            tr.backward(x, torch.zeros(8, 3), None)
        elif helper == "nll_step":
            tr.nll_step(x, _State(6), lr=1e-3)
        else:
            tr.boosted_nll_step(_Mixture(), 1, torch.ones(2), x, torch.zeros(8), _State(6), lr=1e-3)
        return fake.calls[-1]

    name, small_ptr, small_bytes = call()
    assert name == helper and fake.queries[-1] == (helper, 0)
    assert small_bytes >= fake.SMALL and small_bytes < fake.LARGE
    tr.deterministic = True
    _, large_ptr, large_bytes = call()
    assert fake.queries[-1] == (helper, 1), "the size was not asked for again after the switch"
    assert large_bytes >= fake.LARGE, "the workspace sized before the switch was handed to the library again"
    assert large_ptr != small_ptr
    tr.deterministic = False
    _, ptr, nbytes = call()
    assert fake.queries[-1] == (helper, 0) and len(fake.queries) == 3
    assert (ptr, nbytes) == (large_ptr, large_bytes)          # large enough: kept
    tr.handle = None
