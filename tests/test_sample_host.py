"""Drawing from the mixture (gbnf_mixture_sample_begin / _finish), host part: the entry points exist and refuse bad arguments without a
device, the workspace formula, and the preconditions of the case lists that tests/test_hip_sample.py runs on the GPU.

A case: C components synth.synth_boosted_specs(kind, C, d, h, K, seed=41), decreasing rho, u = RandomState(9000 + n).random_sample(n)
as float32, x = synth_batch(n, d, 77 + n), and z = float32(float64 forward of row i under the component drawn for it).  Two
conditions make the GPU tests' bars (X_BAR / ILD_BAR of tests/test_hip_inverse.py) and their exact comparison of `comp` sound:

  1. the float32 oracle inverse -- the reference's own arithmetic -- stays within a third of each bar of the float64 oracle;
  2. every u[i] * T lies at least 1e-6 * T away from every cdf edge: no draw is decided by a rounding.
"""
import ctypes as C
import os
import re

import numpy as np
import pytest

from gbnf_amd import native, synth
from test_hip_inverse import ILD_BAR, X_BAR

REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
SAMPLE_SYMBOLS = ("gbnf_mixture_sample_workspace_bytes", "gbnf_mixture_sample_begin", "gbnf_mixture_sample_finish")
CHUNK = 1024              # rows per workgroup of the partition kernels (SAMPLE_CHUNK, csrc/gbnf_sample.hip)
EDGE_MARGIN = 1e-6

# (name, kind, C, d, h, K, synth keywords)
GEOMETRIES = [
    ("glow-c3-d43-h64-k2", "glow", 3, 43, 64, 2, {}),
    ("realnvp-c4-d21-h64-k2", "realnvp", 4, 21, 64, 2, {}),
    ("glow-c2-d6-h30-k3-additive-reverse", "glow", 2, 6, 30, 3, dict(coupling="additive", permutation="reverse")),
    ("realnvp-c8-d21-h105-k2", "realnvp", 8, 21, 105, 2, {}),
]
NS = (1, 2, 17, 100, 1000)
CASES = [(g, n) for g in GEOMETRIES for n in NS]


def case_id(case):
    return f"{case[0][0]}-n{case[1]}"


def decreasing_rho(n_components):
    """models/boosted_flow.py:32-36, rho_init == "decreasing"."""
    return np.maximum(1.0 / np.power(2.0, np.arange(n_components, dtype=np.float64)), 0.05).astype(np.float32)


def uniforms(n):
    return np.random.RandomState(9000 + n).random_sample(n).astype(np.float32)


def numpy_draw(rho, u, n_used=None):
    """The rule of gbnf_resample_rows on w = rho[0:n_used], restated: (comp, cdf).  In contract only (u in [0,1), a positive total)."""
    w = np.asarray(rho, dtype=np.float32)[: len(rho) if n_used is None else n_used]
    cdf = np.cumsum(np.where((w > 0) & np.isfinite(w), w, 0).astype(np.float64))
    target = np.asarray(u, dtype=np.float32).astype(np.float64) * cdf[-1]
    return np.searchsorted(cdf, target, side="right").astype(np.int32), cdf


def edge_margin(rho, u, n_used=None):
    """min over rows and edges of |u[i] * T - cdf_c| / T"""
    _, cdf = numpy_draw(rho, u, n_used)
    target = np.asarray(u, dtype=np.float32).astype(np.float64) * cdf[-1]
    edges = np.concatenate([[0.0], cdf])
    return float(np.abs(target[:, None] - edges[None, :]).min() / cdf[-1])


def workspace_bytes(n_flows, n, d):
    """include/gbnf.h: sorted z, x and ldj of n + 64 n_flows rows, the chunk histograms, the draw's cdf, each rounded up to 256 bytes."""
    up = lambda b: (b + 255) // 256 * 256
    rows = n + 64 * n_flows
    return 2 * up(4 * rows * d) + up(4 * rows) + up(8 * ((n + CHUNK - 1) // CHUNK) * n_flows) + up(8 * n_flows)


_SPECS, _REFS = {}, {}


def specs_of(geometry):
    name, kind, n_components, d, h, K, kw = geometry
    if name not in _SPECS:
        _SPECS[name] = synth.synth_boosted_specs(kind, n_components, d, h, K, seed=41, **kw)
    return _SPECS[name]


def mixture_reference(specs, rho, u, n, seed, key):
    """(comp, z float32, x64, ild64) for `n` rows: computed once per process under `key`, shared, never written to."""
    if key not in _REFS:
        from oracle import gbnf_oracle as oracle
        d = specs[0]["d"]
        comp, _ = numpy_draw(rho, u)
        x = synth.synth_batch(n, d, seed)
        z = np.zeros((n, d), dtype=np.float32)
        x64, ild64 = np.zeros((n, d)), np.zeros(n)
        for c in range(len(rho)):
            rows = np.nonzero(comp == c)[0]
            if rows.size:
                z[rows] = oracle.component_forward(specs[c], x[rows], backend="numpy64")[0].astype(np.float32)
                x64[rows], ild64[rows] = oracle.component_inverse(specs[c], z[rows].copy(), backend="numpy64")
        for a in (comp, z, x64, ild64):
            a.setflags(write=False)
        _REFS[key] = (comp, z, x64, ild64)
    return _REFS[key]


def case_reference(case):
    """(specs, rho, u, comp, z, x64, ild64) of a (geometry, n) case."""
    geometry, n = case
    specs = specs_of(geometry)
    rho, u = decreasing_rho(len(specs)), uniforms(n)
    return (specs, rho, u) + mixture_reference(specs, rho, u, n, 77 + n, case_id(case))


# ------------------------------------------------------------------ the ABI
def test_new_symbols_are_declared_bound_and_exported():
    text = open(os.path.join(REPO, "include", "gbnf.h")).read()
    assert re.search(r"#define\s+GBNF_ABI_VERSION\s+4\b", text)
    code = " ".join(re.sub(r"/\*.*?\*/", "", text, flags=re.S).split())
    declared = set(re.findall(r"\b(gbnf_[a-z_]+)\s*\(", code))
    L = native.lib()
    raw = C.CDLL(native.LIB_PATH)
    for name in SAMPLE_SYMBOLS:
        assert name in declared, f"{name} is not declared in include/gbnf.h"
        assert name in native.ABI_SYMBOLS
        assert hasattr(raw, name), f"{name} missing from libgbnf_hip.so"
        assert getattr(L, name).argtypes, f"{name} has no argument types in native.lib()"
    assert "int gbnf_mixture_sample_workspace_bytes(int32_t n_flows, int64_t n, int32_t d, int64_t* bytes);" in code
    assert ("int gbnf_mixture_sample_begin(const float* rho_dev, int32_t n_used, const float* u, const float* z_or_null, int64_t n, "
            "int32_t d, int32_t* comp, int64_t* order, int64_t* counts_dev, void* workspace, int64_t workspace_bytes, void* stream);") in code
    assert ("int gbnf_mixture_sample_finish(gbnf_flow* const* flows, int32_t n_flows, const int64_t* counts_host, const int64_t* order, "
            "int64_t n, float* x, float* ldj_or_null, void* workspace, int64_t workspace_bytes, void* stream);") in code
    assert L.gbnf_version() == 4
    assert callable(native.mixture_sample)


def test_header_states_what_the_calls_replace_and_the_rule():
    text = open(os.path.join(REPO, "include", "gbnf.h")).read()
    block = text[text.index("drawing from the mixture"):text.index("int gbnf_mixture_sample_workspace_bytes")]
    for needle in ("models/boosted_flow.py:209-218", ":61-96", "cdf_c = sum_{k <= c} max(rho_k, 0)", "the smallest c with (double)u[i] * T < cdf_c",
                   "roundup64", "GBNF_ERR_INVALID"):
        assert needle in block, needle


def test_entry_points_refuse_bad_arguments_without_a_device():
    L = native.lib()
    nb = C.c_int64(-7)
    buf = (C.c_float * 64)()          # host memory: a refused call never touches it
    p = C.cast(buf, C.c_void_p)
    null_entry = (C.c_void_p * 2)(None, None)
    counts = (C.c_int64 * 2)(8, 8)
    calls = [
        ("workspace, null bytes", lambda: L.gbnf_mixture_sample_workspace_bytes(2, 16, 4, None)),
        ("workspace, n_flows = 0", lambda: L.gbnf_mixture_sample_workspace_bytes(0, 16, 4, C.byref(nb))),
        ("workspace, n = 0", lambda: L.gbnf_mixture_sample_workspace_bytes(2, 0, 4, C.byref(nb))),
        ("workspace, d = 0", lambda: L.gbnf_mixture_sample_workspace_bytes(2, 16, 0, C.byref(nb))),
        ("begin, all null", lambda: L.gbnf_mixture_sample_begin(None, 2, None, None, 16, 4, None, None, None, None, 0, None)),
        ("begin, null rho", lambda: L.gbnf_mixture_sample_begin(None, 2, p, p, 16, 4, p, p, p, p, 1 << 20, None)),
        ("begin, null u", lambda: L.gbnf_mixture_sample_begin(p, 2, None, p, 16, 4, p, p, p, p, 1 << 20, None)),
        ("begin, null comp", lambda: L.gbnf_mixture_sample_begin(p, 2, p, p, 16, 4, None, p, p, p, 1 << 20, None)),
        ("begin, null order", lambda: L.gbnf_mixture_sample_begin(p, 2, p, p, 16, 4, p, None, p, p, 1 << 20, None)),
        ("begin, null counts", lambda: L.gbnf_mixture_sample_begin(p, 2, p, p, 16, 4, p, p, None, p, 1 << 20, None)),
        ("begin, null workspace", lambda: L.gbnf_mixture_sample_begin(p, 2, p, p, 16, 4, p, p, p, None, 1 << 20, None)),
        ("begin, n = 0", lambda: L.gbnf_mixture_sample_begin(p, 2, p, p, 0, 4, p, p, p, p, 1 << 20, None)),
        ("begin, n_used = 0", lambda: L.gbnf_mixture_sample_begin(p, 0, p, p, 16, 4, p, p, p, p, 1 << 20, None)),
        ("begin, short workspace", lambda: L.gbnf_mixture_sample_begin(p, 2, p, p, 16, 4, p, p, p, p, workspace_bytes(2, 16, 4) - 1, None)),
        ("finish, all null", lambda: L.gbnf_mixture_sample_finish(None, 2, None, None, 16, None, None, None, 0, None)),
        ("finish, null flows", lambda: L.gbnf_mixture_sample_finish(None, 2, counts, p, 16, p, p, p, 1 << 20, None)),
        ("finish, null entry", lambda: L.gbnf_mixture_sample_finish(null_entry, 2, counts, p, 16, p, p, p, 1 << 20, None)),
        ("finish, null counts", lambda: L.gbnf_mixture_sample_finish(null_entry, 2, None, p, 16, p, p, p, 1 << 20, None)),
        ("finish, n = 0", lambda: L.gbnf_mixture_sample_finish(null_entry, 2, counts, p, 0, p, p, p, 1 << 20, None)),
        ("finish, n_flows = 0", lambda: L.gbnf_mixture_sample_finish(null_entry, 0, counts, p, 16, p, p, p, 1 << 20, None)),
    ]
    for what, call in calls:
        assert call() == -1, f"{what}: accepted"
        assert L.gbnf_last_error(), f"{what}: no message"
    assert nb.value == -7 and not any(buf)


@pytest.mark.parametrize("n_flows,n,d", [(1, 1, 1), (3, 17, 43), (8, 1000, 21), (8, 1024, 43), (8, 1025, 43), (2, 70001, 6), (8, 65536, 43)])
def test_workspace_is_the_sum_of_its_aligned_pieces(n_flows, n, d):
    nb = C.c_int64()
    assert native.lib().gbnf_mixture_sample_workspace_bytes(n_flows, n, d, C.byref(nb)) == 0
    assert nb.value == workspace_bytes(n_flows, n, d) and nb.value % 256 == 0


# ------------------------------------------------------------------ the case lists
def test_numpy_draw_is_the_documented_rule():
    rho = np.array([1.0, 0.5, 0.0, 0.25], dtype=np.float32)
    comp, cdf = numpy_draw(rho, np.array([0.0, 0.5, 0.58, 0.86, 0.999], dtype=np.float32))
    assert cdf.tolist() == [1.0, 1.5, 1.5, 1.75]
    assert comp.tolist() == [0, 0, 1, 3, 3]                 # the zero-weight component 2 is passed over
    assert numpy_draw(rho, np.array([0.7], dtype=np.float32), n_used=2)[0].tolist() == [1]


@pytest.mark.parametrize("case", CASES, ids=case_id)
def test_case_preconditions(case):
    from oracle import gbnf_oracle as oracle
    specs, rho, u, comp, z, x64, ild64 = case_reference(case)
    n = case[1]
    assert comp.shape == (n,) and comp.min() >= 0 and comp.max() < len(specs)
    margin = edge_margin(rho, u)
    x32, ild32 = np.zeros_like(x64), np.zeros_like(ild64)
    for c in range(len(specs)):
        rows = np.nonzero(comp == c)[0]
        if rows.size:
            a, b = oracle.component_inverse(specs[c], z[rows].copy(), backend="torch")
            x32[rows], ild32[rows] = a, b
    dx = float(np.abs(x32 - x64).max()) / max(1.0, float(np.abs(x64).max()))
    dl = float(np.abs(ild32 - ild64).max()) / max(1.0, float(np.abs(ild64).max()))
    print(f"PRECOND {case_id(case)} f32-oracle dx {dx:.3e} dild {dl:.3e} edge margin {margin:.3e} counts {np.bincount(comp, minlength=len(specs)).tolist()}")
    assert dx <= X_BAR / 3.0, dx
    assert dl <= ILD_BAR / 3.0, dl
    assert margin >= EDGE_MARGIN, margin
    assert float(np.abs(z).max()) < 65504.0


def test_case_lists_cover_what_they_are_for():
    """An empty segment occurs without being arranged, every component is drawn somewhere, and n = 1 is there."""
    counts = {case_id(c): np.bincount(case_reference(c)[3], minlength=len(specs_of(c[0]))) for c in CASES}
    assert any((k == 0).any() and k.sum() >= 17 for k in counts.values())
    for g in GEOMETRIES:
        assert (counts[case_id((g, 1000))] > 0).all()
    assert counts["realnvp-c4-d21-h64-k2-n17"][3] == 0
