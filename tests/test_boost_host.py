"""CPU: the boosting entry points of the C ABI (csrc/gbnf_boost.hip) as far as they go without a device -- exports, the workspace
size, argument validation -- and the float64 numpy reference of the resampler that tests/test_hip_boost.py compares the kernels with,
checked here against its own exclusion margin and the frequency bound on the seeds both files use."""
import ctypes as C

import numpy as np
import pytest

from gbnf_amd import native

BOOST_SYMBOLS = ("gbnf_resample_workspace_bytes", "gbnf_resample_rows", "gbnf_boosted_step_workspace_bytes", "gbnf_boosted_nll_step",
                 "gbnf_mixture_rho_step")
# the wave (64), workgroup (1 024) and chunk (n > 1 024: more than one row per thread) edges of the scan kernel
SCAN_SIZES = (1, 63, 64, 65, 1023, 1024, 1025, 4099, 70001)
DRAW_COUNTS = (1, 5, 8192)
RESAMPLE_CASES = [(n, m) for n in SCAN_SIZES for m in DRAW_COUNTS if m != n]
MARGIN = 1e-9            # a draw whose u * T lies within MARGIN * T of a cdf entry is left out of a comparison
MAX_EXCLUDED = 1e-3      # ... and more than this fraction left out fails it
FREQ_N, FREQ_M = 64, 1 << 18


def case_seed(n, m):
    return 1000 * SCAN_SIZES.index(n) + DRAW_COUNTS.index(m)


def seeded_G(n, seed):
    """Mixture log-densities of a batch, as boosting sees them: around -20 with a spread of 3 nats."""
    return (np.random.RandomState(seed).standard_normal(n) * 3.0 - 20.0).astype(np.float32)


def seeded_uniforms(m, seed):
    u = np.random.RandomState(seed + 500000).random_sample(m).astype(np.float32)
    return np.minimum(u, np.nextafter(np.float32(1.0), np.float32(0.0)))       # (a double just below 1 rounds to 1.0f)


def numpy_boosting_weights(G, beta=1.0):
    """density_experiment.py:624-641 in float32 numpy."""
    a = (-G).astype(np.float32)
    e = np.exp(a - a.max())
    w = (e / e.sum(dtype=np.float32)).astype(np.float32)
    if beta != 1.0:
        w = np.power(w, np.float32(beta))
    if w.max() > 0.1:
        w = np.clip(w, np.float32(0.01), np.float32(0.1))
    s = w.sum(dtype=np.float32)
    if s != 1.0:
        w = w / s
    return w.astype(np.float32)


def shape_weights(w):
    """What the tests do to boosting weights: every 7th row gets none, and the sum is not 1."""
    w = (np.asarray(w, dtype=np.float32) * np.float32(0.75)).copy()
    w[6::7] = 0.0
    return w


def reference_cdf(w):
    w = np.asarray(w, dtype=np.float32)
    return np.cumsum(np.where(np.isfinite(w) & (w > 0), w, np.float32(0.0)).astype(np.float64))


def reference_rows(w, u):
    """The definition in float64: rows = searchsorted(cumsum(max(w, 0)), u * T, side="right"), and the mask of the draws whose
    u * T lies within MARGIN * T of a cdf entry (either neighbour)."""
    cdf = reference_cdf(w)
    T = cdf[-1]
    target = np.asarray(u, dtype=np.float32).astype(np.float64) * T
    rows = np.searchsorted(cdf, target, side="right")
    above = cdf[np.minimum(rows, cdf.size - 1)] - target
    below = np.where(rows > 0, target - cdf[np.maximum(rows - 1, 0)], np.inf)
    near = np.minimum(np.abs(above), np.abs(below)) <= MARGIN * T
    return rows.astype(np.int64), near


def frequency_violations(rows, w, m):
    """Rows whose count leaves the 6-sigma binomial bound |count_j - m p_j| <= 6 sqrt(m p_j (1 - p_j)) + 1, p = w / sum(w)."""
    p = reference_cdf(w)
    p = np.diff(np.concatenate([[0.0], p])) / p[-1]
    count = np.bincount(rows, minlength=p.size).astype(np.float64)
    return np.nonzero(np.abs(count - m * p) > 6.0 * np.sqrt(m * p * (1.0 - p)) + 1.0)[0]


def frequency_case():
    return shape_weights(numpy_boosting_weights(seeded_G(FREQ_N, 77))), seeded_uniforms(FREQ_M, 77)


def test_new_symbols_are_bound_and_exported():
    L = native.lib()
    for name in BOOST_SYMBOLS:
        assert name in native.ABI_SYMBOLS
        assert hasattr(L, name), f"{name} missing from libgbnf_hip.so"
    assert L.gbnf_version() == 4


@pytest.mark.parametrize("n", [1, 31, 32, 33, 4099, 70001])
def test_resample_workspace_is_the_double_cdf(n):
    nb = C.c_int64(-1)
    assert native.lib().gbnf_resample_workspace_bytes(n, C.byref(nb)) == 0
    assert nb.value == (8 * n + 255) // 256 * 256


def test_resample_rows_refuses_bad_arguments_without_a_device():
    L = native.lib()
    n, m = 40, 8
    w, u = (C.c_float * n)(), (C.c_float * m)()
    rows, ws = (C.c_int64 * m)(), (C.c_double * 64)()          # host memory: a refused call never touches it
    p = lambda a: C.cast(a, C.c_void_p)
    nb = C.c_int64()
    assert L.gbnf_resample_workspace_bytes(n, C.byref(nb)) == 0 and nb.value == 512
    bad = [(None, n, p(u), m, p(rows), p(ws), nb.value), (p(w), n, None, m, p(rows), p(ws), nb.value),
           (p(w), n, p(u), m, None, p(ws), nb.value), (p(w), n, p(u), m, p(rows), None, nb.value),
           (p(w), 0, p(u), m, p(rows), p(ws), nb.value), (p(w), n, p(u), 0, p(rows), p(ws), nb.value),
           (p(w), -3, p(u), m, p(rows), p(ws), nb.value), (p(w), n, p(u), m, p(rows), p(ws), nb.value - 1),
           (p(w), n, p(u), m, p(rows), p(ws), 0)]
    for k, a in enumerate(bad):
        assert L.gbnf_resample_rows(*a, None) == -1, f"bad call {k} was accepted"
        assert L.gbnf_last_error(), f"bad call {k} left no message"
    assert L.gbnf_resample_workspace_bytes(0, C.byref(nb)) == -1 and L.gbnf_resample_workspace_bytes(n, None) == -1
    assert not any(rows)


def test_the_other_entry_points_refuse_null_handles_without_a_device():
    L = native.lib()
    nb = C.c_int64()
    assert L.gbnf_boosted_step_workspace_bytes(None, 1, None, 16, C.byref(nb)) == -1
    assert L.gbnf_boosted_nll_step(None, 1, None, 1.0, None, None, 16, None, None, None, None, None, None, None, None, 0, None) == -1
    assert L.gbnf_mixture_rho_step(None, None, 16, 1, None, 0.1, None, None, None) == -1


@pytest.mark.parametrize("n,m", RESAMPLE_CASES)
def test_reference_stays_clear_of_its_exclusion_margin(n, m):
    """The seeds test_hip_boost.py uses: fewer than 0.1 % of the draws lie within the margin, rows are valid and never weightless."""
    w = shape_weights(numpy_boosting_weights(seeded_G(n, case_seed(n, m))))
    u = seeded_uniforms(m, case_seed(n, m))
    rows, near = reference_rows(w, u)
    print(f"n = {n}, m = {m}: {int(near.sum())} draws within the margin")
    assert near.sum() <= MAX_EXCLUDED * m
    assert rows.min() >= 0 and rows.max() < n and (w[rows] > 0).all()
    assert abs(float(w.sum(dtype=np.float64)) - 1.0) > 0.1


def test_reference_on_exact_uniform_weights():
    """w = 1/512 and u on multiples of 1/512: every operation is exact, u = k/512 belongs to row k (the strict <)."""
    w = np.full(512, 1.0 / 512, dtype=np.float32)
    u = (np.arange(512) / 512.0).astype(np.float32)
    rows, _ = reference_rows(w, u)
    assert (rows == np.arange(512)).all()


def test_reference_passes_the_frequency_bound():
    w, u = frequency_case()
    rows, _ = reference_rows(w, u)
    assert frequency_violations(rows, w, FREQ_M).size == 0
