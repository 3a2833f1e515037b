"""The synthetic case tables of the weight-fitting tests: component c is N(c * sep, 1) in one dimension, the rows are drawn from the
mixture with known weights, and the table ll[c][i] = log N(x_i; c * sep, 1) is stored as float32 -- what the library reads.

``evaluations``: how many evaluations the float64 yardstick (tests/weights_oracle.py) makes from uniform weights at TOL before it
stops, measured with these seeds and pinned here; None for the case that does not stop within MAX_ITERS updates (converged = 0).
tests/test_weights_host.py re-measures every count."""
import functools

import numpy as np

TOL = 1e-9
MAX_ITERS = 500
FIXED_UPDATES = 100

# name -> (C, N, true weights, sep, seed, evaluations)
CASES = {
    "c2_n257": (2, 257, (0.8, 0.2), 2.0, 11, 15),
    "c3_n4096": (3, 4096, (0.6, 0.3, 0.1), 2.0, 12, 15),
    "c5_n70001": (5, 70001, (0.4, 0.25, 0.2, 0.1, 0.05), 1.5, 13, 67),
    "c8_n1000": (8, 1000, (0.125,) * 8, 1.0, 14, None),
}
CONVERGING = tuple(k for k, v in CASES.items() if v[5] is not None)
NOT_CONVERGING = "c8_n1000"


def mixture_table(C, N, true_w, sep, seed):
    """(C, N) float32: log N(x_i; c * sep, 1) with x drawn from the mixture of weights ``true_w``."""
    rng = np.random.default_rng(seed)
    comp = rng.choice(C, size=N, p=np.asarray(true_w, dtype=np.float64) / np.sum(true_w))
    mu = np.arange(C, dtype=np.float64) * sep
    x = rng.normal(mu[comp], 1.0)
    ll = -0.5 * (x[None, :] - mu[:, None]) ** 2 - 0.5 * np.log(2.0 * np.pi)
    return np.ascontiguousarray(ll.astype(np.float32))


@functools.lru_cache(maxsize=None)
def table(name):
    """The case's table: computed once, shared by the tests, left unchanged (it is marked read-only)."""
    C, N, true_w, sep, seed, _ = CASES[name]
    ll = mixture_table(C, N, true_w, sep, seed)
    ll.setflags(write=False)
    return ll


@functools.lru_cache(maxsize=None)
def shape_table(C, n, seed=0):
    """A table of an arbitrary shape for the shape sweep: C components half a standard deviation apart, uneven true weights."""
    true_w = np.arange(C, 0, -1, dtype=np.float64)
    ll = mixture_table(C, n, true_w, 0.5 if C > 8 else 1.5, 100 + seed + 7 * C)
    ll.setflags(write=False)
    return ll


def uniform_rho(C):
    return np.ones(C, dtype=np.float32)
