"""CPU: fitting all mixture weights by EM (gbnf_weights_em / gbnf_weights_to_rho) as far as it goes without a device -- header and
binding, the workspace size, every refusal that returns before a launch -- and the float64 yardstick of the GPU tests
(tests/weights_oracle.py) checked on its own: L_t never decreases, a converged case satisfies the fixed-point condition, the weights
written back as rho reproduce the yardstick's G_i through the oracle's own recursion (the recursion IS the flat mixture), the row
exclusion, and how far the final weights move when the sums are taken in another order or in a wider format."""
import ctypes as C
import os
import re

import numpy as np
import pytest

import weights_cases as wc
import weights_oracle as wo
from conftest import REPO

WEIGHTS_SYMBOLS = ("gbnf_weights_em_workspace_bytes", "gbnf_weights_em", "gbnf_weights_to_rho")


def _lib():
    from gbnf_amd import native
    return native.lib()


def test_symbols_are_declared_bound_and_exported():
    from gbnf_amd import native
    text = open(os.path.join(REPO, "include", "gbnf.h")).read()
    code = re.sub(r"/\*.*?\*/", "", text, flags=re.S)
    L = _lib()
    assert native.WEIGHTS_SYMBOLS == WEIGHTS_SYMBOLS
    for name in WEIGHTS_SYMBOLS:
        assert re.search(r"\b%s\s*\(" % name, code), f"{name} is not declared in include/gbnf.h"
        assert name in native.ABI_SYMBOLS
        fn = getattr(L, name)
        assert fn.argtypes is not None and fn.restype is C.c_int, name
        decl = re.search(r"\b%s\s*\(([^;]*)\);" % name, code).group(1)
        assert len(fn.argtypes) == decl.count(",") + 1, f"{name}: {len(fn.argtypes)} argtypes for `{decl}`"
    assert int(re.search(r"#define\s+GBNF_WEIGHTS_MAX_COMPONENTS\s+(\d+)", text).group(1)) == native.WEIGHTS_MAX_COMPONENTS == wo.MAX_COMPONENTS
    assert re.search(r"#define\s+GBNF_WEIGHTS_STATE_DOUBLES\s+\(8 \+ GBNF_WEIGHTS_MAX_COMPONENTS\)", text)
    assert native.WEIGHTS_STATE_DOUBLES == wo.STATE_DOUBLES == 72
    assert sorted(native.WEIGHTS_STATE.values()) == list(range(9))
    for name in ("weights_em", "weights_to_rho"):
        assert callable(getattr(native, name))
    from gbnf_amd import BoostedFlow, image_glow
    assert callable(BoostedFlow.fit_weights) and callable(image_glow.BoostedImageFlow.fit_weights)


def test_workspace_bytes():
    L = _lib()
    nb = C.c_int64(-1)
    for C_ in (1, 8, 64):
        sizes = []
        for n in (0, 1, 1024, 1 << 20, 1 << 33):
            assert L.gbnf_weights_em_workspace_bytes(C_, n, C.byref(nb)) == 0
            sizes.append(nb.value)
            # two buffers of (C + 2) sums per workgroup of the largest grid, in 256-byte steps
            assert nb.value >= 2 * (C_ + 2) * 8 * 256 and nb.value % 256 == 0 and nb.value <= 1 << 20
        assert sizes == sorted(sizes)
    for C_, n, out in ((0, 4, nb), (65, 4, nb), (3, -1, nb)):
        assert L.gbnf_weights_em_workspace_bytes(C_, n, C.byref(out)) == -1 and L.gbnf_last_error()
    assert L.gbnf_weights_em_workspace_bytes(3, 4, None) == -1


def test_refusals_before_any_device_call():
    """Every argument check returns before the device is touched: host addresses stand in for device buffers."""
    L = _lib()
    n = 8
    ll = np.zeros((3, n), dtype=np.float32)
    rho = np.ones(3, dtype=np.float32)
    state = np.full(wo.STATE_DOUBLES, 7.0)
    nb = C.c_int64()
    assert L.gbnf_weights_em_workspace_bytes(3, n, C.byref(nb)) == 0
    ws = np.zeros(nb.value // 8, dtype=np.float64)
    p = lambda a: None if a is None else C.c_void_p(a.ctypes.data)

    def em(ll_=ll, stride=n, C_=3, n_=n, rho_=rho, max_iters=5, tol=1e-9, state_=state, ws_=ws, nbytes=nb.value):
        return L.gbnf_weights_em(p(ll_), stride, C_, n_, p(rho_), max_iters, tol, p(state_), p(ws_), nbytes, None)

    bad = {"null ll": dict(ll_=None), "null rho": dict(rho_=None), "null state": dict(state_=None), "null workspace": dict(ws_=None),
           "n < 0": dict(n_=-1), "C = 0": dict(C_=0), "C = 65": dict(C_=65), "stride < n": dict(stride=n - 1),
           "max_iters < 0": dict(max_iters=-1), "short workspace": dict(nbytes=nb.value - 8), "NaN tol": dict(tol=float("nan"))}
    for what, kw in bad.items():
        assert em(**kw) == -1, f"weights_em, {what}: accepted"
        assert L.gbnf_last_error(), what

    def to_rho(state_=state, C_=3, lo=0.01, hi=100.0, rho_=rho):
        return L.gbnf_weights_to_rho(p(state_), C_, lo, hi, p(rho_), None)

    bad = {"null state": dict(state_=None), "null rho": dict(rho_=None), "C = 0": dict(C_=0), "C = 65": dict(C_=65),
           "rho_min > rho_max": dict(lo=2.0, hi=1.0), "NaN bound": dict(lo=float("nan"))}
    for what, kw in bad.items():
        assert to_rho(**kw) == -1, f"weights_to_rho, {what}: accepted"
        assert L.gbnf_last_error(), what
    assert (state == 7.0).all() and (rho == 1.0).all()


@pytest.mark.parametrize("name", list(wc.CASES))
def test_yardstick_never_decreases_and_stops_where_pinned(name):
    C_, N, _, _, _, evaluations = wc.CASES[name]
    L = []
    s = wo.em(wc.table(name), wc.uniform_rho(C_), wc.MAX_ITERS, wc.TOL, history=L)
    print(f"{name}: {len(L)} evaluations, L_0 {L[0]!r} -> L {L[-1]!r}, last step {s[6]:.3e}")
    # EM never decreases L; rounding may: a decrease is bounded by the sum's own error, N 2^-52 max|G| / N per evaluation
    slack = 2.0 ** -52 * N * max(abs(L[0]), abs(L[-1]))
    assert all(b >= a - slack for a, b in zip(L, L[1:]))
    assert s[2] == N and s[3] == 0 and s[7] == 0 and s[4] == L[0] and s[5] == L[-1]
    assert abs(s[8:8 + C_].sum() - 1.0) <= 1e-12
    if evaluations is None:
        assert len(L) == wc.MAX_ITERS + 1 and s[0] == wc.MAX_ITERS and s[1] == 0 and s[6] > wc.TOL
    else:
        assert len(L) == evaluations and s[0] == evaluations - 1 and s[1] == 1 and s[6] <= wc.TOL


@pytest.mark.parametrize("name", wc.CONVERGING)
def test_fixed_point_condition_at_convergence(name):
    """At a maximum q_c = S_c / (N w_c) is 1 for every w_c > 0.  What the stopping tolerance says about it: an EM update w -> w' = q w
    raises L by at least KL(w' || w) = sum_c w_c q_c log q_c, which is sum_c w_c (q_c - 1)^2 / 2 to leading order (sum_c w_c q_c = 1),
    and the stopping rule saw a rise of at most TOL; so |q_c - 1| <= sqrt(2 TOL / w_c) for the update that stopped, and for the final
    weights too as long as the residual does not grow from one update to the next (EM converges monotonically here).  L is second
    order in the weights: the first-order quantity is tied to the square root of the tolerance, not to the tolerance."""
    C_, N = wc.CASES[name][:2]
    s = wo.em(wc.table(name), wc.uniform_rho(C_), wc.MAX_ITERS, wc.TOL)
    w = s[8:8 + C_]
    _, _, S = wo.evaluate(wc.table(name).astype(np.float64), w)
    q = S / (N * w)
    print(f"{name}: S_c / (N w_c) - 1 = {q - 1.0}, bound {np.sqrt(2.0 * wc.TOL / w)}")
    assert (w > 0).all() and (np.abs(q - 1.0) <= np.sqrt(2.0 * wc.TOL / w)).all()


@pytest.mark.parametrize("name", list(wc.CASES))
def test_rho_written_back_gives_the_flat_mixture_through_the_recursion(name):
    """rho = w * S fed to the oracle's own recursion (density_experiment.py:561-573) gives the yardstick's G_i."""
    from oracle import gbnf_oracle as oracle
    C_ = wc.CASES[name][0]
    ll = wc.table(name)[:, :1000]
    s = wo.em(ll, wc.uniform_rho(C_), 20, 0.0)
    w = s[8:8 + C_]
    for total in (1.0, 3.75):
        G = oracle.mixture_recursion(ll.astype(np.float64), w * total, backend="numpy64")
        want = wo.mixture_G(ll, w)
        assert np.abs(G - want).max() <= 1e-12 * np.abs(want).max()


def test_exclusion_rule():
    ll = np.array(wc.table("c3_n4096")[:, :64])
    ll[1, 3] = -np.inf                       # a single -inf entry: legal
    ll[:, 5] = -np.inf                       # -inf under every component
    ll[0, 7] = np.nan
    ll[2, 9] = np.inf
    keep = wo.used_rows(ll)
    assert keep.sum() == 61 and not keep[[5, 7, 9]].any() and keep[3]
    s = wo.em(ll, wc.uniform_rho(3), 10, 0.0)
    clean = wo.em(np.delete(ll, [5, 7, 9], axis=1), wc.uniform_rho(3), 10, 0.0)
    assert s[2] == 61 and s[3] == 3 and np.isfinite(s).all()
    assert (s[8:11] == clean[8:11]).all() and s[5] == clean[5]
    # no usable row, and a rho that cannot start: a bad start, no update
    for table, rho in ((ll[:, [5, 7, 9]], wc.uniform_rho(3)), (ll[:, :0], wc.uniform_rho(3)), (ll, np.zeros(3, np.float32)),
                       (ll, np.array([1.0, -1.0, 1.0], np.float32)), (ll, np.array([1.0, np.inf, 1.0], np.float32))):
        b = wo.em(table, rho, 10, 1e-9)
        assert b[7] == 1 and b[0] == 0 and b[1] == 0
        new_rho, flags = wo.to_rho(b, np.array([3.0, 2.0, 1.0], np.float32), 3)
        assert (new_rho == [3.0, 2.0, 1.0]).all() and flags == 1


def test_to_rho_of_the_yardstick():
    s = wo.em(wc.table("c3_n4096"), wc.uniform_rho(3), 20, 0.0)
    rho = np.array([1.0, 0.5, 0.25, 0.125], dtype=np.float32)
    new_rho, flags = wo.to_rho(s, rho, 3)
    assert flags == 0 and new_rho[3] == rho[3]
    assert abs(float(new_rho[:3].astype(np.float64).sum()) - 1.75) <= 3 * 2.0 ** -24 * 1.75
    assert np.abs(new_rho[:3] / new_rho[:3].sum() - s[8:11]).max() <= 4 * 2.0 ** -24
    s[8:11] = [0.999, 0.0008, 0.0002]
    new_rho, flags = wo.to_rho(s, np.ones(3, np.float32), 3)
    assert flags == 4 and (new_rho[1:] == np.float32(0.01)).all()


def test_sensitivity_of_the_final_weights():
    """The same 100 updates with the rows in reverse order and with np.longdouble sums: the largest relative difference in the final
    weights over all cases stays below 1e-11.  The GPU tests' bar of 1e-9 is a hundred times that."""
    worst = 0.0
    for name, (C_, *_rest) in wc.CASES.items():
        ll, rho = wc.table(name), wc.uniform_rho(C_)
        w = wo.em(ll, rho, wc.FIXED_UPDATES, 0.0)[8:8 + C_]
        for kw in (dict(reverse=True), dict(dtype=np.longdouble)):
            other = wo.em(ll, rho, wc.FIXED_UPDATES, 0.0, **kw)[8:8 + C_]
            rel = float((np.abs(other - w) / w).max())
            print(f"{name} {kw}: {rel:.3e}")
            worst = max(worst, rel)
    assert worst < 1e-11
