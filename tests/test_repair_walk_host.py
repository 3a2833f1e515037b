"""Host checks of tests/repair_walk_cases.py, so that tests/test_hip_repair_walk.py cannot go quietly blind: whatever the rows per
work item of a bf16x6 variant are (64, 128 or 256), the row counts hold a repair launch of exactly 256 items, one of 257 and one of
at least 513; the marked rows fall into the items that matter; and every mark value keeps the float64 oracle finite and the
problem well-conditioned in float32, so that the bars of the GPU file are attainable on the marked rows."""
import numpy as np
import pytest

import repair_walk_cases as rw


def _launches(rpi):
    return {n: rw.n_items(n, rpi) for n in rw.ROW_COUNTS}


@pytest.mark.parametrize("rpi", rw.ROWS_PER_ITEM)
def test_row_counts_put_the_grid_cap_edge_wherever_it_can_lie(rpi):
    items = _launches(rpi)
    assert rw.GRID_CAP in items.values()                            # no walk: the last launch shape before the cap bites
    assert rw.GRID_CAP + 1 in items.values()                        # one workgroup runs two items
    assert any(v >= 2 * rw.GRID_CAP + 1 for v in items.values())    # some workgroup runs three
    assert any(n % rpi for n in rw.ROW_COUNTS if items[n] > rw.GRID_CAP)      # a ragged last item on a walking launch
    # the geometries with two row counts: n = 70001 walks whatever the form (32769 as well unless an item holds 256 rows)
    short = [rw.n_items(n, rpi) for n in rw.SHORT_COUNTS]
    assert max(short) > rw.GRID_CAP and (rpi == 256 or min(short) > rw.GRID_CAP)
    assert set(rw.SHORT_COUNTS) <= set(rw.ROW_COUNTS)


@pytest.mark.parametrize("n", rw.ROW_COUNTS)
@pytest.mark.parametrize("rpi", rw.ROWS_PER_ITEM)
def test_marked_rows_fall_into_the_items_that_matter(rpi, n):
    rows = rw.marked_rows(n)
    assert rows.size == np.unique(rows).size and rows.min() == 0 and rows.max() == n - 1
    assert np.array_equal(rows, rw.marked_rows(n))                  # seeded: the same rows in every process
    total = rw.n_items(n, rpi)
    pos = np.unique(rows // rpi)                                    # positions in the work list (one component, one batch)
    assert 0 in pos and total - 1 in pos
    if n % rpi:
        assert (n - 1) // rpi == total - 1                          # the ragged last item is the marked one
    # the kernel deals items over the XCDs before it maps them to positions: the same facts in the launch's own item numbers
    items = rw.items_of_rows(rows, n, rpi)
    assert rw.position_of_item(0, total) == 0 and 0 in items
    assert sorted(rw.position_of_item(i, total) for i in range(total)) == list(range(total))
    if total > rw.GRID_CAP:
        assert (pos >= rw.GRID_CAP).any()
        assert any(p + rw.GRID_CAP in pos for p in pos)             # two positions 256 apart
        assert (items >= rw.GRID_CAP).any()                         # a walked item with real work
        both = [i for i in items if i + rw.GRID_CAP in items]       # two items 256 apart: run by the same workgroup
        print(f"WALK rpi {rpi} n {n}: {total} items, {items.size} marked, {int((items >= rw.GRID_CAP).sum())} of them walked, "
              f"{len(both)} workgroups with two marked items")
        assert both, (rpi, n)
        for item in rw.WALKED_ITEMS:                                # workgroups 0 and 1: every item they walk holds a mark
            assert item >= total or item in items, (rpi, n, item)
    # a workgroup whose first item holds no mark but whose second does: the probe's `continue` in front of real work
    # (a 257-item launch walks one item, and that one follows the marked item 0)
    if total > rw.GRID_CAP + 1:
        assert any(i - rw.GRID_CAP not in items for i in items if i >= rw.GRID_CAP)


@pytest.mark.parametrize("n", rw.ROW_COUNTS)
def test_dense_rows_mark_every_item_of_every_form(n):
    rows = rw.dense_rows(n)
    assert rows[0] == 0 and rows[-1] == n - 1 and np.all(np.diff(rows) <= 61)
    for rpi in rw.ROWS_PER_ITEM:
        assert np.unique(rows // rpi).size == rw.n_items(n, rpi)


@pytest.mark.parametrize("C,S", [(3, 2), (3, 3)])
def test_group_launches_straddle_the_cap_too(C, S):
    """3.3: n C S = 16385 k (rounded up): for every rows-per-item value some group launch walks, and the marks of the last
    component's last batch lie in walked items."""
    ns = rw.group_rows_per_batch(C, S)
    assert all(16385 * k <= n * C * S < 16385 * k + C * S for n, k in zip(ns, (1, 2, 4, 8)))
    for rpi in rw.ROWS_PER_ITEM:
        totals = [rw.n_items(n, rpi, C, S) for n in ns]
        assert max(totals) > 2 * rw.GRID_CAP, (rpi, totals)
        assert sum(t > rw.GRID_CAP for t in totals) >= 2, (rpi, totals)




# ------------------------------------------------------------------ the mark values: finite, and a fair question to ask of float32
LL_BAR, Z_BAR = 1e-5, 2e-5       # the bars tests/test_hip_repair_walk.py holds the repaired rows to


def _rel(a, b):
    a, b = np.asarray(a, dtype=np.float64), np.asarray(b, dtype=np.float64)
    return float(np.max(np.abs(a - b) / np.maximum(np.abs(b), 1.0)))


def _fair(tag, spec, rows_in, inverse=False):
    """The float64 oracle is finite on these rows, and the reference's own float32 arithmetic (the oracle's torch backend) is within a
    third of every bar of it: the bars are attainable by a float32-faithful kernel on the rows the GPU tests send to the oracle."""
    from oracle import gbnf_oracle as oracle
    fn = oracle.component_inverse if inverse else oracle.component_forward
    z64, ld64 = fn(spec, rows_in, backend="numpy64")
    z32, ld32 = fn(spec, rows_in.copy(), backend="torch")
    assert np.isfinite(z64).all() and np.isfinite(ld64).all() and np.isfinite(z32).all() and np.isfinite(ld32).all(), tag
    figures = {"z": _rel(z32, z64) / Z_BAR, "ld": _rel(ld32, ld64) / LL_BAR}
    if not inverse:
        ll64 = oracle.component_log_prob(spec, rows_in, backend="numpy64")
        ll32 = oracle.component_log_prob(spec, rows_in.copy(), backend="torch")
        assert np.isfinite(ll64).all() and np.isfinite(ll32).all(), tag
        figures["ll"] = _rel(ll32, ll64) / LL_BAR
    print("FAIR", *tag, " ".join(f"{k} {v:.2f} of its bar" for k, v in figures.items()))
    assert max(figures.values()) <= 1.0 / 3.0, (tag, figures)


@pytest.mark.parametrize("gid", sorted(rw.GEOMETRIES))
def test_mark_values_are_finite_and_well_conditioned(gid):
    """Every (row count, pattern) of 3.1, on the rows the GPU test asks the oracle about; z -> x for the geometries of 3.6; the marks
    do leave the fp16 range and touch no other row."""
    g = rw.GEOMETRIES[gid]
    spec = rw.spec_of(gid)
    assert set(g["counts"]) <= set(rw.ROW_COUNTS)
    for n in g["counts"]:
        for pattern in rw.PATTERNS:
            x, rows, xm = rw.forward_inputs(gid, n, pattern)
            keep = np.ones(n, dtype=bool)
            keep[rows] = False
            assert np.array_equal(xm[keep], x[keep]) and float(np.abs(x).max()) < 100.0
            assert (np.abs(xm[rows]).max(axis=1) > 65504.0).all()
            sub = rw.oracle_rows(rows)
            assert sub.size <= rw.ORACLE_ROWS and sub[0] == rows[0] and sub[-1] == rows[-1]
            _fair((gid, n, pattern), spec, xm[sub])
        if gid in rw.INVERSE_GEOMETRIES and n in rw.SHORT_COUNTS:
            z, rows, zm = rw.inverse_inputs(gid, n)
            assert (np.abs(zm[rows]).max(axis=1) > 65504.0).all()
            _fair((gid, n, "inverse"), spec, zm[rw.oracle_rows(rows)], inverse=True)


@pytest.mark.parametrize("S", [2, 3])
@pytest.mark.parametrize("gid", ["G1", "G2"])
def test_group_inputs_are_finite_and_well_conditioned_for_every_component(gid, S):
    specs = rw.mixture_specs(gid)
    assert len(specs) == 3 and all(s["d"] == rw.spec_of(gid)["d"] and s["kind"] == rw.spec_of(gid)["kind"] for s in specs)
    for k in range(4):
        n, rows, plain, marked = rw.group_inputs(gid, S, k)
        assert len(rows) == len(plain) == len(marked) == S and all(x.shape == (n, specs[0]["d"]) for x in marked)
        assert len({r.tobytes() for r in rows}) == S                       # other marked rows in every batch
        assert np.array_equal(rows[-1], rw.dense_rows(n))
        for c, spec in enumerate(specs):
            for b in (0, S - 1):                                           # what the GPU test asks the oracle about
                _fair((gid, f"S{S}", n, f"c{c}", f"b{b}"), spec, marked[b][rw.oracle_rows(rows[b])[::3]])
