"""The case lists of tests/test_hip_repair_walk.py, importable without a GPU (tests/test_repair_walk_host.py checks them).

A repair launch (csrc/gbnf_flow_kernel_hx3.hip.h, hx3_launch_wv) has at most GRID_CAP workgroups; with more work items than that,
workgroup w walks the items w, w + GRID_CAP, w + 2 GRID_CAP, ...  An item holds 16 * ENT * WAVES rows with ENT in {1, 2} and WAVES in
{4, 8}, fixed per bf16x6 variant at compile time and not visible through the ABI: the lists below assume neither, they put the
GRID_CAP-item edge wherever it can lie (ROWS_PER_ITEM).
"""
import numpy as np

GRID_CAP = 256                        # `if (p.repair && grid > 256) grid = 256`
ROWS_PER_ITEM = (64, 128, 256)        # 16 * ENT * WAVES

# for each rows-per-item value: a launch of exactly 256 items (no walk), one of 257 (one workgroup runs two) and one of >= 513
# (some workgroup runs three); 70001 and 140003: ragged last items for every form
ROW_COUNTS = (16384, 16385, 32768, 32769, 65536, 65537, 70001, 140003)
SHORT_COUNTS = (32769, 70001)
FORCE_NT = (1, 2)
MARK_SEED = 5150


def n_items(n, rows_per_item, n_comp=1, n_batches=1):
    return -(-n // rows_per_item) * n_comp * n_batches


def position_of_item(item, total):
    """The kernel's XCD-aware deal (flow_kernel_hx3, `item -> (comp, batch, grp)`): items go round-robin over the 8 XCDs, each XCD
    owns a contiguous run of the work list.  -> the position in the component-major work list that work item `item` evaluates."""
    xcd, j = item & 7, item >> 3
    base, rem = total >> 3, total & 7
    return xcd * base + min(xcd, rem) + j


def items_of_rows(rows, n, rows_per_item):
    """The work items (one component, one batch) that own `rows`: sorted item indices as the launch numbers them."""
    total = n_items(n, rows_per_item)
    item_at = np.empty(total, dtype=np.int64)
    for item in range(total):
        item_at[position_of_item(item, total)] = item
    return np.unique(item_at[np.asarray(rows, dtype=np.int64) // rows_per_item])


WALKED_ITEMS = (1, GRID_CAP, GRID_CAP + 1, 2 * GRID_CAP, 2 * GRID_CAP + 1)


def marked_rows(n, seed=MARK_SEED):
    """Rows 0 and n - 1, both sides of every place an item edge can lie around the 1st, 255th .. 257th and 512th item of every form,
    and 24 seeded random rows; clipped to [0, n), sorted, unique.

    Those rows are positions in the work list, and the kernel deals its items over the XCDs before it maps them to positions: item 256
    of a 257-item launch evaluates position 32, which none of the rows above touches.  So for every form that walks at this n the first
    row of the positions that items 1, 256, 257, 512 and 513 evaluate is marked as well: workgroups 0 and 1 then evaluate every item
    they walk, one behind the other (item 0 evaluates position 0, which holds row 0)."""
    rows = {0, n - 1}
    for r in ROWS_PER_ITEM:
        for k in (1, 255, 256, 257, 512):
            rows.update((r * k - 1, r * k))
        total = n_items(n, r)
        if total > GRID_CAP:
            rows.update(r * position_of_item(item, total) for item in WALKED_ITEMS if item < total)
    rows.update(int(v) for v in np.random.RandomState(seed + n % 9973).randint(0, n, size=24))
    return np.array(sorted(v for v in rows if 0 <= v < n), dtype=np.int64)


def dense_rows(n):
    """Every 61st row and the last one: every item of every form holds a mark (the last item of n = 256 k + 1 is row n - 1 alone), so
    every workgroup evaluates every item it walks."""
    return np.unique(np.append(np.arange(0, n, 61, dtype=np.int64), n - 1))


PATTERNS = {"marked": marked_rows, "dense": dense_rows}


# ------------------------------------------------------------------ geometries: the smallest that reach a structurally different kernel
def _g1():
    from gbnf_amd import synth
    return synth.synth_glow_spec(6, 30, 3, seed=1)                       # the geometry the existing repair tests use


def _g2():
    from gbnf_amd import synth
    return synth.synth_realnvp_spec(21, 105, 3, batch_norm=True, flip_init=1, seed=7102)       # two nets per step


def _g3():
    from gbnf_amd import synth
    return synth.synth_glow_spec(43, 215, 2, seed=7103)                  # 14 hidden tiles, the heaviest stages


def _g4():
    from gbnf_amd import synth
    return synth.synth_glow_spec(43, 64, 3, depth=2, seed=7104)          # the register-chained depth variants


def _g5():
    from gbnf_amd import synth                                           # one block, the residual variants
    # (trained_like: the last layer of a trained net is small; with nn.Linear's init a ReLU ResidualNet's log-scale grows with its
    #  input and exp(s) of any row beyond the fp16 range overflows float32 and float64 alike.  Seed: see GEOMETRIES.)
    return synth.synth_realnvp_spec(21, 64, 2, depth=1, coupling_network="residual", seed=7108, trained_like=True)


def _g6():
    from gbnf_amd import synth
    return synth.synth_glow_spec(43, 430, 2, seed=7106)                  # 28 tiles, one wave per SIMD


def _g7():
    from gbnf_amd import synth
    return synth.synth_glow_spec(8, 40, 26, seed=7107)                   # per-step tables read from the blob, not LDS


# A marked row must leave the fp16 range in some operand of the f16x3 kernel, keep the float64 oracle (and the float32 kernels) finite,
# and stay a well-conditioned problem in float32: beyond 65504 a float32 sum w x carries an absolute error of 1e-3 .. 1e-1, which a
# tanh unit whose pre-activation happens to cancel to O(1) hands on in full -- the reference's own float32 arithmetic then misses the
# 1e-5 bar against float64, and so would any float32 kernel (tests/test_repair_walk_host.py measures it on every case).
#   "row"       the whole row x 1e6, what test_out_of_range_samples_are_repaired does on this very geometry (d = 6, h = 30: few units).
#               Which units cancel is drawn anew with every row: at d = 43, h >= 215 or K = 26 a handful of rows in a thousand miss the
#               bar in float32 itself (measured: the float32 oracle against float64, ll 9e-5, z 3e-4 of its scale).
#   "features"  two features set to +3.0e5 / -8.0e4, the rest of the row as drawn (what
#               test_rows_beyond_the_fp16_range_are_marked_and_repaired_in_the_same_call does at d = 43, h = 215).  Whether a unit cancels is
#               then a property of the weights, the same for every marked row; the seeds below are such that none does (G5: the first of
#               7105 .. 7108 with the float32 oracle inside a third of every bar).
GEOMETRIES = {
    "G1": dict(make=_g1, counts=ROW_COUNTS, mark="row"),
    "G2": dict(make=_g2, counts=SHORT_COUNTS, mark="features"),
    "G3": dict(make=_g3, counts=SHORT_COUNTS, mark="features"),
    "G4": dict(make=_g4, counts=SHORT_COUNTS, mark="features"),
    "G5": dict(make=_g5, counts=SHORT_COUNTS, mark="features"),
    "G6": dict(make=_g6, counts=SHORT_COUNTS, mark="features"),
    "G7": dict(make=_g7, counts=SHORT_COUNTS, mark="features"),
}
INVERSE_GEOMETRIES = ("G1", "G2")            # 3.6: the marks go into z
ORACLE_ROWS = 60                             # the float64 oracle is asked for at most this many rows per call

_SPECS, _BATCHES = {}, {}


def spec_of(gid):
    if gid not in _SPECS:
        _SPECS[gid] = GEOMETRIES[gid]["make"]()
    return _SPECS[gid]


def mixture_specs(gid, C=3):
    """C components of the geometry's architecture (3.3, 3.5), seeds of their own (RealNVP: component c starts flipped c times)."""
    from gbnf_amd import synth
    if gid == "G1":
        return synth.synth_boosted_specs("glow", C, 6, 30, 3, seed=71)
    if gid == "G2":
        return synth.synth_boosted_specs("realnvp", C, 21, 105, 3, seed=72, batch_norm=True)
    raise KeyError(gid)


def apply_marks(x, rows, mark):
    """A copy of the float32 batch `x` with `rows` pushed out of the fp16 range; every other row keeps its bits."""
    out = np.array(x, dtype=np.float32, copy=True)
    rows = np.asarray(rows, dtype=np.int64)
    if mark == "row":
        out[rows] *= np.float32(1e6)
    elif mark == "features":
        d = out.shape[1]
        out[rows, 3 % d] = np.float32(3.0e5)
        out[rows, (d - 3) % d] = np.float32(-8.0e4)
    else:
        raise ValueError(mark)
    return out


def batch(d, n, seed):
    """A float32 N(0, 1) batch: made once per process, shared, never written to."""
    if (d, n, seed) not in _BATCHES:
        from gbnf_amd import synth
        x = synth.synth_batch(n, d, seed=seed)
        x.setflags(write=False)
        _BATCHES[d, n, seed] = x
    return _BATCHES[d, n, seed]


def oracle_rows(rows):
    """At most ORACLE_ROWS of `rows`, evenly spread, the first and the last included: what the oracle is asked for."""
    if rows.size <= ORACLE_ROWS:
        return rows
    return rows[np.unique(np.linspace(0, rows.size - 1, ORACLE_ROWS).astype(np.int64))]


def forward_inputs(gid, n, pattern):
    """3.1 / 3.2 / 3.4: (the plain batch, the marked rows, the batch with the marks applied)."""
    x = batch(spec_of(gid)["d"], n, seed=n)
    rows = PATTERNS[pattern](n)
    return x, rows, apply_marks(x, rows, GEOMETRIES[gid]["mark"])


def inverse_inputs(gid, n):
    """3.6: the same for z."""
    z = batch(spec_of(gid)["d"], n, seed=n + 1)
    rows = marked_rows(n)
    return z, rows, apply_marks(z, rows, GEOMETRIES[gid]["mark"])


def group_rows_per_batch(C, S):
    """3.3: per-batch row counts n such that n * C * S is 16385 k for k in (1, 2, 4, 8), rounded up to what divides."""
    return [-(-16385 * k // (C * S)) for k in (1, 2, 4, 8)]


def group_inputs(gid, S, k, C=3):
    """3.3: (n, marked rows per batch, plain batches, marked batches): other marked rows in every batch, the last batch -- and with it
    the end of every component's run of work items -- marked densely."""
    n = group_rows_per_batch(C, S)[k]
    d = spec_of(gid)["d"]
    rows = [marked_rows(n, seed=MARK_SEED + 1 + b) for b in range(S - 1)] + [dense_rows(n)]
    plain = [batch(d, n, seed=100 + b) for b in range(S)]
    return n, rows, plain, [apply_marks(x, r, GEOMETRIES[gid]["mark"]) for x, r in zip(plain, rows)]
