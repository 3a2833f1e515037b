"""Host (no GPU): what tests/test_hip_train_large_batch.py asks of the device is reachable in float32, and which weight-gradient block
shapes a trainer can be cut into.

1. The gradient bars.  The forward of every case of tests/train_large_batch_cases.py restated in torch float32 (the oracle's own
   restatement on float32 leaves) and differentiated by autograd: its parameter gradients and g_x must stay within a THIRD of the
   device test's bars (G_RTOL of each tensor's largest entry; with batch statistics the 0.05 x max floor) against the float64
   oracle.  A device result outside the bar is then a kernel finding, not float32 arithmetic.
2. The statistics bars.  The summation orders of bn_stats_kernel (256 strided per-thread sums, the xor tree of a wave, the four
   wave sums) and of the three-launch form from 16384 rows on (64 row chunks of ceil(n / 64) rows, each summed like a block; the 64
   chunk sums added in index order) restated in numpy float32 on the inputs of every BatchNorm step of the table's batch-statistics
   cases: mean and variance must stay within HALF of the device test's tolerances (mean atol 2e-6; variance rtol 1e-5 + atol 1e-6).
   (The device may contract c * c + b into one fma; the restatement rounds the square first.  Either is one rounding per term.)
3. The block shapes.  wg_shape (csrc/gbnf_train.hip, through gbnf_debug_wg_shape: host code, no device) over the Linear layers of
   every geometry gbnf_trainer_create accepts: 256 x 128 and 128 x 256 blocks are never cut, so wg_shape's table and
   gbnf_wgrad_kernel.inc carry no row / no wgrad_block instantiation for them; every shape that IS cut has both, and they agree."""
import ctypes as C
import os
import re

import numpy as np
import pytest

import train_large_batch_cases as T
from conftest import REPO

G_RTOL = 2e-4          # tests/test_hip_train.py (not imported: that module is a GPU module)

_KEYS = {}
for _c in T.CASES:
    _KEYS.setdefault(T.oracle_key(_c), _c)
_BS_KEYS = {k: c for k, c in _KEYS.items() if c[8]}


def _key_id(case):
    kind, d, h, K, n, kw, _, _, bs, _ = case
    return f"{kind}_d{d}_h{h}_K{K}" + "".join(f"_{k}{v}" for k, v in sorted(kw.items())) + f"_n{n}" + ("_bstats" if bs else "")


def _f32_grads(spec, x, g_z, g_l, train):
    """oracle.component_grads with every leaf, the input and the upstream gradients in float32."""
    import torch
    from oracle import gbnf_oracle as oracle

    class F32GradOps(oracle._TorchGradOps):
        def arr(self, a):
            if torch.is_tensor(a):
                return a
            if id(a) not in self.leaves:
                self.leaves[id(a)] = (a, torch.tensor(np.asarray(a, dtype=np.float32), dtype=torch.float32, requires_grad=True))
            return self.leaves[id(a)][1]

        def zeros(self, n):
            return torch.zeros(n, dtype=torch.float32)

    ops = F32GradOps()
    xt = torch.tensor(np.asarray(x, dtype=np.float32), dtype=torch.float32, requires_grad=True)
    z, ld = xt, ops.zeros(xt.shape[0])
    for step in spec["steps"]:
        if spec["kind"] == "glow":
            z, ld = oracle.glow_step(ops, spec, step, z, ld)
        else:
            z, step_ld = oracle.realnvp_step(ops, spec, step, z, train=train)
            ld = ld + step_ld
    assert z.dtype == torch.float32 and ld.dtype == torch.float32
    loss = (z * torch.from_numpy(g_z)).sum() + (ld * torch.from_numpy(g_l)).sum()
    loss.backward()
    return xt.grad.numpy().copy(), [None if a is None else ops.grad_of(a) for a in oracle.param_arrays(spec)]


@pytest.mark.parametrize("case", list(_KEYS.values()), ids=[_key_id(c) for c in _KEYS.values()])
def test_float32_autograd_meets_a_third_of_the_gradient_bars(case):
    from oracle import gbnf_oracle as oracle
    spec, x, g_z, g_l = T.make_inputs(case)
    bs = case[8]
    gx64, grads64 = oracle.component_grads(spec, x, g_z, g_l, train=bs)
    gx32, grads32 = _f32_grads(spec, x, g_z, g_l, bs)
    floor = 0.05 * max(float(np.abs(g).max()) for g in grads64 if g is not None) if bs else 1e-3
    worst = 0.0
    for a, b in zip(grads32, grads64):
        if b is not None:
            worst = max(worst, float(np.abs(a - b).max()) / max(float(np.abs(b).max()), floor))
    e_x = float(np.abs(gx32 - gx64).max()) / float(np.abs(gx64).max())
    print(f"[large batch host] {_key_id(case)}: float32 autograd vs float64: parameters {worst:.2e}, g_x {e_x:.2e} (a third of the bar: {G_RTOL / 3:.2e})")
    assert worst <= G_RTOL / 3 and e_x <= G_RTOL / 3


def _block_sum(v):
    """The sum over axis 0 of v (m, d) float32 in the order of a 256-thread block: thread t adds rows t, t + 256, .. in turn
    (tr_block_sum's caller), the xor tree of each 64-lane wave, then red[0] + red[1] + red[2] + red[3]."""
    m, d = v.shape
    rows = -(-m // 256)
    pad = np.zeros((rows * 256, d), dtype=np.float32)
    pad[:m] = v
    acc = np.zeros((256, d), dtype=np.float32)
    for r in range(rows):
        acc = acc + pad[256 * r:256 * (r + 1)]          # (a thread past the end adds nothing: + 0.0f)
    w = acc.reshape(4, 64, d)
    lane = np.arange(64)
    for mask in (1, 2, 4, 8, 16, 32):
        w = w + w[:, lane ^ mask]
    red = w[:, 0]
    assert red.dtype == np.float32
    return ((red[0] + red[1]) + red[2]) + red[3]


def _stats_single(col):
    """bn_stats_kernel: one block per slot, two passes."""
    n = np.float32(col.shape[0])
    mean = _block_sum(col) / n
    c = col - mean
    return mean, _block_sum(c * c) / np.float32(col.shape[0] - 1)


def _stats_three_launch(col, nb=64):
    """bn_stats_part_kernel pass 1 / pass 2 and bn_stats_final_kernel: nb row chunks of ceil(n / nb) rows, sums in index order."""
    n = col.shape[0]
    per = -(-n // nb)

    def parts(v):
        out = []
        for b in range(nb):
            s0, s1 = b * per, min(b * per + per, n)
            out.append(_block_sum(v[s0:s1]) if s1 > s0 else np.zeros(v.shape[1], dtype=np.float32))
        return out

    def in_order(ps):
        tot = np.zeros_like(ps[0])
        for p in ps:
            tot = tot + p
        return tot

    ps = parts(col)
    mean = in_order(ps) / np.float32(n)           # (pass 2 and the final kernel add the same sums in the same order)
    c = col - mean
    pq = parts(c * c)
    return mean, in_order(pq) / np.float32(n - 1)


def _bn_inputs(spec, x):
    """The float64 input of every BatchNorm step of a RealNVP in train() mode, and the oracle's statistics of it."""
    from oracle import gbnf_oracle as oracle
    ops = oracle._ops("numpy64")
    z = ops.arr(x)
    inputs, stats = [], []
    for step in spec["steps"]:
        if step["bn"] is not None:
            inputs.append(z)
        z, _ = oracle.realnvp_step(ops, spec, step, z, train=True, stats_out=stats)
    assert len(inputs) == len(stats)
    return inputs, stats


@pytest.mark.parametrize("case", list(_BS_KEYS.values()), ids=[_key_id(c) for c in _BS_KEYS.values()])
def test_float32_summation_orders_meet_half_of_the_statistics_bars(case):
    spec, x, _, _ = T.make_inputs(case)
    n = case[4]
    inputs, stats = _bn_inputs(spec, x)
    form = _stats_single if n < 16384 else _stats_three_launch          # launch_bn_stats
    e_m = e_v = 0.0
    for z64, (mean64, var64) in zip(inputs, stats):
        mean, var = form(z64.astype(np.float32))
        assert mean.dtype == np.float32 and var.dtype == np.float32
        e_m = max(e_m, float(np.abs(mean - mean64).max()))
        e_v = max(e_v, float((np.abs(var - var64) / (1e-6 + 1e-5 * np.abs(var64))).max()))
    print(f"[large batch host] {_key_id(case)} ({form.__name__}): mean abs err {e_m:.2e} (half the bar: 1e-6), "
          f"variance err / (1e-6 + 1e-5 |var|) {e_v:.2e} (half the bar: 0.5)")
    assert e_m <= 0.5 * 2e-6
    assert e_v <= 0.5


# ---- 3. the block shapes --------------------------------------------------------------------------------------------------------
def _wg_shape(L, M, N, cap):
    out = (C.c_int32 * 4)()
    assert L.gbnf_debug_wg_shape(M, N, cap, out) == 0
    return tuple(int(v) for v in out)


def _layer_shapes():
    """(rows, cols) of every Linear of every coupling net gbnf_trainer_create accepts: coupled halves of at most 32 features
    (TR_MAX_IN), h <= 512 (TR_MAX_HIDDEN), all hidden layers h x h (check_net) whatever the depth or the ResidualNet form; the
    last layer has d2, d1 or (Glow, affine) 2 d2 rows."""
    shapes = set()
    for h in range(1, 513):
        shapes.add((h, h))
        for half in range(1, 33):
            shapes.add((h, half))
            shapes.add((half, h))
            shapes.add((2 * half, h))
    return shapes


def test_reachable_weight_gradient_block_shapes():
    """Done: the two table rows {256,128} and {128,256} and their wgrad_block instantiations are DELETED (not reachable)."""
    from gbnf_amd import native
    L = native.lib()
    L.gbnf_debug_wg_shape.argtypes = [C.c_int32, C.c_int32, C.c_int32, C.POINTER(C.c_int32)]
    L.gbnf_debug_wg_shape.restype = C.c_int
    reach = {256: {}, 128: {}}
    for cap in reach:
        for M, N in _layer_shapes():
            bm, bn, wm, wn = _wg_shape(L, M, N, cap)
            reach[cap].setdefault((bm, bn), (wm, wn))
            assert reach[cap][(bm, bn)] == (wm, wn)
    print(f"[large batch host] blocks at cap 256: {sorted(reach[256])}; at cap 128: {sorted(reach[128])}")
    assert set(reach[256]) == {(64, 64), (128, 64), (256, 64), (64, 128), (128, 128), (64, 256), (256, 256)}
    assert set(reach[128]) == {(64, 64), (128, 64), (64, 128), (128, 128)}
    # every block that is cut has a table row: 8 waves as wm x wn, whole 16 x 16 tiles per wave
    for cap in reach:
        for (bm, bn), (wm, wn) in reach[cap].items():
            assert wm * wn == 8 and bm % (16 * wm) == 0 and bn % (16 * wn) == 0, (bm, bn, wm, wn)
    # ... and the rows that are never cut are gone (a 200 x 100 problem belongs to no trainer)
    assert _wg_shape(L, 200, 100, 256) == (256, 128, 0, 0)
    assert _wg_shape(L, 100, 200, 256) == (128, 256, 0, 0)
    # the kernel's instantiations are exactly the blocks that are cut, with the tiles per wave the table implies
    inc = os.path.join(REPO, "gradient-boosted-normalizing-flows_amd", "csrc", "gbnf_wgrad_kernel.inc")
    with open(inc) as f:
        cases = re.findall(r"^\s*WG_CASE\((\d+), (\d+), (\d+), (\d+), (\d+), (\d+)\);", f.read(), flags=re.M)
    cases = {(int(bm), int(bn)): (int(nd), int(na), int(tm), int(tn)) for bm, bn, nd, na, tm, tn in cases}
    assert set(cases) == set(reach[256])
    for (bm, bn), (nd, na, tm, tn) in cases.items():
        wm, wn = reach[256][(bm, bn)]
        assert (tm, tn) == (bm // (16 * wm), bn // (16 * wn)), (bm, bn)
        assert (nd, na) == (max(bm // 128, 1), max(bn // 128, 1)), (bm, bn)        # 128-row pieces per thread of each operand
