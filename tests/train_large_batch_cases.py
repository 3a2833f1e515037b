"""The case table of the large-batch training tests (tests/test_hip_train_large_batch.py on the device, tests/test_train_large_batch_host.py
on the host): the batch sizes at which the trainer changes how it launches, on the geometries the bench lines are measured on.

Every case is ``(kind, d, h, K, n, kw, math, deterministic, batch_stats, expected_plan)``; ``expected_plan`` is the literal
``(list, chunk, Y)`` that ``wgrad_plan`` (csrc/gbnf_train.hip) must give for it -- list 0 = probs_dev (block edges up to 256), 1 =
probs_small_dev (up to 128), 2 = probs_safe_dev (64 x 64, the bf16x6 trainer) -- which the device test asserts through
gbnf_debug_trainer_wgrad_plan: a retuning of the plan that silently leaves a regime fails there instead of losing the coverage.

How the literals were worked out (np = n rounded up to 32 rows; dW blocks per step of one net):
  MINIBOONE Glow d = 43, h = 215: Linear layers 215 x 21, 215 x 215 (``depth`` of them), 44 x 215
      probs_dev        256 x 64, 256 x 256, 64 x 256      -> 2 / 3 / 4 blocks per step at depth 0 / 1 / 2
      probs_small_dev  2 of 128 x 64, 4 of 128 x 128, 2 of 64 x 128 -> 4 / 8 / 12
      probs_safe_dev   4, 16, 4 of 64 x 64                -> 8 / 24 / 40
  HEPMASS RealNVP d = 21, h = 105, two nets per step: 105 x 10|11, 105 x 105, 11|10 x 105
      both f16x3 lists 128 x 64, 128 x 128, 64 x 128      -> 4 / 6 / 8 blocks per step;   probs_safe_dev 2, 4, 2 -> 8 / 16 / 24
  narrow Glow d = 8, h = 64: 64 x 4, 64 x 64, 8 x 64: one 64 x 64 block each -> 3 per step on every list
  chunk = the largest power of two in [128, 2048] reached by doubling while blocks x (np // (2 chunk)) >= 240 (bf16x6: 1024);
  Y = ceil(np / chunk); probs_small_dev while np <= 16384.
With K >= 2 none of these geometries gives probs_dev at chunk 128 (it needs blocks x 64 < 240, i.e. at most 3 blocks: K = 1), and
bf16x6 reaches chunk 2048 only from 128 blocks on (MINIBOONE at K = 6): neither is in the table.

The traced forward takes 32-sample waves (NT = 2) from ceil(n / 32) >= 1024 waves on (pick_nt, nt2_min_waves), i.e. from n = 32737:
n = 32736 is the last batch on 16-sample waves, 32767 and 32769 run NT = 2 with a ragged tail.

Tanh nets only: a ReLU net at these sizes has pre-activations within float32 round-off of the kink, which no float32 implementation
resolves like the float64 oracle (ReLU stays covered at small n, tests/test_hip_train.py)."""

MINIBOONE = ("glow", 43, 215)
HEPMASS = ("realnvp", 21, 105)
NARROW = ("glow", 8, 64)
BIG, SMALL, SAFE = 0, 1, 2
F, B6 = "f16x3", "bf16x6"

CASES = [
    # ---- MINIBOONE Glow, depth 1: probs_small_dev at every chunk, the last chunk ragged in every way
    (*MINIBOONE, 2, 3073, {}, F, False, False, (SMALL, 128, 25)),       # np = 3104 = 24 x 128 + 32: a last chunk of one k-step
    (*MINIBOONE, 2, 4193, {}, F, False, False, (SMALL, 256, 17)),       # np = 4224 = 16 x 256 + 128: four k-steps
    (*MINIBOONE, 2, 8193, {}, F, False, False, (SMALL, 512, 17)),       # np = 8224 = 16 x 512 + 32: one k-step
    (*MINIBOONE, 2, 8193, {}, F, True, False, (SMALL, 512, 17)),        #   ... deterministic: 17 partials per entry
    (*MINIBOONE, 2, 15430, {}, F, False, False, (SMALL, 1024, 16)),     # np = 15456 = 15 x 1024 + 96: three k-steps
    (*MINIBOONE, 2, 16384, {}, F, False, False, (SMALL, 1024, 16)),     # the last batch on probs_small_dev: every chunk full
    (*MINIBOONE, 5, 16384, {}, F, False, False, (SMALL, 2048, 8)),      # 40 blocks: chunk 2048, full
    # ---- ... probs_dev (256 x 256 on one register set, 256 x 64, 64 x 256)
    (*MINIBOONE, 2, 16385, {}, F, False, False, (BIG, 256, 65)),        # the first batch on probs_dev; np = 16416 = 64 x 256 + 32
    (*MINIBOONE, 2, 32736, {}, F, False, False, (BIG, 512, 64)),        # the last batch on 16-sample waves; 63 x 512 + 480: 15 k-steps
    (*MINIBOONE, 2, 32769, {}, F, False, False, (BIG, 512, 65)),        # automatic NT = 2; np = 32800 = 64 x 512 + 32: one k-step
    (*MINIBOONE, 2, 32769, {}, F, True, False, (BIG, 512, 65)),         #   ... deterministic: 65 partials per entry
    (*MINIBOONE, 3, 32850, {}, F, False, False, (BIG, 1024, 33)),       # np = 32864 = 32 x 1024 + 96: three k-steps
    (*MINIBOONE, 5, 32767, {}, F, False, False, (BIG, 2048, 16)),       # NT = 2 with a row short of a full batch; every chunk full
    # ---- ... depth 0 and depth 2
    (*MINIBOONE, 4, 32769, {"depth": 0}, F, False, False, (BIG, 1024, 33)),
    (*MINIBOONE, 2, 16417, {"depth": 2}, F, False, False, (BIG, 512, 33)),      # np = 16448 = 32 x 512 + 64
    # ---- ... the bf16x6 trainer (wgrad_safe_kernel) above chunk 128
    (*MINIBOONE, 2, 8193, {}, B6, False, False, (SAFE, 256, 33)),
    (*MINIBOONE, 2, 16385, {}, B6, False, False, (SAFE, 512, 33)),
    (*MINIBOONE, 2, 16385, {}, B6, True, False, (SAFE, 512, 33)),
    (*MINIBOONE, 2, 32769, {}, B6, False, False, (SAFE, 1024, 33)),
    # ---- a geometry whose lists hold only 64-edge blocks
    (*NARROW, 4, 16384, {}, F, False, False, (SMALL, 512, 32)),
    (*NARROW, 4, 32769, {}, F, False, False, (BIG, 1024, 33)),
    # ---- HEPMASS RealNVP with BatchNorm: running statistics around the NT switch, batch statistics around the 16384 switch
    (*HEPMASS, 3, 32767, {}, F, False, False, (BIG, 2048, 16)),
    (*HEPMASS, 3, 32769, {}, F, False, False, (BIG, 2048, 17)),
    (*HEPMASS, 3, 16383, {}, F, False, True, (SMALL, 1024, 16)),        # the last call of bn_stats_kernel (one block per slot)
    (*HEPMASS, 3, 16384, {}, F, False, True, (SMALL, 1024, 16)),        # the first three-launch call: 64 row chunks of 256
    (*HEPMASS, 3, 16385, {}, F, False, True, (BIG, 1024, 17)),          # per = 257: a short last row chunk (194 rows)
    (*HEPMASS, 3, 16385, {}, B6, False, True, (SAFE, 512, 33)),         #   ... on the bf16x6 trainer
    (*HEPMASS, 3, 32769, {}, F, False, True, (BIG, 2048, 17)),          # the three-launch form under the automatic NT = 2 forward
    (*HEPMASS, 2, 20001, {"depth": 2}, F, False, True, (BIG, 1024, 20)),
]

# the fused step (gbnf_trainer_nll_step) on batch statistics, three-launch form with a short last row chunk
FUSED_STEP_CASE = (*HEPMASS, 3, 16385, {})


def padded(n):
    """Rows of the trainer's buffers at a batch of n (TrainLayout::padded: whole 32-row workgroups)."""
    return (n + 31) // 32 * 32


def last_chunk_ksteps(case):
    """k-steps (32 samples each) of the last sample chunk of a case's weight-gradient launch, from its expected plan."""
    n, (_, chunk, Y) = case[4], case[9]
    last = padded(n) - (Y - 1) * chunk
    assert 0 < last <= chunk and last % 32 == 0, case
    return last // 32


def case_id(case):
    kind, d, h, K, n, kw, math, det, bs, _ = case
    extra = "".join(f"_{k}{v}" for k, v in sorted(kw.items()))
    return f"{kind}_d{d}_h{h}_K{K}{extra}_n{n}_{math}" + ("_det" if det else "") + ("_bstats" if bs else "")


def oracle_key(case):
    """What the float64 oracle's results depend on: the geometry, n and the BatchNorm mode (not the math mode, not determinism)."""
    kind, d, h, K, n, kw, _, _, bs, _ = case
    return (kind, d, h, K, n, tuple(sorted(kw.items())), bs)


def make_inputs(case):
    """(spec, x, g_z, g_ldj) of a case: the same on the host and on the device."""
    import numpy as np
    from gbnf_amd import synth
    kind, d, h, K, n, kw = case[:6]
    seed = 7000 + 13 * K + (n % 1000)
    spec = synth.synth_glow_spec(d, h, K, seed=seed, **kw) if kind == "glow" else synth.synth_realnvp_spec(d, h, K, seed=seed, flip_init=n % 2, **kw)
    x = synth.synth_batch(n, d, seed=seed + 1)
    rng = np.random.RandomState(seed + 2)
    g_z = rng.standard_normal(x.shape).astype(np.float32)
    g_l = rng.standard_normal(n).astype(np.float32)
    return spec, x, g_z, g_l


# ---- what the table must cover between its cases (a change of the table that drops one of these fails at import) -------------------
assert 20 <= len(CASES) <= 30
assert len({case_id(c) for c in CASES}) == len(CASES)
assert all(2 <= c[3] <= 5 for c in CASES)
assert all(c[5].get("act", "tanh") == "tanh" and c[5].get("coupling_network", "tanh") == "tanh" for c in CASES)       # Tanh nets only
assert all((c[9][0] == SAFE) == (c[6] == B6) for c in CASES)
assert all((c[9][0] == SMALL) == (padded(c[4]) <= 16384) for c in CASES if c[6] == F)
_f16 = [c for c in CASES if c[6] == F]
# geometries: MINIBOONE at every depth, HEPMASS with BatchNorm, a geometry of 64-edge blocks only
assert {c[5].get("depth", 1) for c in CASES if c[:3] == MINIBOONE} == {0, 1, 2}
assert any(c[:3] == HEPMASS for c in CASES) and any(c[:3] == NARROW for c in CASES)
# lists and chunks
assert {c[9][1] for c in _f16 if c[9][0] == SMALL} == {128, 256, 512, 1024, 2048}
assert {c[9][1] for c in _f16 if c[9][0] == BIG} == {256, 512, 1024, 2048}          # (chunk 128 on probs_dev needs K = 1: see above)
assert any(c[:4] == (*MINIBOONE, 5) and c[4] >= 32737 and c[9][:2] == (BIG, 2048) for c in CASES)
assert any(c[:5] == (*MINIBOONE, 5, 16384) and c[9] == (SMALL, 2048, 8) for c in CASES)
# bf16x6 at two chunk values or more above 128
assert len({c[9][1] for c in CASES if c[6] == B6 and c[9][1] > 128}) >= 2
# ragged last chunks on each f16x3 list: one k-step with n = Y' chunk + 1, an odd number of k-steps above 1, full
for _list in (SMALL, BIG):
    _on = [c for c in _f16 if c[9][0] == _list and c[:3] == MINIBOONE]
    assert any(last_chunk_ksteps(c) == 1 and c[4] == (c[9][2] - 1) * c[9][1] + 1 for c in _on), _list
    assert any(last_chunk_ksteps(c) > 1 and last_chunk_ksteps(c) % 2 == 1 for c in _on), _list
    assert any(last_chunk_ksteps(c) * 32 == c[9][1] for c in _on), _list
# the list boundary on one geometry
assert {c[4] for c in _f16 if c[:4] == (*MINIBOONE, 2) and not c[7]} >= {16384, 16385}
# deterministic mode: each f16x3 list and bf16x6, Y >= 4 and chunk >= 512
for _list in (SMALL, BIG, SAFE):
    assert any(c[7] and c[9][0] == _list and c[9][2] >= 4 and c[9][1] >= 512 for c in CASES), _list
# every deterministic case has its twin with the mode off
assert all(any(d[:7] == c[:7] and not d[7] and d[8:] == c[8:] for d in CASES) for c in CASES if c[7])
# batch statistics around the switch of launch_bn_stats, under NT = 2, and at depth 2
_bs = [c for c in CASES if c[8]]
assert all(c[0] == "realnvp" for c in _bs)
assert {c[4] for c in _bs if c[6] == F and c[5].get("depth", 1) == 1} >= {16383, 16384, 16385, 32769}
assert any(c[5].get("depth") == 2 and 19000 <= c[4] <= 21000 for c in _bs)
# the automatic NT = 2 forward: a Glow and a RealNVP at 32769, 32767, and the last batch on 16-sample waves
for _kind in ("glow", "realnvp"):
    assert any(c[0] == _kind and c[4] == 32769 and c[6] == F and not c[7] for c in CASES)
    assert any(c[0] == _kind and c[4] == 32767 for c in CASES)
assert any(c[4] == 32736 for c in CASES)
assert FUSED_STEP_CASE[:3] == HEPMASS and FUSED_STEP_CASE[4] == 16385
