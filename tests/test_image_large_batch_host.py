"""Host (no GPU): what tests/test_hip_image_large_batch.py relies on.

1. Regimes.  Every case of tests/image_large_batch_cases.py reaches the launch regime it is listed for, computed from the Python
   restatements of wgrad_shape, the seed's bpc and an_launch_stats (the device test anchors the slice counts to the library).
2. Yardstick margin.  The float32 run of the float64 yardstick (image_grad_oracle.grads on float32 leaves) stays within
   G_RTOL / 20 = 1e-5 of it, in the measure of _check_grads; the float32 oracle.image_actnorm_init within MARGIN = 1e-6 on A1, A2.  A
   device result outside G_RTOL is then a kernel finding, not float32 arithmetic.
3. Kinks.  A multi-image batch of a ReLU net cannot be kink-free: the share of ReLU pre-activations inside kink_report's margin is
   at most 2e-4 per tensor -- and (2) shows that these do not move the answer.

Measured (float32 against float64 gradients / worst kink share): W1 7.4e-6 / 5.8e-5, W2 1.1e-6 / 1.1e-4, W3 9.3e-7 / 5.1e-5,
W4 1.1e-6 / 6.6e-5, W5 8.7e-7 / 6.3e-5; ActNorm2d init float32 against float64: A1 4.2e-7, A2 2.1e-7.  The float32 figures depend on
the order in which the host's convolution adds (thread count, instruction set): W1 gave 4.6e-6 to 7.4e-6 and W4 1.1e-6 to 3.1e-6 on 1,
4 and 8 threads -- the worst tensor of W1 is the last 3x3's bias gradient, a float32 sum of 10240 terms."""
import numpy as np
import pytest

import image_actnorm_init_cases as aic
import image_grad_oracle as igo
import image_large_batch_cases as T


def _row(rows, what):
    return next(r for r in rows if r["what"] == what)


def test_w1_caps_the_wide_1x1_launch():
    rows = T.launch_table("W1")
    wide = _row(rows, "level 0 step 0 conv 1")
    assert (wide["cout"], wide["cin"], wide["ks"]) == (256, 256, 1)
    assert (wide["blocks"], wide["items"], wide["wanted"], wide["slices"]) == (16, 160, 80, 64) and wide["capped"]
    assert wide["per_slice"] == (2, 3) and wide["empty"] == []
    others = [r for r in rows if r is not wide]
    assert sorted(r["slices"] for r in others) == [27, 40, 80] and not any(r["capped"] for r in others)
    assert T.seed_bpc("W1") == (4, 10, 10)


def test_w2_caps_the_seed_and_leaves_most_items_outside_the_map():
    Cz, bpc, wanted = T.seed_bpc("W2")
    assert (Cz, bpc, wanted) == (64, 4, 5)
    n = T.CASES["W2"][2]
    assert n > 256                                         # the seed's row loop: more rows than the 256 threads of workgroup 0
    assert T.levels(T.CASES["W2"][0], 1) == [(64, 16, 2, 2)]
    assert -(-(n - 1) * 2 * 2 // T.SEED_ENTRIES) == T.OPT_MAX_PARTIALS // Cz          # one image fewer: 4 wanted, the cap does not bind
    rows = T.launch_table("W2")
    assert [(r["slices"], r["capped"]) for r in rows] == [(1024, True), (1024, True), (1024, True), (684, False)]
    for r in rows:
        assert r["blocks"] == 1 and r["slices"] % 4 == 0, r["what"]
        assert r["per_slice"][0] < r["per_slice"][1]       # n is odd: the items do not divide
        assert r["empty"] == [y for y in range(r["slices"]) if y % 4], r["what"]        # only strip 0 holds rows of the 2 x 2 map


def test_w3_has_slices_entirely_outside_the_map():
    assert T.levels(T.CASES["W3"][0], 1) == [(4, 16, 6, 16)]
    rows = T.launch_table("W3")
    for what in ("level 0 step 0 mix", "level 0 step 0 conv 1"):
        r = _row(rows, what)
        assert r["ks"] == 1 and (r["items"], r["slices"], r["blocks"]) == (128, 64, 1) and not r["capped"]
        assert r["empty"] == [y for y in range(64) if y % 4 >= 2]          # strips 2 and 3 start at rows 8 and 12 of a 6-row map
    last = _row(rows, "level 0 step 0 conv 2")
    assert last["slices"] == 32 and len(last["empty"]) == 16
    first = _row(rows, "level 0 step 0 conv 0")
    assert first["slices"] % 4 != 0 and first["empty"] == []               # a slice count that mixes the strips


def test_w4_is_the_two_level_shape():
    size, kw, n, _ = T.CASES["W4"]
    assert (size, kw["L"]) == ((3, 32, 32), 2)
    assert T.levels(size, 2) == [(12, 16, 16, 16), (24, 8, 8, 8)]
    rows = T.launch_table("W4")
    assert any(r["what"] == "level 0 split" for r in rows)
    assert (min(r["slices"] for r in rows), max(r["slices"] for r in rows)) == (8, 48) and not any(r["capped"] for r in rows)
    assert T.seed_bpc("W4") == (24, 2, 2)
    from gbnf_amd import synth
    assert synth.synth_image_glow_spec(size, seed=1, **kw)["learn_top"] is not None


def test_w5_caps_the_two_halves_net():
    size, kw, n, _ = T.CASES["W5"]
    assert kw["h"] > 256 and n == 16
    wide = _row(T.launch_table("W5"), "level 0 step 0 conv 1")
    assert (wide["blocks"], wide["items"], wide["wanted"], wide["slices"]) == (36, 64, 32, 28) and wide["capped"]
    assert wide["per_slice"] == (2, 3)


def test_deterministic_reduce_runs_its_unrolled_loop_and_its_tail():
    """img_train_wgrad_reduce_kernel adds 8 slices at a time, then the rest: the deterministic cases have launches with whole
    eights only, with a tail only past several eights, and with more slices than any small case (18)."""
    slices = {name: [r["slices"] for r in T.launch_table(name)] for name in ("W1", "W3", "W5")}
    flat = [s for v in slices.values() for s in v]
    assert any(s % 8 == 0 and s >= 64 for s in flat)
    assert any(s % 8 != 0 and s > 18 for s in flat)
    assert 27 in slices["W1"] and 28 in slices["W5"] and 22 in slices["W3"]


def test_init_cases_reach_the_chunk_cap_and_a_short_last_chunk():
    size, kw, n = T.INIT_CASES["A1"]
    assert T.levels(size, kw["L"]) == [(4, 16, 16, 16)]
    per, chunks, group = T.an_chunks(16, n)
    assert -(-n // group) > T.AN_MAX_CHUNKS                      # the cap binds
    assert (per, chunks, group) == (8, 33, 4) and n - (chunks - 1) * per == 3          # ... and the last chunk leaves wave 3 idle
    size, kw, n = T.INIT_CASES["A2"]
    assert [H for _, H, _, _ in T.levels(size, kw["L"])] == [16, 8]
    assert T.an_chunks(8, n) == (16, 2, 16) and n - 16 == 7
    assert T.an_chunks(16, n) == (4, 6, 4)
    # the largest batch of the earlier tests stays below the cap on either storage
    assert T.an_chunks(16, 40)[1] == 10 and T.an_chunks(8, 40)[1] == 3


@pytest.mark.parametrize("name", sorted(T.CASES))
def test_float32_yardstick_stays_inside_the_margin(name):
    out64, ref64 = T.grads(name)
    out32, ref32 = T.grads(name, True, "float32")
    worst = T.worst_grad_error(ref32, ref64)
    ez = float((out32["z"].double() - out64["z"]).abs().max()) / float(out64["z"].abs().max())
    print(f"[image large batch host] {name}: float32 against float64: gradients {worst:.2e} of {T.F32_MARGIN:.0e}, z {ez:.2e}")
    assert worst <= T.F32_MARGIN


@pytest.mark.parametrize("name", sorted(T.CASES))
def test_kink_share_is_capped(name):
    spec, x, noise, _, _ = T.make_case(name)
    rows = igo.kink_report(spec, x, noise)
    assert rows
    share = max(inside / units for inside, units in rows)
    print(f"[image large batch host] {name}: worst share of ReLU pre-activations inside the kink margin {share:.2e} of {T.KINK_SHARE:.0e}")
    assert share <= T.KINK_SHARE


@pytest.mark.parametrize("name", sorted(T.INIT_CASES))
def test_float32_init_oracle_stays_inside_the_margin(name):
    w = aic.worst(T.init_oracle(name, "float32"), T.init_oracle(name))
    print(f"[image large batch host] {name}: float32 ActNorm2d init against float64 {w:.2e} of {aic.MARGIN:.0e}")
    assert w <= aic.MARGIN
    assert max(float(np.abs(l).max()) for _, l in T.init_oracle(name)) < 10.0          # logs of order one: the bar is absolute, in effect
