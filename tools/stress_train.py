#!/usr/bin/env python3
"""Randomised stress of the training kernels against the float64 autograd oracle (many more geometries than the test
suite runs; opt-in, GPU).  usage: python tools/stress_train.py [cases] [seed]

Lines: ok / KINK / FAIL.  KINK = a ReLU network whose gradient differs from the float64 oracle because f32 round-off put
a pre-activation of magnitude ~1e-7 on the other side of zero for one sample (expected about 1e-6 * n * h * layers * K
times per case; one such sample changes a weight gradient by ~1/sqrt(n) of its largest entry).  The tool tells it from a
kernel error by re-running the oracle with the ReLU threshold at -5e-6 and +5e-6, and -- where that bracket does not explain the case -- by
asking the per-step kernels (another float32 implementation) for the same gradients: tanh networks never show it."""
import os, sys
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT); sys.path.insert(0, os.path.join(ROOT, "tests"))
import numpy as np, torch
from gbnf_amd import native, synth
from oracle import gbnf_oracle as oracle
from test_hip_train import _dev_spec, _check_grads, G_RTOL

def gen_case(rng, k):
    """Case k of the stream `rng` (the draw order is part of the tool: tools/debug_train_case.py replays it)."""
    kind = "glow" if rng.randint(3) else "realnvp"
    d = int(rng.choice([2, 3, 5, 6, 8, 13, 21, 33, 43, 50, 63, 64]))
    h = int(rng.choice([5, 16, 30, 33, 64, 105, 129, 215, 256, 257, 315, 430, 512]))
    K = int(rng.randint(1, 7))
    if os.environ.get("GBNF_STRESS_K"):          # e.g. GBNF_STRESS_K=13,24: long flows (the chained sweeps take K <= 24 since round 6; same draw count)
        lo, hi = (int(v) for v in os.environ["GBNF_STRESS_K"].split(","))
        K = lo + (K * 7919 + k) % (hi - lo + 1)
    n = int(rng.choice([1, 2, 15, 16, 17, 31, 32, 33, 100, 257, 1000, 1537, 2049, 3000]))
    depth = int(rng.choice([0, 1, 1, 1, 2]))
    if kind == "glow":
        extra = dict(act=str(rng.choice(["tanh", "relu", "random"])), coupling=str(rng.choice(["affine", "additive"])),
                     permutation=str(rng.choice(["shuffle", "reverse"])), depth=depth)
        spec = synth.synth_glow_spec(d, h, K, seed=5000 + k, **extra)
    else:
        extra = dict(coupling_network=str(rng.choice(["tanh", "relu", "mixed", "random", "residual"])), batch_norm=bool(rng.randint(2)),
                     flip_init=int(rng.randint(2)), depth=depth)
        if extra["coupling_network"] == "residual":
            extra["depth"] = 1 if depth < 2 else 2          # blocks: mostly one (the register-chained kernels), sometimes two (per-step kernels)
        spec = synth.synth_realnvp_spec(d, h, K, seed=5000 + k, **extra)
    return kind, d, h, K, n, extra, spec


def main():
    # [CASES [SEED]] [--math f16x3|bf16x6|repair]: the trainer's math mode; a range-safe mode draws a quarter of the cases with one row
    # beyond the fp16 range (as tools/stress_image.py does) and no case counts as BLOWN for having left it
    argv = list(sys.argv[1:])
    math = "f16x3"
    if "--math" in argv:
        k = argv.index("--math")
        math = argv[k + 1]
        del argv[k:k + 2]
    if math not in ("f16x3", "bf16x6", "repair"):
        sys.exit("--math must be f16x3, bf16x6 or repair")
    safe = math != "f16x3"
    cases = int(argv[0]) if len(argv) > 0 else 60
    rng = np.random.RandomState(int(argv[1]) if len(argv) > 1 else 2024)
    dev = torch.device("cuda:0")
    bad = 0
    skipped = 0
    for k in range(cases):
        kind, d, h, K, n, extra, spec = gen_case(rng, k)
        tag = f"{kind} d={d} h={h} K={K} n={n} {extra}"
        try:
            tr = native.NativeTrainer(_dev_spec(spec, dev), math=math)
        except native.GbnfError as e:
            print("skip (unsupported):", tag, "|", str(e)[:80])
            skipped += 1
            continue
        x = synth.synth_batch(n, d, seed=k)
        if safe and k % 4 == 3:
            x[(7 * k) % n, :] = np.float32(3.0e5)
            tag += " out-of-range row"
        gscale = np.float32(10.0 ** rng.uniform(-6, 4))          # the scale of the caller's loss is arbitrary
        g_z = rng.standard_normal(x.shape).astype(np.float32) * gscale
        g_l = rng.standard_normal(n).astype(np.float32) * gscale
        xd = torch.from_numpy(x).to(dev)
        grads = None
        try:
            native.saturation_count(reset=True)
            z, ldj, trace = tr.forward(xd, want_trace=True)
            z64, ldj64 = oracle.component_forward(spec, x, backend="numpy64")
            n_sat = native.saturation_count(reset=True)
            if (n_sat > 0 and not safe) or not (np.isfinite(z64).all() and np.isfinite(ldj64).all()):
                # an exploding model (long RealNVPs without BatchNorm on random weights): the float64 oracle overflows, or hidden operands
                # left the fp16 range and the library SAYS so (gbnf_saturation_count: BoostedFlow.check_numerics raises on it) -- not a case
                print("BLOWN", tag, f"| the library's saturation counter: {n_sat}; float64 oracle finite: {bool(np.isfinite(z64).all())}")
                continue
            e_l = float(np.abs(ldj.cpu().numpy() - ldj64).max() / max(1.0, float(np.abs(ldj64).max())))
            e_z = float(np.abs(z.cpu().numpy() - z64).max() / max(1.0, float(np.abs(z64).max())))
            if e_l > 1e-5 or e_z > 2e-5:
                # the forward sweep is off the float64 oracle: conditioning (long flows, exploding scales) or a kernel?  The float32
                # oracle -- the reference's own arithmetic -- is the witness, as in tools/stress_eval.py
                z32, ldj32 = oracle.component_forward(spec, x, backend="torch")
                o_l = float(np.abs(ldj32 - ldj64).max() / max(1.0, float(np.abs(ldj64).max())))
                o_z = float(np.abs(z32 - z64).max() / max(1.0, float(np.abs(z64).max())))
                cond = e_l <= max(1e-5, 3.0 * o_l) and e_z <= max(2e-5, 3.0 * o_z)
                print("COND" if cond else "FAIL", tag, f"| forward: ldj {e_l:.1e} z {e_z:.1e} off float64; the f32 oracle itself: ldj {o_l:.1e} z {o_z:.1e}")
                bad += 0 if cond else 1
                continue
            gx64, grads64 = oracle.component_grads(spec, x, g_z, g_l)
            gx, grads = tr.backward(xd, torch.from_numpy(g_z).to(dev), torch.from_numpy(g_l).to(dev), want_gx=True, trace=trace)
            _check_grads(grads, grads64, tag, floor=1e-3 * float(gscale))
            assert np.abs(gx.cpu().numpy() - gx64).max() <= G_RTOL * max(float(np.abs(gx64).max()), 1e-3 * float(gscale)), "gx"
            gx2, grads2 = tr.backward(xd, torch.from_numpy(g_z).to(dev), torch.from_numpy(g_l).to(dev), want_gx=True, trace=None)
            assert np.abs(gx2.cpu().numpy() - gx64).max() <= G_RTOL * max(float(np.abs(gx64).max()), 1e-3 * float(gscale)), "gx (no trace)"
            print("ok  ", tag)
        except AssertionError as e:
            # is it the kernels or the problem?  A ReLU net's gradient jumps when a pre-activation crosses zero, and f32
            # round-off (~1e-6 absolute on a sum of h products) decides the side for the few pre-activations that close to
            # zero (expected count ~ 1e-6 * n * h * layers * K).  Bracket: the oracle with the ReLU threshold at -tol and
            # +tol; an entry of a gradient is fine if it lies in the interval those two and the plain oracle span.
            tol = 5e-6
            _, g_lo = oracle.component_grads(spec, x, g_z, g_l, relu_shift=-tol)
            _, g_hi = oracle.component_grads(spec, x, g_z, g_l, relu_shift=+tol)
            worst_out, errs = 0.0, []
            for i, (a, b) in enumerate(zip(grads, grads64)):
                if b is None:
                    continue
                a = a.cpu().numpy().reshape(b.shape).astype(np.float64)
                lo = np.minimum(np.minimum(g_lo[i], g_hi[i]), b); hi = np.maximum(np.maximum(g_lo[i], g_hi[i]), b)
                out = np.maximum(np.maximum(lo - a, a - hi), 0.0).max() / max(np.abs(b).max(), 1e-3 * float(gscale))
                worst_out = max(worst_out, float(out))
                errs.append((float(np.abs(a - b).max() / max(np.abs(b).max(), 1e-3 * float(gscale))), i, b.shape))
            errs = sorted(errs, reverse=True)[:3]
            # (the bracket moves ALL near-zero units together, round-off moves an arbitrary subset: entries that several
            # of them touch may stay a little outside -- a kink explains the case if most of the deviation is gone)
            kink = worst_out <= max(G_RTOL, 0.2 * errs[0][0])
            if not kink:
                # second witness: the per-step kernels, another float32 implementation of the same step.  A kink moves with the
                # implementation (it deviates from the float64 oracle by as much, on the same tensors or on others); a kernel error of
                # the register-chained path does not show there.  (Pre-activations of 430 .. 512 products carry ~1e-5 of float32
                # round-off: more than the bracket's 5e-6 -- tools/debug_train_case.py replays a case with wider brackets)
                try:
                    _, grads_ps = tr.backward(xd, torch.from_numpy(g_z).to(dev), torch.from_numpy(g_l).to(dev), trace=None)
                    dev_ps = max(float(np.abs(a.cpu().numpy().reshape(b.shape).astype(np.float64) - b).max() / max(np.abs(b).max(), 1e-3 * float(gscale)))
                                 for a, b in zip(grads_ps, grads64) if b is not None)
                    kink = dev_ps >= 0.3 * errs[0][0]
                except Exception:
                    pass
            if not kink:
                # third witness: the float64 forward itself -- the smallest |ReLU pre-activation| of the batch.  One within float32
                # round-off of zero (a few 1e-6 for sums of 256 .. 512 split-f16 products) is a sample whose path a float32 kernel may
                # legitimately take the other way: its whole contribution moves (1 / n of a gradient's scale, on the layers below it)
                class _MinOps(oracle._TorchGradOps):
                    smallest = float("inf")
                    def relu(self, a):
                        _MinOps.smallest = min(_MinOps.smallest, float(a.detach().abs().min()))
                        return torch.relu(a)
                mops = _MinOps()
                zt, ldt = torch.tensor(x.astype(np.float64)), mops.zeros(n)
                for st_ in spec["steps"]:
                    if kind == "glow":
                        zt, ldt = oracle.glow_step(mops, spec, st_, zt, ldt)
                    else:
                        zt, sl_ = oracle.realnvp_step(mops, spec, st_, zt)
                if _MinOps.smallest < 5e-6:
                    kink = True
                    print(f"     (smallest |ReLU pre-activation| of the batch in float64: {_MinOps.smallest:.1e})")
            bad += 0 if kink else 1
            print("KINK" if kink else "FAIL", tag, "| worst tensors", [(f"{e:.1e}", i, sh) for e, i, sh in errs],
                  f"| outside the ReLU-threshold bracket by {worst_out:.1e}")
    print(f"{cases} cases, {skipped} skipped as unsupported, {bad} failures")
    if skipped == cases:
        sys.exit("every case was skipped as unsupported: nothing was tested")
    sys.exit(1 if bad else 0)


if __name__ == "__main__":
    main()
