#!/usr/bin/env python3
"""The score grad_x log p(x) of the image path: BASELINE.json configs[3] (3 x 32 x 32, K = 8, L = 2, h = 256), one component and
the C = 4 boosted model, at batch 64 and 256.

    python tools/bench_image_score.py [--batches 64,256] [--components 4] [--steps 20] [--reps 5] [--warmup 5] [--skip-eager]

Per batch, each line the median / min / max over ``reps`` windows of ``steps`` calls, same build, same process, same warm-up:
  component_score   BoostedFlow(args).component_score(x, 0, noise): forward, seed and the data-gradient-only backward in one call
  fwd_bwd_weights   native.NativeImageTrainer forward + the unchanged gbnf_image_trainer_backward (weight gradients, no g_x): what
                    the library could do for an input gradient's cost before -- (a) = fwd_bwd_weights / component_score is what
                    dropping the weight gradients saves, although the left side also computes the last adjoint
  score             BoostedFlow(args).score(x, noise=noise) of the C-component model: ONE library call
  (b)               C x component_score / score
  eager             the same mixture score from the float32 form of the yardstick restatement (tests/image_grad_oracle.py) under
                    PyTorch eager autograd on the card, x the only leaf (no weight gradients there either); (c) = eager / score
"""
import argparse
import json
import os
import statistics
import sys
import time

import numpy as np
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tests"))

import image_grad_oracle as igo  # noqa: E402
from gbnf_amd import BoostedFlow, image_glow, native, synth  # noqa: E402


def timed(fn, steps, reps, warmup):
    for _ in range(warmup):
        fn()
    out = []
    for _ in range(reps):
        torch.cuda.synchronize()
        t0 = time.perf_counter()
        for _ in range(steps):
            fn()
        torch.cuda.synchronize()
        out.append(1e3 * (time.perf_counter() - t0) / steps)
    return {"ms_median": statistics.median(out), "ms_min": min(out), "ms_max": max(out)}


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--batches", default="64,256")
    ap.add_argument("--components", type=int, default=4)
    ap.add_argument("--steps", type=int, default=20)
    ap.add_argument("--reps", type=int, default=5)
    ap.add_argument("--warmup", type=int, default=5)
    ap.add_argument("--K", type=int, default=8)
    ap.add_argument("--L", type=int, default=2)
    ap.add_argument("--hidden", type=int, default=256)
    ap.add_argument("--skip-eager", action="store_true")
    a = ap.parse_args()
    dev = torch.device("cuda:0")
    C = a.components
    specs = [synth.synth_image_glow_spec((3, 32, 32), h=a.hidden, K=a.K, L=a.L, seed=3 + c) for c in range(C)]
    args = argparse.Namespace(
        num_flows=a.K, z_size=3072, density_evaluation=True, device=dev, cuda=True, component_type="glow", num_components=C,
        rho_init="decreasing", learn_top=True, y_classes=0, y_condition=False, sample_size=4, input_size=[3, 32, 32], h_size=a.hidden,
        num_blocks=a.L, actnorm_scale=1.0, flow_permutation="invconv", flow_coupling="affine", LU_decomposed=False,
        num_dequant_blocks=0, coupling_network="tanh", coupling_network_depth=1, batch_norm=False)
    m = BoostedFlow(args)
    for c, sp in enumerate(specs):
        image_glow.load_image_spec(m.flows[c], sp)
    m.eval()
    tr = native.NativeImageTrainer(igo.dev_spec(specs[0], dev))
    rho = m.rho.detach().double()
    log_w = torch.log(rho / rho.sum()).float().view(-1, 1)
    P = [{k: v.detach().to(dev).float() for k, v in igo.leaf_params(sp, torch.float32).items()} for sp in specs]
    out = {"workload": f"image score 3x32x32 K={a.K} L={a.L} h={a.hidden} C={C}", "steps": a.steps, "reps": a.reps, "warmup": a.warmup,
           "batches": {}}
    for batch in (int(b) for b in a.batches.split(",")):
        x, noise = synth.synth_image_batch(batch, seed=4)
        xd, nd = torch.from_numpy(x).to(dev), torch.from_numpy(noise).to(dev)
        g_ldj = torch.ones(batch, device=dev)
        flat = torch.zeros(tr.grad_floats, device=dev)

        def fwd_bwd_weights():
            z, ldj, trace = tr.forward(xd, nd)
            flat.zero_()
            tr.backward(trace, z, g_ldj, out=flat)

        res = {"component_score": timed(lambda: m.component_score(xd, 0, nd), a.steps, a.reps, a.warmup),
               "fwd_bwd_weights": timed(fwd_bwd_weights, a.steps, a.reps, a.warmup),
               "score": timed(lambda: m.score(xd, noise=nd), a.steps, a.reps, a.warmup)}
        res["a_weights_over_score"] = res["fwd_bwd_weights"]["ms_median"] / res["component_score"]["ms_median"]
        res["b_components_over_score"] = C * res["component_score"]["ms_median"] / res["score"]["ms_median"]
        if not a.skip_eager:
            def eager():
                xl = xd.clone().requires_grad_(True)
                ll = torch.stack([igo.forward(specs[c], P[c], xl, nd)["ll"] for c in range(C)])
                torch.logsumexp(ll + log_w, dim=0).sum().backward()
                return xl.grad
            res["eager"] = timed(eager, max(a.steps // 4, 1), a.reps, max(a.warmup // 2, 1))
            res["c_eager_over_score"] = res["eager"]["ms_median"] / res["score"]["ms_median"]
            ref, got = eager(), m.score(xd, noise=nd)
            res["max_abs_diff_vs_eager_over_max"] = float((ref - got).abs().max() / ref.abs().max())
        out["batches"][str(batch)] = res
    print(json.dumps(out))


if __name__ == "__main__":
    main()
