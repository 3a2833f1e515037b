#!/usr/bin/env python3
"""Training step (forward + backward) of ONE image Glow component: BASELINE.json configs[3] (3 x 32 x 32, K = 8, L = 2, h = 256) at
batch 64.

    python tools/bench_image_train.py [--batch 64] [--steps 50] [--reps 5] [--warmup 5] [--K 8] [--hidden 256] [--skip-eager]
                                      [--deterministic]

Three lines, each the median / min / max over ``reps`` windows of ``steps`` steps, in this process order with the same warm-up:
  module   the user-facing step: BoostedFlow(args) in train mode, model.component_forward(x, 0, noise), nll = -mean(ll), nll.backward()
           (HIP forward and backward, the 1x1 log-determinants and the learned top prior in torch: everything the loop needs)
  eager    the SAME nll from the float32 form of the yardstick restatement (tests/image_grad_oracle.py) under PyTorch eager autograd
  library  native.NativeImageTrainer forward + backward alone with a hand-made seed (no 1x1 log-determinants, no prior, no autograd):
           the kernels' share of the module line, NOT comparable with the eager line
plus the arithmetic floor (3 x the forward's multiply-adds at the 155 TF/s f32-MFMA peak).  Per-kernel times: run it under
`rocprofv3 --kernel-trace --stats -- python tools/bench_image_train.py --skip-eager --reps 1` (a run of its own).
``--deterministic``: the module and library lines in the image trainer's deterministic mode (ordered weight-gradient and log-det sums);
the output then also carries the forward / backward workspace bytes of both modes."""
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


def nll_of(z, z_mu, z_var, ldj):
    return -((-0.5 * (z_var + (z - z_mu) ** 2 * (-z_var).exp())).sum(dim=[1, 2, 3]) + ldj).mean()


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--batch", type=int, default=64)
    ap.add_argument("--steps", type=int, default=50)
    ap.add_argument("--reps", type=int, default=5)
    ap.add_argument("--warmup", type=int, default=5)
    ap.add_argument("--K", type=int, default=8)
    ap.add_argument("--L", type=int, default=2)
    ap.add_argument("--hidden", type=int, default=256)
    ap.add_argument("--skip-eager", action="store_true")
    ap.add_argument("--deterministic", action="store_true")
    a = ap.parse_args()
    dev = torch.device("cuda:0")
    sp = synth.synth_image_glow_spec((3, 32, 32), h=a.hidden, K=a.K, L=a.L, seed=3)
    x, noise = synth.synth_image_batch(a.batch, seed=4)
    xd, nd = torch.from_numpy(x).to(dev), torch.from_numpy(noise).to(dev)
    macs = native.NativeImageFlow(sp, math="f32").macs_per_image
    out = {"workload": f"image train step 3x32x32 K={a.K} L={a.L} h={a.hidden} batch={a.batch}", "steps": a.steps, "reps": a.reps,
           "warmup": a.warmup, "deterministic": bool(a.deterministic), "floor_ms": 1e3 * 3 * 2 * macs * a.batch / 155e12}

    args = argparse.Namespace(
        num_flows=a.K, z_size=3072, density_evaluation=True, device=dev, cuda=True, component_type="glow", num_components=1,
        rho_init="decreasing", learn_top=True, y_classes=0, y_condition=False, sample_size=4, input_size=[3, 32, 32], h_size=a.hidden,
        num_blocks=a.L, actnorm_scale=1.0, flow_permutation="invconv", flow_coupling="affine", LU_decomposed=False,
        num_dequant_blocks=0, coupling_network="tanh", coupling_network_depth=1, batch_norm=False, image_deterministic=bool(a.deterministic))
    m = BoostedFlow(args)
    image_glow.load_image_spec(m.flows[0], sp)
    m.train()

    def module_step():
        m.zero_grad(set_to_none=True)
        nll_of(*m.component_forward(xd, 0, nd)[:4]).backward()
    out["module"] = timed(module_step, a.steps, a.reps, a.warmup)
    out["module"]["images_per_s"] = 1e3 * a.batch / out["module"]["ms_median"]

    if not a.skip_eager:
        P = {k: v.detach().to(dev).float().requires_grad_(True) for k, v in igo.leaf_params(sp, torch.float32).items()}

        def eager_step():
            for p in P.values():
                p.grad = None
            o = igo.forward(sp, P, xd, nd)
            nll_of(o["z"], o["z_mu"], o["z_var"], o["ldj"]).backward()
        out["eager"] = timed(eager_step, a.steps, a.reps, a.warmup)
        out["eager"]["images_per_s"] = 1e3 * a.batch / out["eager"]["ms_median"]
        out["module_over_eager"] = out["eager"]["ms_median"] / out["module"]["ms_median"]

    tr = native.NativeImageTrainer(igo.dev_spec(sp, dev), deterministic=a.deterministic)
    if a.deterministic:
        out["workspace_bytes"] = tr.workspace_bytes(a.batch)
        tr.deterministic = False
        out["workspace_bytes_default"] = tr.workspace_bytes(a.batch)
        tr.deterministic = True
    g_ldj = torch.full((a.batch,), -1.0 / a.batch, device=dev)
    flat = torch.zeros(tr.grad_floats, device=dev)

    def library_step():
        z, ldj, trace = tr.forward(xd, nd)
        flat.zero_()
        tr.backward(trace, z * (1.0 / a.batch), g_ldj, out=flat)
    out["library"] = timed(library_step, a.steps, a.reps, a.warmup)
    print(json.dumps(out))


if __name__ == "__main__":
    main()
