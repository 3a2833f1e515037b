#!/usr/bin/env python3
"""One iteration of ``update_rho`` for a boosted image model, two ways: BASELINE.json configs[3]'s geometry (3 x 32 x 32, K = 8, L = 2,
h = 256), C = 4 components, the weight of component 3, batch 64 and 256.

    python tools/bench_image_rho.py [--batch 64] [--steps 50] [--reps 5] [--warmup 5] [--order composed,call,call_read]

  composed   the iteration built from the module's public evaluation calls: model.component_log_prob(x, 4, noise) (the component chains
             overlap on side streams), the reference's recursion in torch, the mean, one .item(), the clamped update on the host
  call       the body of BoostedImageFlow.update_rho up to min_iters: one gbnf_image_mixture_rho_step (the chains one after another on
             one stream), nothing read back
  call_read  the same followed by the read of the 4 statistics, as update_rho does after min_iters
``composed`` is the yardstick: the library call is measured against it, never against itself.  Each line: median [min - max] over
``reps`` windows of ``steps`` iterations, same warm-up, the discipline of tools/bench_image_fused_step.py; one process prints one JSON
line and runs the modes in ``--order`` (run it in both orders: the first mode of a process also pays the allocator's warm-up)."""
import argparse
import json
import os
import sys

import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tools"))

from bench_image_train import timed  # noqa: E402
from gbnf_amd import BoostedFlow, image_glow, native, synth  # noqa: E402

MODES = ("composed", "call", "call_read")


def build(a, dev):
    args = argparse.Namespace(
        num_flows=a.K, z_size=3072, density_evaluation=True, device=dev, cuda=True, component_type="glow", num_components=a.C,
        rho_init="decreasing", learn_top=True, y_classes=0, y_condition=False, sample_size=4, input_size=[3, 32, 32], h_size=a.hidden,
        num_blocks=a.L, actnorm_scale=1.0, flow_permutation="invconv", flow_coupling="affine", LU_decomposed=False,
        num_dequant_blocks=0, coupling_network="tanh", coupling_network_depth=1, batch_norm=False, rho_iters=100, rho_lr=0.005)
    m = BoostedFlow(args)
    for c in range(a.C):
        image_glow.load_image_spec(m.flows[c], synth.synth_image_glow_spec((3, 32, 32), h=a.hidden, K=a.K, L=a.L, seed=3 + c))
    m.component = a.C - 1
    m.eval()
    return m


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--batch", type=int, default=64)
    ap.add_argument("--steps", type=int, default=50)
    ap.add_argument("--reps", type=int, default=5)
    ap.add_argument("--warmup", type=int, default=5)
    ap.add_argument("--K", type=int, default=8)
    ap.add_argument("--L", type=int, default=2)
    ap.add_argument("--hidden", type=int, default=256)
    ap.add_argument("--C", type=int, default=4)
    ap.add_argument("--order", default=",".join(MODES))
    a = ap.parse_args()
    order = [s for s in a.order.split(",") if s]
    if not order or any(s not in MODES for s in order):
        ap.error(f"--order takes a comma-separated list of {MODES}")
    dev = torch.device("cuda:0")
    m = build(a, dev)
    c = m.component
    x, noise = synth.synth_image_batch(a.batch, seed=4)
    xd, nd = torch.from_numpy(x).to(dev), torch.from_numpy(noise).to(dev)
    step_size = 1e-7          # (rho stays where it is: every iteration does the same work)
    out = {"workload": f"image update_rho iteration 3x32x32 K={a.K} L={a.L} h={a.hidden} C={a.C} component={c} batch={a.batch}",
           "steps": a.steps, "reps": a.reps, "warmup": a.warmup, "order": order}
    last = {}

    @torch.no_grad()
    def composed():
        ll = m.component_log_prob(xd, c + 1, nd)
        full = ll[:, 0]
        for k in range(1, c):
            full = torch.logsumexp(torch.stack([torch.log(1 - m.rho[k]) + full, torch.log(m.rho[k]) + ll[:, k]], dim=1), dim=1)
        grad = torch.mean(full - ll[:, c]).item()
        prev = last.get("rho", 0.125)
        last["rho"] = min(max(prev - step_size * grad, 0.01), 100.0)
        m.rho[c] = last["rho"]
        last["grad_composed"] = grad

    @torch.no_grad()
    def call():
        stats = native.NativeImageFlow.rho_step([m.native_flow(k) for k in range(c + 1)], xd, nd, c, m.rho, step_size)
        torch.autograd.graph.increment_version([m.rho])
        return stats

    def call_read():
        last["grad_call"] = call().tolist()[0]

    fns = {"composed": composed, "call": call, "call_read": call_read}
    for mode in order:
        out[mode] = timed(fns[mode], a.steps, a.reps, a.warmup)
    for key in ("grad_composed", "grad_call"):
        if key in last:
            out[key] = last[key]
    if "composed" in out and "call" in out:
        out["composed_over_call"] = out["composed"]["ms_median"] / out["call"]["ms_median"]
    print(json.dumps(out))


if __name__ == "__main__":
    main()
