#!/usr/bin/env python3
"""The log-density of a batch under EVERY class of a class-conditional CIFAR-shaped image Glow component (3 x 32 x 32, K = 8, L = 2,
h = 256, batch 256), two ways, in one process:

    python tools/bench_image_class_table.py [--batch 256] [--steps 10] [--reps 5] [--warmup 3] [--K 8] [--hidden 256] [--classes 10 100]

  forward_y  Y calls of handle.forward(x, noise, y=e_k): gbnf_image_flow_forward_y once per class, what the table cost before -- the baseline
  classes    one handle.forward_classes(x, noise): gbnf_image_flow_forward_classes, one flow pass and one small launch
per class count, and the two tables' largest relative difference.  Then ``marginal_log_prob`` (label-free log p(x): C forward_classes,
the recursion over rho, Bayes' rule) of a C = 4 model beside ``log_prob(x, y_onehot=y)`` of the same model (C forward_y).
Each line: median [min - max] over ``reps`` windows of ``steps`` calls, same warm-up, the discipline of tools/bench_image_train.py.
One JSON line."""
import argparse
import json
import os
import sys

import numpy as np
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tools"))

from bench_image_train import timed  # noqa: E402
from gbnf_amd import BoostedFlow, image_glow, native, synth  # noqa: E402


def build(a, dev, classes, components):
    args = argparse.Namespace(
        num_flows=a.K, z_size=3072, density_evaluation=True, device=dev, cuda=True, component_type="glow", num_components=components,
        rho_init="decreasing", learn_top=True, y_classes=classes, y_condition=True, sample_size=4, input_size=[3, 32, 32],
        h_size=a.hidden, num_blocks=a.L, actnorm_scale=1.0, flow_permutation="invconv", flow_coupling="affine", LU_decomposed=False,
        num_dequant_blocks=0, coupling_network="tanh", coupling_network_depth=1, batch_norm=False)
    m = BoostedFlow(args)
    for c in range(components):
        image_glow.load_image_spec(m.flows[c], synth.synth_image_glow_spec((3, 32, 32), h=a.hidden, K=a.K, L=a.L, seed=3 + c, y_classes=classes))
    m.eval()
    return m


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--batch", type=int, default=256)
    ap.add_argument("--steps", type=int, default=10)
    ap.add_argument("--reps", type=int, default=5)
    ap.add_argument("--warmup", type=int, default=3)
    ap.add_argument("--K", type=int, default=8)
    ap.add_argument("--L", type=int, default=2)
    ap.add_argument("--hidden", type=int, default=256)
    ap.add_argument("--classes", type=int, nargs="+", default=[10, 100])
    ap.add_argument("--components", type=int, default=4)
    a = ap.parse_args()
    dev = torch.device("cuda:0")
    x, noise = synth.synth_image_batch(a.batch, seed=4)
    xd, nd = torch.from_numpy(x).to(dev), torch.from_numpy(noise).to(dev)
    out = {"workload": f"class table 3x32x32 K={a.K} L={a.L} h={a.hidden} batch={a.batch}", "steps": a.steps, "reps": a.reps, "warmup": a.warmup}
    for Y in a.classes:
        flow = native.NativeImageFlow(synth.synth_image_glow_spec((3, 32, 32), h=a.hidden, K=a.K, L=a.L, seed=3, y_classes=Y))
        ys = [torch.zeros((a.batch, Y), device=dev) for _ in range(Y)]
        for k, y in enumerate(ys):
            y[:, k] = 1.0
        last = {}

        def per_class():
            last["y"] = torch.stack([flow.forward(xd, nd, want_z=False, y=y, want_logits=False)[2] for y in ys], dim=1)

        def classes():
            last["t"] = flow.forward_classes(xd, nd)[2]
        row = {"forward_y": timed(per_class, a.steps, a.reps, a.warmup), "classes": timed(classes, a.steps, a.reps, a.warmup)}
        row["speedup"] = row["forward_y"]["ms_median"] / row["classes"]["ms_median"]
        row["max_rel_diff"] = float(((last["t"].double() - last["y"].double()).abs() / last["y"].double().abs()).max())
        out[f"Y={Y}"] = row
        del flow
    Y = a.classes[0]
    m = build(a, dev, Y, a.components)
    y = np.zeros((a.batch, Y), dtype=np.float32)
    y[np.arange(a.batch), np.random.RandomState(5).randint(0, Y, size=a.batch)] = 1.0
    yd = torch.from_numpy(y).to(dev)
    out[f"marginal_log_prob C={a.components} Y={Y}"] = timed(lambda: m.marginal_log_prob(xd, noise=nd), a.steps, a.reps, a.warmup)
    out[f"log_prob(y) C={a.components} Y={Y}"] = timed(lambda: m.log_prob(xd, noise=nd, y_onehot=yd), a.steps, a.reps, a.warmup)
    print(json.dumps(out))


if __name__ == "__main__":
    main()
