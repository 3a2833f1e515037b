#!/usr/bin/env python3
"""One whole training step of one CIFAR-shaped image Glow component (3 x 32 x 32, K = 8, L = 2, h = 256, batch 256, AdamW, clip 50,
bits per dimension), plain and class-conditional, in one process:

    python tools/bench_image_ycond_step.py [--batch 256] [--steps 20] [--reps 5] [--warmup 5] [--K 8] [--hidden 256] [--classes 10]

  plain   model.training_step(x, noise=noise, ...): gbnf_image_trainer_nll_step, the step as it was before class conditioning
  ycond   the same parameters with y_condition: model.training_step(x, noise=noise, y_onehot=y, ...): gbnf_image_trainer_nll_step_y
          (the seed kernel replaced by the per-image kernel, one reduction launch more, six small regions more in the update)
Each line: median [min - max] over ``reps`` windows of ``steps`` steps, same warm-up, the discipline of tools/bench_image_train.py and
tools/bench_image_fused_step.py.  One JSON line."""
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
from gbnf_amd import BoostedFlow, image_glow, synth  # noqa: E402


def build(a, sp, dev, classes):
    args = argparse.Namespace(
        num_flows=a.K, z_size=3072, density_evaluation=True, device=dev, cuda=True, component_type="glow", num_components=1,
        rho_init="decreasing", learn_top=True, y_classes=classes, y_condition=classes > 0, sample_size=4, input_size=[3, 32, 32],
        h_size=a.hidden, num_blocks=a.L, actnorm_scale=1.0, flow_permutation="invconv", flow_coupling="affine", LU_decomposed=False,
        num_dequant_blocks=0, coupling_network="tanh", coupling_network_depth=1, batch_norm=False)
    m = BoostedFlow(args)
    image_glow.load_image_spec(m.flows[0], sp)
    m.train()
    return m


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--batch", type=int, default=256)
    ap.add_argument("--steps", type=int, default=20)
    ap.add_argument("--reps", type=int, default=5)
    ap.add_argument("--warmup", type=int, default=5)
    ap.add_argument("--K", type=int, default=8)
    ap.add_argument("--L", type=int, default=2)
    ap.add_argument("--hidden", type=int, default=256)
    ap.add_argument("--classes", type=int, default=10)
    ap.add_argument("--lr", type=float, default=1e-5)
    a = ap.parse_args()
    dev = torch.device("cuda:0")
    x, noise = synth.synth_image_batch(a.batch, seed=4)
    xd, nd = torch.from_numpy(x).to(dev), torch.from_numpy(noise).to(dev)
    y = np.zeros((a.batch, a.classes), dtype=np.float32)
    y[np.arange(a.batch), np.random.RandomState(5).randint(0, a.classes, size=a.batch)] = 1.0
    yd = torch.from_numpy(y).to(dev)
    out = {"workload": f"image step 3x32x32 K={a.K} L={a.L} h={a.hidden} batch={a.batch} AdamW clip 50 bpd, Y={a.classes}",
           "steps": a.steps, "reps": a.reps, "warmup": a.warmup}
    hyper = dict(lr=a.lr, weight_decay=1e-5, max_grad_norm=50.0)
    for name, classes in (("plain", 0), ("ycond", a.classes)):
        m = build(a, synth.synth_image_glow_spec((3, 32, 32), h=a.hidden, K=a.K, L=a.L, seed=3, y_classes=classes), dev, classes)
        last = {}
        extra = dict(y_onehot=yd) if classes else {}

        def step():
            last.update(m.training_step(xd, noise=nd, **hyper, **extra))
        out[name] = timed(step, a.steps, a.reps, a.warmup)
        out[name]["bpd"] = float(last["bpd"])
        if classes:
            out[name]["loss_classes"] = float(last["loss_classes"])
        del m
    out["ycond_over_plain"] = out["ycond"]["ms_median"] / out["plain"]["ms_median"]
    print(json.dumps(out))


if __name__ == "__main__":
    main()
