#!/usr/bin/env python3
"""One WHOLE training step of one image Glow component -- loss, backward, clip_grad_norm_(50), AdamW -- two ways, in one process:
BASELINE.json configs[3] (3 x 32 x 32, K = 8, L = 2, h = 256) at batch 64, LU-decomposed 1x1 convolutions, learned top prior, bits per
dimension.

    python tools/bench_image_fused_step.py [--batch 64] [--steps 50] [--reps 5] [--warmup 5] [--K 8] [--hidden 256] [--only fused]
                                           [--deterministic]

  module   the eager step around the library's forward / backward: model.component_forward(x, 0, noise) in train mode -> the
           reference's loss -> backward() -> clip_grad_norm_ -> torch.optim.AdamW.step()
  fused    model.training_step(x, noise=noise, lr=..., max_grad_norm=50, weight_decay=...): gbnf_image_trainer_nll_step
Each line: median [min - max] over ``reps`` windows of ``steps`` steps, same warm-up, the discipline of tools/bench_image_train.py.
Per-kernel times of the new launches: a run of its own under
`rocprofv3 --kernel-trace --stats -- python tools/bench_image_fused_step.py --only fused --reps 1`.
``--deterministic``: both lines in the image trainer's deterministic mode."""
import argparse
import json
import math
import os
import sys

import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tools"))

from bench_image_train import nll_of, timed  # noqa: E402
from gbnf_amd import BoostedFlow, image_glow, synth  # noqa: E402


def build(a, sp, dev):
    """BoostedFlow(args) with LU 1x1s holding the spec's numbers: the matrices through their LU parameterisation."""
    args = argparse.Namespace(
        num_flows=a.K, z_size=3072, density_evaluation=True, device=dev, cuda=True, component_type="glow", num_components=1,
        rho_init="decreasing", learn_top=True, y_classes=0, y_condition=False, sample_size=4, input_size=[3, 32, 32], h_size=a.hidden,
        num_blocks=a.L, actnorm_scale=1.0, flow_permutation="invconv", flow_coupling="affine", LU_decomposed=True,
        num_dequant_blocks=0, coupling_network="tanh", coupling_network_depth=1, batch_norm=False, image_deterministic=bool(a.deterministic))
    m = BoostedFlow(args)
    glow = m.flows[0]
    steps = [st for lv in sp["levels"] for st in lv["steps"]]
    splits = [lv["split"] for lv in sp["levels"] if lv["split"] is not None]
    si = pi = 0
    for layer in glow.flow.layers:
        if isinstance(layer, image_glow.FlowStep):
            st = steps[si]
            si += 1
            image_glow._put(layer.actnorm.bias, st["an_bias"])
            image_glow._put(layer.actnorm.logs, st["an_logs"])
            p, lower, upper = torch.linalg.lu(torch.from_numpy(st["perm_w"]).double())
            s = torch.diag(upper)
            inv = layer.invconv
            for dst, src in ((inv.p, p), (inv.sign_s, torch.sign(s)), (inv.lower, lower), (inv.upper, torch.triu(upper, 1)),
                             (inv.log_s, torch.log(torch.abs(s)))):
                image_glow._put(dst, src.numpy())
            for cm, c in zip([q for q in layer.block.network if not isinstance(q, torch.nn.ReLU)], st["convs"]):
                image_glow._load_conv(cm, c)
        elif isinstance(layer, image_glow.Split2d):
            image_glow._load_conv(layer.conv, splits[pi])
            pi += 1
    image_glow._load_conv(glow.learn_top_fn, sp["learn_top"])
    glow.set_actnorm_init()
    m.train()
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
    ap.add_argument("--lr", type=float, default=1e-5)
    ap.add_argument("--only", choices=("module", "fused"), default=None)
    ap.add_argument("--deterministic", action="store_true")
    a = ap.parse_args()
    dev = torch.device("cuda:0")
    sp = synth.synth_image_glow_spec((3, 32, 32), h=a.hidden, K=a.K, L=a.L, seed=3)
    x, noise = synth.synth_image_batch(a.batch, seed=4)
    xd, nd = torch.from_numpy(x).to(dev), torch.from_numpy(noise).to(dev)
    per_dim = 1.0 / (math.log(2.0) * 3072)
    out = {"workload": f"image fused step 3x32x32 K={a.K} L={a.L} h={a.hidden} batch={a.batch} LU AdamW clip 50 bpd", "steps": a.steps,
           "reps": a.reps, "warmup": a.warmup, "deterministic": bool(a.deterministic)}

    if a.only != "fused":
        m = build(a, sp, dev)
        params = list(m.flows[0].parameters())
        opt = torch.optim.AdamW(params, lr=a.lr, weight_decay=1e-5)

        def module_step():
            opt.zero_grad(set_to_none=True)
            (nll_of(*m.component_forward(xd, 0, nd)[:4]) * per_dim).backward()
            torch.nn.utils.clip_grad_norm_(params, 50.0)
            opt.step()
        out["module"] = timed(module_step, a.steps, a.reps, a.warmup)
        out["module"]["bpd"] = float(nll_of(*m.component_forward(xd, 0, nd)[:4]).detach()) * per_dim

    if a.only != "module":
        f = build(a, sp, dev)
        last = {}

        def fused_step():
            last.update(f.training_step(xd, noise=nd, lr=a.lr, weight_decay=1e-5, max_grad_norm=50.0))
        out["fused"] = timed(fused_step, a.steps, a.reps, a.warmup)
        out["fused"]["bpd"] = float(last["bpd"])
    if "module" in out and "fused" in out:
        out["module_over_fused"] = out["module"]["ms_median"] / out["fused"]["ms_median"]
    print(json.dumps(out))


if __name__ == "__main__":
    main()
