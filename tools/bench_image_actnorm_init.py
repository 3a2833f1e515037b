#!/usr/bin/env python3
"""The data-dependent ActNorm2d initialisation of one freshly constructed image Glow component, two ways, in one process:

    python tools/bench_image_actnorm_init.py [--batch 64] [--reps 5] [--K 8] [--L 2] [--hidden 256]

  default  BoostedImageFlow.initialize_actnorms(x, noise=noise): layer by layer -- per layer the parameters to the host, a new
           exact-f32 evaluation handle, the component up to that layer (gbnf_image_flow_actnorm_stats), bias / logs in eager torch
  fused    initialize_actnorms(x, noise=noise, fused=True): one gbnf_image_trainer_actnorm_init call on the component's trainer
           (its creation included: the model is fresh)
at the BASELINE CIFAR shape (3 x 32 x 32, K = 8, L = 2, h = 256, LU 1x1s, batch 64) and at 1 x 28 x 28 with the same model.  Every run
builds a new model (not timed); the time is that of the call, device-synchronised on both sides.  One untimed run of each path comes
first (library and code-object loading).  One JSON line: per configuration the median [min, max] of ``reps`` runs of each path in ms
and default / fused."""
import argparse
import json
import os
import statistics
import sys
import time

import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

from gbnf_amd import BoostedFlow, synth  # noqa: E402


def fresh(a, size, dev):
    args = argparse.Namespace(
        num_flows=a.K, z_size=size[0] * size[1] * size[2], density_evaluation=True, device=dev, cuda=True, component_type="glow",
        num_components=1, rho_init="decreasing", learn_top=True, y_classes=0, y_condition=False, sample_size=4, input_size=list(size),
        h_size=a.hidden, num_blocks=a.L, actnorm_scale=1.0, flow_permutation="invconv", flow_coupling="affine", LU_decomposed=True,
        num_dequant_blocks=0, coupling_network="tanh", coupling_network_depth=1, batch_norm=False)
    return BoostedFlow(args)


def one_run(a, size, dev, xd, nd, fused):
    torch.manual_seed(0)
    m = fresh(a, size, dev)
    torch.cuda.synchronize()
    t0 = time.perf_counter()
    m.initialize_actnorms(xd, noise=nd, fused=fused)
    torch.cuda.synchronize()
    ms = (time.perf_counter() - t0) * 1e3
    assert all(t.inited for t in m.flows[0]._actnorms())
    return ms, m


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--batch", type=int, default=64)
    ap.add_argument("--reps", type=int, default=5)
    ap.add_argument("--K", type=int, default=8)
    ap.add_argument("--L", type=int, default=2)
    ap.add_argument("--hidden", type=int, default=256)
    a = ap.parse_args()
    dev = torch.device("cuda:0")
    out = {"workload": f"image ActNorm2d data init K={a.K} L={a.L} h={a.hidden} batch={a.batch} LU, fresh model per run", "reps": a.reps,
           "configs": {}}
    for size in ((3, 32, 32), (1, 28, 28)):
        x, noise = synth.synth_image_batch(a.batch, size, seed=4)
        xd, nd = torch.from_numpy(x).to(dev), torch.from_numpy(noise).to(dev)
        res = {}
        last = {}
        for name, fused in (("default", False), ("fused", True)):
            one_run(a, size, dev, xd, nd, fused)
            ms = []
            for _ in range(a.reps):
                t, last[name] = one_run(a, size, dev, xd, nd, fused)
                ms.append(t)
            res[name] = {"ms_median": statistics.median(ms), "ms_min": min(ms), "ms_max": max(ms)}
        res["default_over_fused"] = res["default"]["ms_median"] / res["fused"]["ms_median"]
        res["layers"] = len(last["fused"].flows[0]._actnorms())
        res["max_abs_difference"] = max(
            float((p.logs.detach() - q.logs.detach()).abs().max()) for p, q in zip(last["default"].flows[0]._actnorms(), last["fused"].flows[0]._actnorms()))
        out["configs"]["x".join(str(v) for v in size)] = res
    print(json.dumps(out))


if __name__ == "__main__":
    main()
