#!/usr/bin/env python3
"""The score grad_x log p(x) of the tabular path: MINIBOONE-shaped Glow (d = 43, h = 215, K = 5), C = 4, at N = 512 and N = 65536.

    python tools/bench_score.py [--batches 512,65536] [--components 4] [--steps 10] [--events 16] [--warmup 5]

Per batch, the median / min / max over ``events`` device-event windows of ``steps`` calls each, same build, same process, same warm-up:
  (a) score         BoostedFlow.score(x): the evaluation path's table (one launch), then ONE gbnf_mixture_score call
  (a') no table     native.mixture_score on the same trainers without a table: a second (traced) forward per component instead
                    of the evaluation pass
  (b) composition   what a user had before: C calls of component_forward(x.requires_grad_(), c, differentiable=True), the base
                    log-density and logsumexp in torch, autograd.grad -- C full backwards whose weight gradients are thrown away.
                    It uses nothing this tool's commit added, so it runs unchanged on the commit before
  (b') frozen       the same composition with every parameter's requires_grad off: the recorded backward then takes
                    gbnf_trainer_backward_x (before that short-cut existed: the same as (b))
  (c) log_prob      BoostedFlow.log_prob(x) alone: the floor
and max |score - composition| / max |composition| on the timed inputs.
"""
import argparse
import json
import math
import os
import statistics
import sys

import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

from gbnf_amd import BoostedFlow, native, synth  # noqa: E402


def timed(fn, steps, events, warmup):
    for _ in range(warmup):
        fn()
    out = []
    for _ in range(events):
        t0, t1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        t0.record()
        for _ in range(steps):
            fn()
        t1.record()
        t1.synchronize()
        out.append(t0.elapsed_time(t1) / steps)
    return {"ms_median": statistics.median(out), "ms_min": min(out), "ms_max": max(out)}


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--batches", default="512,65536")
    ap.add_argument("--components", type=int, default=4)
    ap.add_argument("--steps", type=int, default=10)
    ap.add_argument("--events", type=int, default=16)
    ap.add_argument("--warmup", type=int, default=5)
    ap.add_argument("--d", type=int, default=43)
    ap.add_argument("--hidden", type=int, default=215)
    ap.add_argument("--K", type=int, default=5)
    a = ap.parse_args()
    if not torch.cuda.is_available():
        sys.exit("bench_score.py measures on the MI355X: no device visible")
    dev = torch.device("cuda:0")
    C, d = a.components, a.d
    args = argparse.Namespace(
        num_flows=a.K, z_size=d, density_evaluation=True, device=dev, cuda=True, component_type="glow", num_components=C,
        rho_init="decreasing", learn_top=False, y_classes=0, y_condition=False, sample_size=4, input_size=[d], h_size=a.hidden,
        num_blocks=1, actnorm_scale=1.0, flow_permutation="shuffle", flow_coupling="affine", LU_decomposed=False,
        num_dequant_blocks=0, coupling_network="tanh", coupling_network_depth=1, batch_norm=False)
    m = BoostedFlow(args)
    for c, sp in enumerate(synth.synth_boosted_specs("glow", C, d, a.hidden, a.K, seed=1)):
        m.load_spec(c, sp)
    m.all_trained = True
    m.eval()
    rho = m.rho.detach().float()
    log_w = torch.log(rho / rho.sum()).view(-1, 1).contiguous()
    out = {"workload": f"tabular score glow d={d} h={a.hidden} K={a.K} C={C}", "steps": a.steps, "events": a.events, "warmup": a.warmup,
           "batches": {}}
    for batch in (int(b) for b in a.batches.split(",")):
        xd = torch.from_numpy(synth.synth_batch(batch, d, seed=0)).to(dev)

        def composition():
            xl = xd.clone().requires_grad_(True)
            ll = []
            for c in range(C):
                z, ldj = m.component_forward(xl, c, differentiable=True)
                ll.append(torch.sum(-0.5 * math.log(2 * math.pi) - 0.5 * z * z, dim=1) + ldj)
            G = torch.logsumexp(torch.stack(ll) + log_w, dim=0)
            return torch.autograd.grad(G.sum(), xl)[0]

        trainers, log_w_flat = [m.native_trainer(c) for c in range(C)], log_w.view(-1)

        def no_table():
            return native.mixture_score(trainers, log_w_flat, xd)[0]

        res = {"a_score": timed(lambda: m.score(xd), a.steps, a.events, a.warmup),
               "a_no_table": timed(no_table, a.steps, a.events, a.warmup),
               "b_composition": timed(composition, a.steps, a.events, a.warmup),
               "c_log_prob": timed(lambda: m.log_prob(xd), a.steps, a.events, a.warmup)}
        for p in m.parameters():          # (b'): frozen outside the timed windows
            p.requires_grad_(False)
        try:
            res["b_frozen_composition"] = timed(composition, a.steps, a.events, a.warmup)
        finally:
            for p in m.parameters():
                p.requires_grad_(True)
        res["composition_over_score"] = res["b_composition"]["ms_median"] / res["a_score"]["ms_median"]
        res["score_over_log_prob"] = res["a_score"]["ms_median"] / res["c_log_prob"]["ms_median"]
        ref, got = composition(), m.score(xd)
        res["max_abs_diff_vs_composition_over_max"] = float((ref - got).abs().max() / ref.abs().max())
        out["batches"][str(batch)] = res
    print(json.dumps(out))


if __name__ == "__main__":
    main()
