#!/usr/bin/env python3
"""The joint likelihood step of the whole mixture: MINIBOONE-shaped Glow (d = 43, h = 215, K = 5), C = 4, at n = 512 and n = 65536.

    python tools/bench_mixture_step.py [--batches 512,65536] [--components 4] [--reps 20] [--warmup 5]

Three legs, alternated within one process (a, b, c, a, b, c, ...), every repetition between two device synchronisations and timed on
the host clock (the legs differ in host work, which is what is being compared); median and minimum per leg:
  (a) mixture_training_step   BoostedFlow.mixture_training_step(x): ONE gbnf_mixture_nll_step call
  (b) eager composition       what a user had before: C calls of component_forward(x, c, differentiable=True), the base log-density
                              and logsumexp in torch, backward, clip_grad_norm_ over all parameters, one torch.optim.AdamW over them
  (c) C nll_step calls        the floor: the same flow work (C traced forwards, C backwards, C updates) without the coupling -- every
                              component on its own NLL, its own clip
All three move the parameters (lr = 1e-5: they stay where the timing started, near enough).
"""
import argparse
import json
import math
import os
import statistics
import sys
import time

import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

from gbnf_amd import BoostedFlow, native, synth  # noqa: E402


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--batches", default="512,65536")
    ap.add_argument("--components", type=int, default=4)
    ap.add_argument("--reps", type=int, default=20)
    ap.add_argument("--warmup", type=int, default=5)
    ap.add_argument("--d", type=int, default=43)
    ap.add_argument("--hidden", type=int, default=215)
    ap.add_argument("--K", type=int, default=5)
    a = ap.parse_args()
    if a.reps < 20:
        sys.exit("bench_mixture_step.py: at least 20 repetitions")
    if not torch.cuda.is_available():
        sys.exit("bench_mixture_step.py measures on the MI355X: no device visible")
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
    lr, clip = 1e-5, 5.0
    params = [p for c in range(C) for p in m.flows[c].parameters()]
    adamw = torch.optim.AdamW(params, lr=lr, weight_decay=0.0)
    trainers = [m.native_trainer(c) for c in range(C)]
    floor_states = [native.OptState(t, "adamw") for t in trainers]
    out = {"workload": f"mixture step glow d={d} h={a.hidden} K={a.K} C={C}", "reps": a.reps, "warmup": a.warmup, "batches": {}}
    for batch in (int(b) for b in a.batches.split(",")):
        xd = torch.from_numpy(synth.synth_batch(batch, d, seed=0)).to(dev)

        def fused():
            return m.mixture_training_step(xd, lr=lr, max_grad_norm=clip)["nll"]

        def eager():
            rho = m.rho[:C].detach().float()
            log_w = torch.log(rho / rho.sum()).view(-1, 1)
            adamw.zero_grad(set_to_none=True)
            ll = []
            for c in range(C):
                z, ldj = m.component_forward(xd, c, differentiable=True)
                ll.append(torch.sum(-0.5 * math.log(2 * math.pi) - 0.5 * z * z, dim=1) + ldj)
            nll = -torch.logsumexp(torch.stack(ll) + log_w, dim=0).mean()
            nll.backward()
            torch.nn.utils.clip_grad_norm_(params, clip)
            adamw.step()
            return nll

        def floor():
            return [t.nll_step(xd, s, lr=lr, max_grad_norm=clip)[0] for t, s in zip(trainers, floor_states)]

        legs = {"a_mixture_training_step": fused, "b_eager_composition": eager, "c_nll_steps": floor}
        nll_fused, nll_eager = float(fused()), float(eager().detach())
        times = {k: [] for k in legs}
        for it in range(a.warmup + a.reps):
            for k, fn in legs.items():
                torch.cuda.synchronize()
                t0 = time.perf_counter()
                fn()
                torch.cuda.synchronize()
                if it >= a.warmup:
                    times[k].append((time.perf_counter() - t0) * 1e3)
        res = {k: {"ms_median": statistics.median(v), "ms_min": min(v)} for k, v in times.items()}
        res["eager_over_fused"] = res["b_eager_composition"]["ms_median"] / res["a_mixture_training_step"]["ms_median"]
        res["fused_over_floor"] = res["a_mixture_training_step"]["ms_median"] / res["c_nll_steps"]["ms_median"]
        res["nll_fused_then_eager"] = [nll_fused, nll_eager]
        out["batches"][str(batch)] = res
    print(json.dumps(out))


if __name__ == "__main__":
    main()
