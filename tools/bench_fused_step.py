#!/usr/bin/env python3
"""One boosted training step of density_experiment.py:340-384 three ways, in the same process on the same model (MINIBOONE Glow, the model,
batch sizes and warm-up of tools/bench_boosted_step.py):

  (a) module   the drop-in module as the reference's loop drives it: boosting_weights, torch.multinomial, the row gather, the recorded
               forward, the NLL in torch ops, loss.backward(), clip_grad_norm_, torch.optim.AdamW
  (b) fused    BoostedFlow.training_step: boosting_weights + torch.multinomial, then ONE library call (gather, forward, loss seed,
               backward, gradient norm, clip, AdamW on the live tensors: gbnf_trainer_nll_step)
  (c) onecall  BoostedFlow.training_step(uniforms=True): torch.rand, then ONE library call for all of it (mixture log-density, weights,
               inverse-CDF resample, and the step of (b): gbnf_boosted_nll_step)

Wall time per step (host clock around a window that ends in a synchronise) and GPU time between two events around the same window,
in alternating rounds of the paths; one JSON line.

    python tools/bench_fused_step.py [--batch 512] [--steps 200] [--rounds 5] [--components 4]
"""
import argparse, json, math, os, statistics, sys, time
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT); sys.path.insert(0, os.path.join(ROOT, "tests"))
import torch
from gbnf_amd import BoostedFlow
from test_hip_train import _args

LR, WEIGHT_DECAY, MAX_GRAD_NORM = 1e-3, 1e-5, 10.0       # the reference's MINIBOONE settings, density_experiment.py:183-185


def lns(z):
    return torch.sum(-0.5 * math.log(2 * math.pi) - 0.5 * z.pow(2), dim=-1)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--batch", type=int, default=512)
    ap.add_argument("--steps", type=int, default=200)
    ap.add_argument("--rounds", type=int, default=5)
    ap.add_argument("--components", type=int, default=4)
    ap.add_argument("--deterministic", action="store_true", help="time the same step in deterministic mode (ordered weight-gradient flush)")
    a = ap.parse_args()
    dev = torch.device("cuda:0")
    torch.manual_seed(0)
    d, h, K, C = 43, 215, 5, a.components
    margs = _args("glow", d, h, K, C, dev)
    margs.deterministic = a.deterministic
    m = BoostedFlow(margs).to(dev)
    x = torch.randn(a.batch, d, device=dev)
    m.train()
    with torch.no_grad():
        for c in range(C):                       # ActNorm data-dependent init of every component
            m.component = c
            m(x=x, components="c")
    m.component = C - 1                          # train the last component against the C-1 fixed ones
    params = list(m.flows[C - 1].parameters())
    opt = torch.optim.AdamW(params, lr=LR, weight_decay=WEIGHT_DECAY)
    for name, p_ in m.named_parameters():        # init_boosted_lr, density_experiment.py:537-538
        p_.requires_grad = name.startswith(f"flows.{m.component}")

    def module_step():
        opt.zero_grad(set_to_none=False)
        with torch.no_grad():
            w, _ = m.boosting_weights(x)                                    # :624-640
        xr = x[torch.multinomial(w, x.size(0), replacement=True)]           # :642-644
        z, _, _, ldj, _ = m(x=xr, components="c")
        loss = torch.mean(-(lns(z) + ldj))
        loss.backward()
        torch.nn.utils.clip_grad_norm_(params, MAX_GRAD_NORM)               # :363-364
        opt.step()

    def fused_step():
        m.training_step(x, lr=LR, weight_decay=WEIGHT_DECAY, max_grad_norm=MAX_GRAD_NORM)

    def window(fn):
        """-> (wall ms per step, GPU ms per step between events) of one window of a.steps steps"""
        ev = [torch.cuda.Event(enable_timing=True) for _ in range(2)]
        torch.cuda.synchronize()
        t0 = time.perf_counter()
        ev[0].record()
        for _ in range(a.steps):
            fn()
        ev[1].record()
        torch.cuda.synchronize()
        return (time.perf_counter() - t0) / a.steps * 1e3, ev[0].elapsed_time(ev[1]) / a.steps

    def onecall_step():
        m.training_step(x, lr=LR, weight_decay=WEIGHT_DECAY, max_grad_norm=MAX_GRAD_NORM, uniforms=True)

    paths = {"module": module_step, "fused": fused_step, "onecall": onecall_step}
    for fn in paths.values():
        for _ in range(20):
            fn()
    res = {k: [] for k in paths}
    for _ in range(a.rounds):                    # alternating: a drift of the machine hits both paths alike
        for k, fn in paths.items():
            res[k].append(window(fn))
    out = {"metric": "boosted training step, MINIBOONE Glow: module path (clip_grad_norm_ + torch.optim.AdamW) vs BoostedFlow.training_step "
                     "(value) vs training_step(uniforms=True), the one-call boosted step",
           "unit": "ms/step", "batch": a.batch, "components": C, "steps_per_window": a.steps, "rounds": a.rounds,
           "data": "synthetic", "dtype": "f16x3", "lr": LR, "weight_decay": WEIGHT_DECAY, "max_grad_norm": MAX_GRAD_NORM}
    for k, r in res.items():
        wall, gpu = [w for w, _ in r], [g for _, g in r]
        out[f"{k}_ms_per_step_wall"] = statistics.median(wall)
        out[f"{k}_ms_per_step_wall_min_max"] = [min(wall), max(wall)]
        out[f"{k}_ms_per_step_gpu_events"] = statistics.median(gpu)
    out["value"] = out["fused_ms_per_step_wall"]
    out["speedup_wall"] = out["module_ms_per_step_wall"] / out["fused_ms_per_step_wall"]
    out["onecall_speedup_wall_vs_fused"] = out["fused_ms_per_step_wall"] / out["onecall_ms_per_step_wall"]
    out["note"] = ("wall: host clock around a window that ends in a synchronise, median over alternating rounds; gpu_events: device time "
                   "between two events around the same window (host gaps included while the stream runs dry)")
    print(json.dumps(out))


if __name__ == "__main__":
    main()
