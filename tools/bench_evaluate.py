#!/usr/bin/env python3
"""Time one validation pass: ``model.evaluate(loader)`` against the eager loop a caller writes without it, on the same build.

    python tools/bench_evaluate.py [--repeats 9] [--warmup 2] [--passes 10] [--case tabular|image|both]

tabular  a MINIBOONE-shaped Boosted-Glow (C = 4, d = 43, h = 215, K = 5) at component 3, 64 batches of 512 rows.  The eager loop is
         density_experiment.py:549-588 as written: per batch ``component + 1`` module forwards with the recursion in torch, the forward
         of ``"c"``, then ``torch.cat`` and ``.mean().item()``.
image    a CIFAR-shaped Boosted-Glow (C = 4, 3x32x32, K = 8, L = 2, h = 256) at component 3, 8 batches of 64.  The eager loop is
         ``component_log_prob`` + the recursion per batch with one ``.item()`` per batch, as image_experiment.py:302-334 reads its loss.
         A third leg, ``one_call``, runs gbnf_image_mixture_evaluate per batch (the chains one after the other on one stream).

Both forms see the same device-resident batches (and, for images, the same seeded noise); they are timed alternately in windows of several passes, each pass
ending in the host read that delivers its result, with a host clock around the window.  Prints one JSON line per case: medians and ranges in
milliseconds per pass, and the two forms' results side by side.  Needs the MI355X; there is no CPU path."""
import argparse
import json
import math
import os
import statistics
import sys
import time

import numpy as np

REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
if REPO not in sys.path:
    sys.path.insert(0, REPO)


def tabular_model(dev, C_=4, d=43, h=215, K=5):
    import torch
    from gbnf_amd import BoostedFlow, synth
    args = argparse.Namespace(
        num_flows=K, z_size=d, density_evaluation=True, device=dev, cuda=True, component_type="glow", num_components=C_,
        rho_init="decreasing", learn_top=False, y_classes=0, y_condition=False, sample_size=4, input_size=[d], h_size=h, num_blocks=1,
        actnorm_scale=1.0, flow_permutation="shuffle", flow_coupling="affine", LU_decomposed=False, num_dequant_blocks=0,
        coupling_network="tanh", coupling_network_depth=1, batch_norm=True, boosted=True)
    m = BoostedFlow(args)
    for c, spec in enumerate(synth.synth_boosted_specs("glow", C_, d, h, K, seed=1)):
        m.load_spec(c, spec)
    m.component = C_ - 1
    m.eval()
    return m


def tabular_eager(m, loader):
    """density_experiment.py:549-588."""
    import torch
    G_nll, g_nll = [], []
    with torch.no_grad():
        for (x, _) in loader:
            G_ll = None
            for c in range(m.component + 1):
                z_G, _, _, ldj_G, _ = m(x=x, components=c)
                ll = torch.sum(-0.5 * math.log(2 * math.pi) - 0.5 * z_G.pow(2), dim=-1) + ldj_G
                if c == 0:
                    G_ll = ll
                else:
                    rho_simplex = m.rho[0:(c + 1)] / torch.sum(m.rho[0:(c + 1)])
                    last_ll = torch.log(1 - rho_simplex[c]) + G_ll
                    next_ll = torch.log(rho_simplex[c]) + ll
                    G_ll = torch.logsumexp(torch.cat([last_ll.view(-1, 1), next_ll.view(-1, 1)], dim=1), dim=1)
            G_nll.append(-1.0 * G_ll.detach())
            z_g, _, _, ldj_g, _ = m(x=x, components="c")
            g_nll.append(-1.0 * (torch.sum(-0.5 * math.log(2 * math.pi) - 0.5 * z_g.pow(2), dim=-1) + ldj_g).detach())
        G_nll, g_nll = torch.cat(G_nll, dim=0), torch.cat(g_nll, dim=0)
        return {"nll": G_nll.mean().item(), "g_nll": g_nll.mean().item(), "ratio": torch.mean(g_nll - G_nll).item()}


def image_model(dev, C_=4, size=(3, 32, 32), h=256, K=8, L=2):
    import torch
    from gbnf_amd import BoostedFlow, image_glow, synth
    args = argparse.Namespace(
        num_flows=K, z_size=int(np.prod(size)), density_evaluation=True, device=dev, cuda=True, component_type="glow", num_components=C_,
        rho_init="decreasing", learn_top=True, y_classes=0, y_condition=False, sample_size=4, input_size=list(size), h_size=h,
        num_blocks=L, actnorm_scale=1.0, flow_permutation="invconv", flow_coupling="affine", LU_decomposed=False, num_dequant_blocks=0,
        coupling_network="tanh", coupling_network_depth=1, batch_norm=False, boosted=True)
    torch.manual_seed(0)
    m = BoostedFlow(args)
    for c in range(C_):
        image_glow.load_image_spec(m.flows[c], synth.synth_image_glow_spec(size, h=h, K=K, L=L, seed=1 + c))
    m.component = C_ - 1
    m.eval()
    return m


def image_eager(m, loader, generator):
    """component_log_prob + the recursion per batch, the loss read back per batch (image_experiment.py:302-336)."""
    import torch
    from gbnf_amd import native
    per_dim = 1.0 / (math.log(2.0) * float(np.prod(m.args.input_size)))
    loss, n_used = 0.0, m.component + 1
    with torch.no_grad():
        for (x, _) in loader:
            noise = torch.rand(x.shape, generator=generator, device=x.device)
            ll = m.component_log_prob(x, n_used, noise)
            G = native.mixture_lse(ll.t().contiguous(), m.rho)
            loss += (-G.mean() * per_dim).item()
    return {"bpd_batch_mean": loss / len(loader)}


def timed(fn, passes):
    """Milliseconds per pass over a window of ``passes`` passes (each ends in the host read of its result), and the last result."""
    import torch
    torch.cuda.synchronize()
    t0 = time.perf_counter()
    for _ in range(passes):
        out = fn()
    torch.cuda.synchronize()
    return (time.perf_counter() - t0) * 1e3 / passes, out


def image_one_call(m, loader, generator):
    """The same pass with gbnf_image_mixture_evaluate per batch: the components' chains one after the other on one stream."""
    import torch
    from gbnf_amd import native
    n_used, state = m.component + 1, None
    with torch.no_grad():
        for (x, _) in loader:
            noise = torch.rand(x.shape, generator=generator, device=x.device)
            state = native.eval_state(x.device) if state is None else state
            native.NativeImageFlow.evaluate([m.native_flow(k) for k in range(n_used)], x, noise, m.component, m.rho, state)
    s = state.tolist()
    return {"bpd": -s[2] / s[0] / (math.log(2.0) * float(np.prod(m.args.input_size)))}


def compare(name, module_fn, eager_fn, warmup, repeats, passes, extra, one_call_fn=None):
    fns = {"evaluate": module_fn, "eager": eager_fn}
    if one_call_fn is not None:
        fns["one_call"] = one_call_fn
    for _ in range(warmup):
        for fn in fns.values():
            fn()
    times, outs = {k: [] for k in fns}, {}
    for _ in range(repeats):        # alternating: the machine's drift hits all forms alike
        for k, fn in fns.items():
            t, outs[k] = timed(fn, passes)
            times[k].append(t)
    res = {"case": name, "repeats": repeats, "warmup": warmup, "passes_per_window": passes}
    for k, t in times.items():
        res[k + "_ms"] = {"median": statistics.median(t), "min": min(t), "max": max(t)}
    res["eager_over_evaluate"] = statistics.median(times["eager"]) / statistics.median(times["evaluate"])
    res.update(outs)
    res.update(extra)
    print(json.dumps(res), flush=True)
    return res


def main(argv=None):
    ap = argparse.ArgumentParser()
    ap.add_argument("--repeats", type=int, default=9)
    ap.add_argument("--warmup", type=int, default=2)
    ap.add_argument("--passes", type=int, default=10, help="passes per timed window (tabular; the image case takes half as many)")
    ap.add_argument("--case", choices=("tabular", "image", "both"), default="both")
    a = ap.parse_args(argv)
    import torch
    from gbnf_amd import synth
    if not torch.cuda.is_available():
        raise SystemExit("bench_evaluate.py needs the MI355X: there is no CPU path")
    dev = torch.device("cuda:0")
    torch.cuda.set_device(dev)
    if a.case in ("tabular", "both"):
        m = tabular_model(dev)
        loader = [(torch.from_numpy(synth.synth_batch(512, 43, seed=100 + b)).to(dev), None) for b in range(64)]
        compare("tabular", lambda: m.evaluate(loader), lambda: tabular_eager(m, loader), a.warmup, a.repeats, a.passes,
                {"shape": "Boosted-Glow C=4 d=43 h=215 K=5, component 3", "batches": 64, "rows_per_batch": 512})
    if a.case in ("image", "both"):
        m = image_model(dev)
        loader = [(torch.from_numpy(synth.synth_image_batch(64, (3, 32, 32), seed=100 + b)[0]).to(dev), None) for b in range(8)]
        gen = lambda: torch.Generator(device=dev).manual_seed(7)
        compare("image", lambda: m.evaluate(loader, noise_generator=gen()), lambda: image_eager(m, loader, gen()), a.warmup, a.repeats,
                max(1, a.passes // 2), {"shape": "Boosted-Glow C=4 3x32x32 K=8 L=2 h=256, component 3", "batches": 8, "rows_per_batch": 64},
                one_call_fn=lambda: image_one_call(m, loader, gen()))
    return 0


if __name__ == "__main__":
    sys.exit(main())
