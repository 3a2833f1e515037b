#!/usr/bin/env python3
"""Time fitting all mixture weights: ``model.fit_weights(loader)`` against the two ways to set weights without it, on the same build.

    python tools/bench_fit_weights.py [--repeats 9] [--warmup 2] [--passes 3] [--max-iters 1000] [--tol 1e-9]

A MINIBOONE-shaped Boosted-Glow (C = 8, d = 43, h = 215, K = 5), 64 device-resident batches of 512 rows.  Legs, timed alternately in
windows of several passes, each pass ending in the host read that delivers its result, with a host clock around the window:

  fit_weights   ``model.fit_weights(loader)``: the table fill (one flow launch per batch), ONE gbnf_weights_em call, gbnf_weights_to_rho,
                one host read
  fill          the table fill alone (the same launches, then a synchronise)
  em            gbnf_weights_em alone on the filled table, and the host read of its state
  update_rho    ``model.update_rho(loader, fused=True)`` at ``rho_iters = 100`` with the model at its last component: every iteration
                re-runs all component forwards on a batch and moves rho[7] alone; 4 floats read back per iteration after the tenth
  eager_em      EM in eager torch on the same filled table (float64): ``torch.logsumexp``, a softmax mean, one ``.item()`` per iteration,
                the same stopping rule

rho is put back to its start before every pass, so every pass does the same work.  Prints one JSON line: medians and ranges in
milliseconds per pass, and what each leg arrived at.  Needs the MI355X; there is no CPU path."""
import argparse
import json
import os
import statistics
import sys
import time

REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
if REPO not in sys.path:
    sys.path.insert(0, REPO)


class Loader:
    """Device-resident batches with a ``dataset`` whose length sizes the table, as a torch DataLoader has."""

    def __init__(self, batches):
        self.batches = batches
        self.dataset = range(sum(int(x.shape[0]) for x, _ in batches))

    def __iter__(self):
        return iter(self.batches)

    def __len__(self):
        return len(self.batches)


def model(dev, C_=8, d=43, h=215, K=5):
    from gbnf_amd import BoostedFlow, synth
    args = argparse.Namespace(
        num_flows=K, z_size=d, density_evaluation=True, device=dev, cuda=True, component_type="glow", num_components=C_,
        rho_init="decreasing", learn_top=False, y_classes=0, y_condition=False, sample_size=4, input_size=[d], h_size=h, num_blocks=1,
        actnorm_scale=1.0, flow_permutation="shuffle", flow_coupling="affine", LU_decomposed=False, num_dequant_blocks=0,
        coupling_network="tanh", coupling_network_depth=1, batch_norm=True, boosted=True, rho_iters=100, rho_lr=0.1)
    m = BoostedFlow(args)
    for c, spec in enumerate(synth.synth_boosted_specs("glow", C_, d, h, K, seed=1)):
        m.load_spec(c, spec)
    m.component = C_ - 1
    m.eval()
    return m


def fill(m, loader, table):
    """The table fill of fit_weights: every batch's component log-likelihoods into its columns, one launch per batch."""
    import torch
    from gbnf_amd import native
    n_used, filled = table.shape[0], 0
    with torch.no_grad(), torch.cuda.device(table.device):
        mix = m.native_mixture(n_used)
        for (x, _) in loader:
            mix.prepared_component_log_prob(x, table, 0, n_used, col_offset=filled)(native._stream_ptr())
            filled += x.shape[0]
    torch.cuda.synchronize()
    return {"rows": filled}


def em(table, rho, max_iters, tol):
    from gbnf_amd import native
    out = native.weights_report(native.weights_em(table, rho, max_iters, tol), table.shape[0])
    return {k: out[k] for k in ("nll_before", "nll_after", "iters", "converged")}


def eager_em(table, rho, max_iters, tol):
    """The iteration of gbnf_weights_em in eager torch float64 on the same table, one host read per iteration."""
    import torch
    ll = table.double()
    n_used, n = ll.shape
    w = rho[:n_used].double() / rho[:n_used].double().sum()
    t, prev, first = 0, None, None
    while True:
        a = torch.log(w)[:, None] + ll
        G = torch.logsumexp(a, dim=0)
        L = G.mean().item()
        first = L if first is None else first
        if (prev is not None and tol > 0 and abs(L - prev) <= tol) or t == max_iters:
            break
        w = torch.softmax(a, dim=0).mean(dim=1)
        prev, t = L, t + 1
    return {"nll_before": -first, "nll_after": -L, "iters": t, "converged": t < max_iters}


def timed(fn, passes):
    import torch
    torch.cuda.synchronize()
    t0 = time.perf_counter()
    for _ in range(passes):
        out = fn()
    torch.cuda.synchronize()
    return (time.perf_counter() - t0) * 1e3 / passes, out


def main(argv=None):
    ap = argparse.ArgumentParser()
    ap.add_argument("--repeats", type=int, default=9)
    ap.add_argument("--warmup", type=int, default=2)
    ap.add_argument("--passes", type=int, default=3, help="passes per timed window")
    ap.add_argument("--max-iters", type=int, default=1000)
    ap.add_argument("--tol", type=float, default=1e-9)
    a = ap.parse_args(argv)
    import torch
    from gbnf_amd import synth
    if not torch.cuda.is_available():
        raise SystemExit("bench_fit_weights.py needs the MI355X: there is no CPU path")
    dev = torch.device("cuda:0")
    torch.cuda.set_device(dev)
    m = model(dev)
    C_, batches, rows = m.num_components, 64, 512
    loader = Loader([(torch.from_numpy(synth.synth_batch(rows, 43, seed=100 + b)).to(dev), None) for b in range(batches)])
    rho0 = m.rho.detach().clone()
    table = torch.empty((C_, batches * rows), dtype=torch.float32, device=dev)
    fill(m, loader, table)

    def reset(fn):
        def run():
            with torch.no_grad():
                m.rho.copy_(rho0)
            return fn()
        return run

    def update_rho():
        m.update_rho(loader, fused=True)
        return {"rho_last": float(m.rho[C_ - 1])}

    fns = {"fit_weights": reset(lambda: m.fit_weights(loader, n_used=C_, max_iters=a.max_iters, tol=a.tol)),
           "fill": lambda: fill(m, loader, table),
           "em": lambda: em(table, rho0, a.max_iters, a.tol),
           "update_rho": reset(update_rho),
           "eager_em": lambda: eager_em(table, rho0, a.max_iters, a.tol)}
    for _ in range(a.warmup):
        for fn in fns.values():
            fn()
    times, outs = {k: [] for k in fns}, {}
    for _ in range(a.repeats):        # alternating: the machine's drift hits all legs alike
        for k, fn in fns.items():
            t, outs[k] = timed(fn, a.passes)
            times[k].append(t)
    res = {"shape": f"Boosted-Glow C={C_} d=43 h=215 K=5", "batches": batches, "rows_per_batch": rows, "max_iters": a.max_iters, "tol": a.tol,
           "repeats": a.repeats, "warmup": a.warmup, "passes_per_window": a.passes}
    for k, t in times.items():
        res[k + "_ms"] = {"median": statistics.median(t), "min": min(t), "max": max(t)}
    res.update(outs)
    reset(update_rho)()               # (outside the clock) the mixture's nll on the same rows under what update_rho leaves
    res["update_rho"]["nll_after"] = m.evaluate(loader, n_used=C_)["nll"]
    print(json.dumps(res), flush=True)
    return 0


if __name__ == "__main__":
    sys.exit(main())
