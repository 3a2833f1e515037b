#!/usr/bin/env python3
"""Drawing from the boosted mixture, MINIBOONE Boosted-Glow C = 8 (d = 43, h = 215, K = 5): samples/s of BoostedFlow.sample beside

  floor   the same n rows through ONE component's component_inverse: the same inverse work, no draw, partition or copies;
  eager   what a user writes without it: torch.multinomial per row, a boolean-mask loop over the components, a scatter back;

and where the time over the floor goes: the draw (gbnf_resample_rows alone), the partition (begin without z, minus the draw), the
gather (begin with z, minus begin without), the host read of the segment sizes, the C per-segment inverse launches (each on its
own rows, no copies) and the scatter (finish minus those launches).  z and the uniforms are made once and handed to every path, so
no path pays for the random numbers.  Every figure is a host clock around a loop that ends in a device synchronise, after a warm-up
of the same shape; the parts are timed in loops of their own and are differences of such figures, not a trace.
usage: python tools/bench_sample.py [--n 16,4096,65536] [--iters 200] [--out FILE]"""
import argparse
import os
import sys
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
import torch
from gbnf_amd import BoostedFlow, native, synth

ap = argparse.ArgumentParser()
ap.add_argument("--n", default="16,4096,65536")
ap.add_argument("--iters", type=int, default=200)
ap.add_argument("--out", default=None)
opt = ap.parse_args()

dev = torch.device("cuda:0")
NC, d, h, K = 8, 43, 215, 5
args = argparse.Namespace(
    num_flows=K, z_size=d, density_evaluation=True, device=dev, cuda=True, component_type="glow", num_components=NC, rho_init="decreasing",
    learn_top=False, y_classes=0, y_condition=False, sample_size=64, input_size=[d], h_size=h, num_blocks=1, actnorm_scale=1.0,
    flow_permutation="shuffle", flow_coupling="affine", LU_decomposed=False, num_dequant_blocks=0, coupling_network="tanh",
    coupling_network_depth=1, batch_norm=False)
m = BoostedFlow(args)
for c, spec in enumerate(synth.synth_boosted_specs("glow", NC, d, h, K, seed=1)):
    m.load_spec(c, spec)
m.eval()
m.all_trained = True
rho = m.rho.contiguous().float()
flows = [m.native_flow(c) for c in range(NC)]
lines = []


def say(s):
    print(s, flush=True)
    lines.append(s)


def timed(f, iters):
    """us per call: warm-up, then a synchronised window of at least `iters` calls and 0.3 s; the median of three windows."""
    for _ in range(max(3, iters // 10)):
        f()
    torch.cuda.synchronize()
    out = []
    for _ in range(3):
        k, t0 = 0, time.perf_counter()
        while k < iters or time.perf_counter() - t0 < 0.3:
            f()
            k += 1
        torch.cuda.synchronize()
        out.append((time.perf_counter() - t0) / k * 1e6)
    return sorted(out)[1]


def eager(z, simplex):
    comp = torch.multinomial(simplex, z.shape[0], replacement=True)
    x = torch.empty_like(z)
    for c in range(NC):
        mask = comp == c
        if bool(mask.any()):
            x[mask] = m.component_inverse(z[mask], c)[0]
    return x


say(f"# BoostedFlow.sample, MINIBOONE Boosted-Glow C = {NC} (d = {d}, h = {h}, K = {K}), decreasing rho; us per call, host clock around a "
    "synchronised loop")
for n in (int(v) for v in opt.n.split(",")):
    iters = max(20, opt.iters if n <= 4096 else opt.iters // 4)
    g = torch.Generator(device=dev)
    g.manual_seed(n)
    z = torch.randn(n, d, device=dev, generator=g)
    u = torch.rand(n, device=dev, generator=g)
    simplex = rho / rho.sum()
    # the three paths
    t_sample = timed(lambda: m.sample(z=z, uniforms=u), iters)
    t_floor = timed(lambda: m.component_inverse(z, 0), iters)
    t_eager = timed(lambda: eager(z, simplex), iters)
    # the parts
    t_draw = timed(lambda: native.resample_rows(rho, u), iters)
    t_part = timed(lambda: native.mixture_partition(rho, u, NC), iters)
    t_begin = timed(lambda: native.mixture_partition(rho, u, NC, z), iters)
    t_read = timed(lambda: native.mixture_partition(rho, u, NC, z)[2].cpu(), iters)
    comp, order, counts, _ = native.mixture_partition(rho, u, NC, z)
    sizes = counts.cpu().tolist()
    segs = [s.contiguous() for s in torch.split(z[order], sizes)]

    def launches():
        for c, s in enumerate(segs):
            if s.shape[0]:
                flows[c].inverse(s, want_ldj=False)
    t_launch = timed(launches, iters)
    t_native = timed(lambda: native.mixture_sample(flows, rho, u, z, want_ldj=False), iters)
    x = m.sample(z=z, uniforms=u)
    ok = all(torch.equal(x[order[sum(sizes[:c]):sum(sizes[:c + 1])]], flows[c].inverse(segs[c], want_ldj=False)[0])
             for c in range(NC) if sizes[c])
    say(f"n = {n:6d}  segments {sizes}  rows bit-equal to the per-component inverse: {ok}")
    say(f"  sample {t_sample:9.1f} us ({n / t_sample:8.3f} M samples/s) | floor {t_floor:9.1f} us ({n / t_floor:8.3f} M/s) | "
        f"eager mask loop {t_eager:9.1f} us ({n / t_eager:8.3f} M/s) | sample / floor {t_sample / t_floor:5.2f} x, eager / sample "
        f"{t_eager / t_sample:5.2f} x")
    say(f"  parts: draw {t_draw:7.1f} | partition {t_part - t_draw:7.1f} | gather {t_begin - t_part:7.1f} | host read {t_read - t_begin:7.1f} | "
        f"{sum(1 for s in sizes if s)} inverse launches {t_launch:8.1f} | scatter + finish {t_native - t_read - t_launch:7.1f} | "
        f"module over native.mixture_sample {t_sample - t_native:6.1f}   (native.mixture_sample {t_native:9.1f} us)")
if opt.out:
    os.makedirs(os.path.dirname(os.path.abspath(opt.out)), exist_ok=True)
    with open(opt.out, "w") as f:
        f.write("\n".join(lines) + "\n")
