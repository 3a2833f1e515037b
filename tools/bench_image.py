#!/usr/bin/env python3
"""BASELINE.json configs[3]: CIFAR-10 3x32x32 multi-scale Boosted-Glow C=4 (K=8 steps per level, L=2 levels, h=256,
invconv, affine, learned top prior), density evaluation of a batch of synthetic images already resident in HBM:
all C components + the mixture log-sum-exp -> G (N,).  Prints one JSON line (same fields as bench.py).

    python tools/bench_image.py [--batch 64 --components 4 --K 8 --hidden 256 --steps 20 --warmup 3 --cpu-seconds 15]
"""
import argparse
import json
import os
import sys
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

import numpy as np
import torch

F32_MFMA_PEAK_TFLOPS = 157.3   # MI355X_MICROARCH.md: dense f32 matrix peak
F16_MFMA_PEAK_TFLOPS = 2500.0  # dense f16/bf16 matrix peak (no sparsity)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--batch", type=int, default=64)
    ap.add_argument("--components", type=int, default=4)
    ap.add_argument("--K", type=int, default=8)
    ap.add_argument("--L", type=int, default=2)
    ap.add_argument("--hidden", type=int, default=256)
    ap.add_argument("--depth", type=int, default=1, help="--coupling_network_depth: 1x1 layers between the two 3x3s (0, 1, 2)")
    ap.add_argument("--input", type=int, nargs=3, default=[3, 32, 32], metavar=("C", "H", "W"),
                    help="image shape: 3 32 32 (CIFAR: BASELINE configs[3], the default), 1 28 28 (MNIST / Omniglot / Caltech), 1 28 20 (Frey faces)")
    ap.add_argument("--steps", type=int, default=40)        # (10 steps read 6 % low: the first replays of a fresh graph are slower)
    ap.add_argument("--warmup", type=int, default=5)
    ap.add_argument("--cpu-seconds", type=float, default=15.0)
    ap.add_argument("--graph", dest="graph", action="store_true", default=True,
                    help="capture one step in a HIP graph and replay it (default since round 3: a step is ~200 short launches and "
                         "host-bound as plain stream launches; the stream-launch rate is reported beside it)")
    ap.add_argument("--no-graph", dest="graph", action="store_false", help="time plain stream launches only")
    ap.add_argument("--no-streams", dest="streams", action="store_false",
                    help="all components on one stream (default: one HIP stream per component, their launch chains overlap, "
                         "as BoostedImageFlow.component_log_prob does)")
    ap.add_argument("--eval-deterministic", dest="eval_deterministic", action="store_true",
                    help="the handles' deterministic mode (gbnf_image_flow_set_deterministic: ordered log-det sums); without it "
                         "nothing changes")
    a = ap.parse_args()
    from gbnf_amd import native, synth
    from oracle import gbnf_oracle as oracle
    dev = torch.device("cuda:0")
    size = tuple(a.input)
    specs = [synth.synth_image_glow_spec(size, a.hidden, a.K, a.L, seed=100 + c, depth=a.depth) for c in range(a.components)]
    flows = [native.NativeImageFlow(sp) for sp in specs]
    if a.eval_deterministic:
        for f in flows:
            f.deterministic = True
    x_np, noise_np = synth.synth_image_batch(a.batch, size, seed=0)
    x, noise = torch.from_numpy(x_np).to(dev), torch.from_numpy(noise_np).to(dev)
    rho = torch.clamp(1.0 / torch.pow(2.0, torch.arange(a.components * 1.0)), min=0.05).to(dev)
    ll = torch.empty((a.components, a.batch), dtype=torch.float32, device=dev)

    streams = [torch.cuda.Stream() for _ in flows] if a.streams else None

    def step():
        if streams is None:
            for c, f in enumerate(flows):
                ll[c] = f.forward(x, noise, want_z=False)[2]
            return native.mixture_lse(ll, rho)
        # the components are independent until the recursion: one stream each, so that their (latency-bound) launch
        # chains overlap on the GPU
        cur = torch.cuda.current_stream()
        for c, (f, s_) in enumerate(zip(flows, streams)):
            s_.wait_stream(cur)
            with torch.cuda.stream(s_):
                ll[c] = f.forward(x, noise, want_z=False)[2]
        for s_ in streams:
            cur.wait_stream(s_)
        return native.mixture_lse(ll, rho)

    for _ in range(a.warmup):
        G = step()
    torch.cuda.synchronize()
    run = step
    stream_rate = None
    if a.graph:      # the plain stream-launch form first (what rounds 1-2 reported as `value`)
        t0 = time.perf_counter()
        for _ in range(a.steps):
            step()
        torch.cuda.synchronize()
        stream_rate = a.batch / ((time.perf_counter() - t0) / a.steps)
    if a.graph:      # the ~50 launches per component replayed as one HIP graph (same kernels, same buffers)
        graph = torch.cuda.CUDAGraph()
        side = torch.cuda.Stream()
        side.wait_stream(torch.cuda.current_stream())
        with torch.cuda.stream(side):
            step()
        torch.cuda.current_stream().wait_stream(side)
        with torch.cuda.graph(graph):
            G_static = step()

        def run():
            graph.replay()
            return G_static
        run()
        torch.cuda.synchronize()
    ev0, ev1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    t0 = time.perf_counter()
    ev0.record()
    for _ in range(a.steps):
        G = run()
    ev1.record()
    torch.cuda.synchronize()
    dt = (time.perf_counter() - t0) / a.steps
    gpu_ms = ev0.elapsed_time(ev1) / a.steps
    flops = 2.0 * sum(f.macs_per_image for f in flows) * a.batch
    exact = os.environ.get("GBNF_MATH") == "f32"                       # which kernels the coupling nets ran on (depth 1 here)
    peak = F32_MFMA_PEAK_TFLOPS if exact else F16_MFMA_PEAK_TFLOPS
    # CPU baseline: the oracle (torch CPU, reference op order) on a bounded sample of the same images
    # (threads: the fastest of a quick probe over {1, 4, 8, 16, 32, 64} on ONE pass of the stated sample, as bench.py's headline leg)
    ns = min(a.batch, 4)
    host_cores = os.cpu_count() or 1
    cands = [t for t in (1, 4, 8, 16, 32, 64) if t <= host_cores] or [1]
    probe, best_t = {}, cands[0]
    with torch.no_grad():
        oracle.image_component_forward(specs[0], x_np[:1], noise_np[:1])
        for t in (cands if a.cpu_seconds > 0 else []):
            torch.set_num_threads(t)
            oracle.image_component_forward(specs[0], x_np[:1], noise_np[:1])
            t0 = time.perf_counter()
            oracle.image_component_forward(specs[0], x_np[:ns], noise_np[:ns])
            probe[t] = ns / (time.perf_counter() - t0)
            if probe[t] >= probe[best_t]:
                best_t = t
        torch.set_num_threads(best_t)
        t0 = time.perf_counter()
        passes = 0
        G_cpu = None
        while True:
            lls = [oracle.image_component_forward(sp, x_np[:ns], noise_np[:ns])[4] for sp in specs]
            G_cpu = oracle.mixture_recursion(np.stack(lls), rho.cpu().numpy())
            passes += 1
            if time.perf_counter() - t0 > a.cpu_seconds:
                break
        cpu_dt = (time.perf_counter() - t0) / passes
    err = float(np.abs(G.cpu().numpy()[:ns] - G_cpu).max() / np.abs(G_cpu).max())
    print(json.dumps({
        "metric": "density-eval images/sec, CIFAR-10 3x32x32 multi-scale Boosted-Glow" if size == (3, 32, 32)
                  else f"density-eval images/sec, {size[0]}x{size[1]}x{size[2]} multi-scale Boosted-Glow", "value": a.batch / dt, "unit": "images/s",
        "n_gpus": 1, "steps": a.steps, "warmup": a.warmup, "ms_per_step": dt * 1e3, "higher_is_better": True,
        "scaling": "strong", "vs_baseline": None, "dtype": "f32" if exact else "f16x3", "data": "synthetic",
        "stream_launches_value": stream_rate,
        "config": {"workload": f"{'cifar_glow' if size == (3, 32, 32) else 'image_glow'}: {size[0]}x{size[1]}x{size[2]}, C={a.components} components, K={a.K} steps x L={a.L} levels, h={a.hidden}, "
                               f"invconv, affine, learn_top, batch={a.batch}, synthetic images + weights",
                   "launch": ("HIP graph replay" if a.graph else "stream launches") + (", one stream per component" if a.streams else ""),
                   **({"eval_deterministic": True} if a.eval_deterministic else {})},
        # the coupling nets (99 % of the FLOPs) run on the split-f16 kernels img_mid_hx3 / img_last_hx3 unless GBNF_MATH=f32:
        # the peak is that of the pipe they run on; achieved = ALGORITHMIC f32 FLOPs (the f16 pipe executes 3x that)
        "roofline": {"kernel": "gbnf::img_conv_kernel (all convolutions, exact f32)" if exact else
                               "gbnf::img_net_hx3_kernel (one fused kernel per coupling net, f16x3) + img_conv_kernel (1x1 mixes, Split2d priors: f32)",
                     "bound": "mfma", "achieved": flops / (gpu_ms * 1e-3) / 1e12,
                     "peak": peak, "unit": "TFLOP/s", "frac": flops / (gpu_ms * 1e-3) / 1e12 / peak,
                     "vs_f32_mfma_peak": flops / (gpu_ms * 1e-3) / 1e12 / F32_MFMA_PEAK_TFLOPS,
                     "executed_frac": (1.0 if exact else 3.0) * flops / (gpu_ms * 1e-3) / 1e12 / peak,
                     "traffic": measured_traffic(a), "gpu_ms_per_step": gpu_ms, "flops_per_step": flops},
        "cpu_baseline": {"value": ns / cpu_dt, "unit": "images/s", "cores": torch.get_num_threads(), "kind": "port",
                         "host_cores": host_cores, "thread_probe_images_per_s": {str(k): v for k, v in probe.items()},
                         "sample": f"{passes} pass(es) over {ns} of the {a.batch} images, all {a.components} components + recursion, "
                                   f"torch-CPU oracle in the reference's op order, {torch.get_num_threads()} threads (fastest of {cands})"},
        "speedup_vs_cpu": (a.batch / dt) / (ns / cpu_dt), "max_rel_err_vs_cpu": err}))


def measured_traffic(a):
    """HBM-side bytes per benchmark step (all kernels of the step) from the PMC passes committed under profiles/
    (2 x FETCH_SIZE + WRITE_SIZE, MI355X_MICROARCH.md) -- only for the exact workload they were taken on."""
    try:
        rec = json.load(open(os.path.join(ROOT, "profiles", "image_traffic.json")))
    except (OSError, ValueError):
        return None
    for r in rec.get("workloads", []):
        w = r.get("workload", {})
        if tuple(w.get("input", (3, 32, 32))) == tuple(a.input) and \
                (w.get("batch"), w.get("components"), w.get("K"), w.get("L"), w.get("hidden")) == (a.batch, a.components, a.K, a.L, a.hidden) \
                and os.environ.get("GBNF_MATH", "default") == w.get("math", "default"):
            return float(r["traffic_bytes_per_step"])
    return None


if __name__ == "__main__":
    main()
