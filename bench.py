#!/usr/bin/env python3
"""Headline benchmark: density-eval samples/sec of a Boosted-Glow mixture on MI355X.

    python bench.py [--gpus N --steps K --warmup W] [--dump-outputs DIR] [--full]
    python -m torch.distributed.run --nnodes=1 --nproc-per-node N --master-addr 127.0.0.1 \
        --master-port P bench.py --gpus N --steps K --warmup W

`python bench.py --gpus N` with N > 1 and no WORLD_SIZE in the environment starts that launcher itself as a child
process (before anything here touches torch or the GPU) and relays rank 0's JSON line.

Workload (BASELINE.json metric): MINIBOONE-shaped d=43, Boosted-Glow C=8 (K=5 flow steps, coupling
net 21->215->215->44 tanh, shuffle permutation, affine coupling), batch 4096 synthetic N(0,1) rows
already resident in HBM, random-init synthetic weights.  One "step" = one pass of the hot path over
one batch: all C component flows + the mixture log-sum-exp  ->  G (N,).

Consecutive batches are independent, so they are served in groups of S = 32 (the same S for every N: one flow launch,
one all-gather, one recursion launch per group -- gbnf_amd.sharded.GroupPipeline, the class the GPU tests exercise).
N > 1: the C components are sharded over the ranks (contiguous blocks, C/N each), x is replicated, one RCCL all-gather
of float32[C/N, S*batch] per rank per group rebuilds (C, S*batch) before the recursion; total work is fixed =>
"scaling": "strong".

Timing: 2000 x `--prewarm` untimed steps let the clocks of a cold GPU settle, then W untimed warm-up steps, then exactly
K timed steps between barriers + device synchronisations, MAX over ranks.

A plain run does only that and prints the line: set-up, warm-up, the K timed steps, the outputs of the last timed step if
`--dump-outputs DIR` is given (DIR/G.npy: G (batch,) of that step, float32; inputs and weights come from fixed seeds, so two
runs with the same arguments compute from identical inputs), and the result line.  `--full` adds everything else the
benchmark measures: the CPU baseline, the other legs and BASELINE configurations, the repetitions of a short timed region
(a run of fewer than 4 groups is repeated 21 x and `value` comes from the median repetition) and the full record.

Prints ONE JSON line on rank 0, the LAST line on stdout, at most LINE_LIMIT (6000) bytes (compact_line: the driver contract's
keys only), including
  "ms_per_step":  milliseconds one timed step took
  "dtype":        the arithmetic the timed kernel computes in ("f16x3" = f32 operands split into two fp16 pieces, three
                  f16 MFMAs per product, f32 accumulate; "bf16x6"; "f32" = exact f32-input MFMA)
  "roofline":     dominant kernel (the fused flow kernel) against the dense MFMA peak of the pipe it runs on
  "cpu_baseline": (--full) the torch-CPU oracle ("port" of the reference path) timed on this box's cores
  "configs" / "legs_summary": (--full, N = 1) one [value, frac, executed_frac] triple per other BASELINE configuration / leg.
Everything else a --full run measures -- the legs in full (the exact-f32 kernel, one batch per launch, the reference's batch
sizes, the module's evaluate loop, every other configuration's own line), the notes, the thread probes -- goes to stderr
and to the side file the line names ("full_record", set by --full-record).
"""
import argparse
import ctypes
import json
import os
import subprocess
import sys
import time

REPO = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, REPO)

F32_MFMA_PEAK_TFLOPS = 157.3   # /opt/skills/guides/MI355X_MICROARCH.md: dense f32 matrix peak
F16_MFMA_PEAK_TFLOPS = 2500.0  # same guide: dense bf16/f16 matrix peak (no sparsity)
HBM_PEAK_GBS = 8000.0          # same guide: HBM3E spec peak
GROUP = 32                     # batches per flow launch / all-gather / recursion launch, for every N (at 8 GPUs a rank
                               # holds one component: a 16-batch launch is a single round of workgroups, 123 us, and the
                               # per-group host + collective cost shows; 32 measured +10 % there, +1-3 % at N = 1)

ROWS_PER_ROUND = 65536         # one round of the split kernel's workgroups: 256 CUs x 2 workgroups x 4 waves x 32 samples

CONFIGS = {
    # name: (kind, d, h, K, default C, default batch)
    "miniboone_glow": ("glow", 43, 215, 5, 8, 4096),
    "hepmass_realnvp": ("realnvp", 21, 105, 5, 8, 65536),
}
MATH_NAME = {0: "f32", 1: "f16x3", 2: "bf16x6"}
MATH_TEXT = {
    "f32": "f32: exact f32-input MFMA (v_mfma_f32_16x16x4_f32)",
    "f16x3": "f16x3: f32 operands split into two fp16 pieces, 3 f16 MFMAs per product, f32 accumulate",
    "bf16x6": "bf16x6: f32 operands split into three bf16 pieces, 6 bf16 MFMAs per product, f32 accumulate",
}
PRODUCTS = {"f32": 1.0, "f16x3": 3.0, "bf16x6": 6.0}


LINE_LIMIT = 6000          # bytes: the driver parses the LAST stdout line and keeps only a few KB of it (BENCH_r05: a 20 KB line
                           # came back `parsed: null`); everything else goes to stderr and to FULL_RECORD
FULL_RECORD = os.path.join("gpurun_out", "bench_full.json")


def _pick(dct, keys):
    return {k: dct[k] for k in keys if isinstance(dct, dict) and k in dct}


def _short(v, n):
    return v if not isinstance(v, str) or len(v) <= n else v[: n - 3] + "..."


def compact_line(out, full_record=FULL_RECORD):
    """The ONE line the driver parses: the contract's keys, `roofline` and `cpu_baseline` as the tier asks for them, and one
    (value, frac, executed_frac) triple per other configuration -- nothing else.  The legs, the notes and the thread probes are in
    the full record (stderr + `full_record`).  Kept under LINE_LIMIT by construction: free-text fields are clipped, and if a
    worst case still overflows, the optional blocks go one by one (tests/test_bench_host.py feeds it one)."""
    rl, cb, lg = out.get("roofline") or {}, out.get("cpu_baseline"), out.get("legs") or {}
    line = _pick(out, ("metric", "value", "unit", "n_gpus", "steps", "warmup", "ms_per_step", "higher_is_better", "scaling",
                       "vs_baseline", "dtype", "data"))
    cfg = _pick(out.get("config") or {}, ("workload", "global_batch", "components", "group", "parallelism", "emulated"))
    line["config"] = {k: _short(v, 160) for k, v in cfg.items()}
    line["timing"] = _pick(out.get("timing") or {}, ("repetitions", "value_from", "elapsed_ms_median", "elapsed_ms_min", "elapsed_ms_max"))
    r = _pick(rl, ("kernel", "bound", "achieved", "peak", "unit", "frac", "executed_frac", "traffic", "launch_ms", "flops_per_launch",
                   "hbm_algorithmic_bytes_per_launch"))
    if "kernel" in r:
        r["kernel"] = _short(r["kernel"], 120)
    src = rl.get("traffic_source")
    r["traffic_source"] = (f"{src.get('file')} ({src.get('pmc_summary')}, taken {src.get('taken')}): looked up by exact workload, "
                           "not counted in this run") if isinstance(src, dict) else None
    line["roofline"] = r
    if isinstance(cb, dict):
        c = _pick(cb, ("value", "unit", "cores", "kind", "cpu_model", "host_cores", "one_thread_value", "sample"))
        c["sample"] = _short(c.get("sample"), 300)
        line["cpu_baseline"] = c
    else:
        line["cpu_baseline"] = cb
    line.update(_pick(out, ("speedup_vs_cpu", "max_rel_err_vs_cpu")))
    if isinstance(out.get("rccl"), dict):
        rc = out["rccl"]
        line["rccl"] = {"ranks_seen": rc.get("ranks_seen"), "allgather_us": rc.get("allgather_us"),
                        "allgather_bytes_per_rank": rc.get("allgather_bytes_per_rank"),
                        "pipeline": _short((rc.get("pipeline") or {}).get("kind"), 40),
                        "fallback_reason": _short((rc.get("pipeline") or {}).get("fallback_reason"), 120)}
    g = out.get("numerics_guard")
    if isinstance(g, dict):
        line["numerics_guard"] = _pick(g, ("checks", "worst_rel_err", "demoted", "tolerance"))

    def val(name, key="value"):
        v = lg.get(name)
        return v.get(key) if isinstance(v, dict) else None
    if lg:
        small = lg.get("reference_batch_sizes") or {}
        line["legs_summary"] = {
            "group1": [val("group1"), val("group1", "frac")],
            "f32_exact": [val("f32_exact"), val("f32_exact", "frac")],
            "bf16x6": [val("bf16x6"), val("bf16x6", "executed_frac")],
            "fresh_batches": val("fresh_batches"),
            "log_prob_us_per_call": {k: (v.get("us_per_call") if isinstance(v, dict) else None) for k, v in small.items() if k.isdigit()},
            "module_evaluate_loop": val("module_evaluate_loop"), "module_calls_only_ms": val("module_evaluate_loop", "module_calls_only_ms"),
            "boosted_step_batch512_ms": ((lg.get("configs") or {}).get("boosted_step_batch512") or {}).get("ms_per_step"),
            "boosted_step_batch512_library_ms": ((lg.get("configs") or {}).get("boosted_step_batch512") or {}).get("library_ms_per_step"),
        }
        cfgs = lg.get("configs") or {}
        line["configs"] = {_short(k, 60): ([v.get("value"), (v.get("roofline") or {}).get("frac"), (v.get("roofline") or {}).get("executed_frac")]
                                           if isinstance(v, dict) and "error" not in v else "error")
                           for k, v in cfgs.items()}
        line["configs_columns"] = ["value (unit of that workload)", "roofline.frac", "roofline.executed_frac"]
    line["full_record"] = full_record
    text = json.dumps(line, separators=(",", ":"))
    for drop in ("legs_summary", "configs_columns", "configs", "numerics_guard", "timing", "rccl"):
        if len(text) <= LINE_LIMIT:
            break
        line.pop(drop, None)
        line["dropped_for_length"] = line.get("dropped_for_length", []) + [drop]
        text = json.dumps(line, separators=(",", ":"))
    if len(text) > LINE_LIMIT:
        raise AssertionError(f"bench line is {len(text)} bytes > {LINE_LIMIT}")
    return text


def emit_full_record(out, path=FULL_RECORD):
    """Everything measured (legs, notes, probes): pretty-printed to stderr and written next to the other gpurun outputs."""
    text = json.dumps(out, indent=1, default=str)
    print("[bench] full record follows (stderr); the driver's line is the last line on stdout", file=sys.stderr)
    print(text, file=sys.stderr)
    try:
        os.makedirs(os.path.dirname(os.path.join(REPO, path)), exist_ok=True)
        with open(os.path.join(REPO, path), "w") as f:
            f.write(text + "\n")
    except OSError as e:
        print(f"[bench] could not write {path}: {e}", file=sys.stderr)


def _cpu_model():
    try:
        with open("/proc/cpuinfo") as f:
            for line in f:
                if line.lower().startswith("model name"):
                    return line.split(":", 1)[1].strip()
    except OSError:
        pass
    return "unknown"


def cpu_baseline(specs, rho, x_np, budget_s):
    """Times the oracle (torch CPU, the reference's op order) on a bounded sample of the SAME workload.

    Thread count: the reference sets torch.set_num_threads(cores - 1) (density_experiment.py:280-287),
    which is pathological on a many-core host for these small GEMMs (256 threads: ~100 s per pass), so
    the baseline is given its best setting: a quick probe over {1, 4, 8, 16, 32, 64} threads ON THE STATED WORKLOAD (all
    components + recursion, 1024 rows) picks the fastest, and `cores` reports the threads actually used.  Then whole passes (all components + recursion) are
    timed until ~budget_s seconds are spent (first pass untimed).  `one_thread_value` is the same whole pass (all
    components + recursion) on ONE thread over a bounded row sample (the reference scripts' own default is one worker)."""
    import torch
    from oracle import gbnf_oracle as oracle
    host_cores = os.cpu_count() or 1
    cands = [t for t in (1, 4, 8, 16, 32, 64) if t <= host_cores] or [1]
    probe_x = x_np[: min(1024, x_np.shape[0])]
    best_t, best_dt = cands[0], None
    probe = {}
    with torch.no_grad():
        # the probe runs the STATED workload (every component + the recursion), not one component: the best thread count
        # of a single 1024 x 215 GEMM chain is not the best one of the whole pass on a many-core host
        for t in cands:
            torch.set_num_threads(t)
            oracle.mixture_log_prob(specs, rho, probe_x[:128])       # warm
            t0 = time.perf_counter()
            oracle.mixture_log_prob(specs, rho, probe_x)
            dt = time.perf_counter() - t0
            probe[t] = probe_x.shape[0] / dt
            if best_dt is None or dt < best_dt:
                best_t, best_dt = t, dt
            if dt > 4.0:
                break
        # one thread, the stated workload (all components + the recursion) on a row sample worth ~2 s
        torch.set_num_threads(1)
        n1 = min(x_np.shape[0], 1024)
        oracle.mixture_log_prob(specs, rho, x_np[:64])
        t0 = time.perf_counter()
        oracle.mixture_log_prob(specs, rho, x_np[:n1])
        one_thread = n1 / (time.perf_counter() - t0)
        torch.set_num_threads(best_t)
        est = best_dt * x_np.shape[0] / probe_x.shape[0]
        n = x_np.shape[0]
        if est > budget_s / 2:                                        # keep the leg bounded: fewer rows
            n = max(256, int(x_np.shape[0] * (budget_s / 2) / est))
        xs = x_np[:n]
        ll, G = oracle.mixture_log_prob(specs, rho, xs)               # warm-up pass (untimed)
        t0 = time.perf_counter()
        passes = 0
        while True:
            ll, G = oracle.mixture_log_prob(specs, rho, xs)
            passes += 1
            el = time.perf_counter() - t0
            if el >= budget_s or passes >= 500:
                break
    return {
        "value": n * passes / el, "unit": "samples/s", "cores": best_t, "kind": "port",
        "host_cores": host_cores, "cpu_model": _cpu_model(), "one_thread_value": one_thread,
        "thread_probe_samples_per_s": {str(k): v for k, v in probe.items()},
        "one_thread_sample": f"one pass over {n1} rows, all {len(specs)} components + mixture recursion, 1 thread",
        "sample": f"{passes} pass(es) over {n} of the {x_np.shape[0]} rows, all {len(specs)} components + mixture "
                  f"recursion, torch-CPU oracle in the reference's op order, {best_t} threads "
                  f"(fastest of {cands}), {el:.1f} s",
    }, G, n


def module_evaluate_leg(specs, kind, d, h, K, C, xs, iters=100):
    """What "drops into density_experiment.py unchanged" costs: the reference's evaluate loop
    (density_experiment.py:561-573: one model(x=x, components=c) call per component, the base density and the 2-way
    logsumexp recursion in torch ops) through the drop-in module, host time included, and the module's one-call form.
    Every iteration evaluates ANOTHER batch tensor (xs is cycled, as a data loader would): since round 4 the module serves the
    loop's C calls on one batch from ONE launch, and a loop over one and the same tensor would time table look-ups only."""
    import math
    import torch
    from gbnf_amd import BoostedFlow
    x = xs[0]
    dev = x.device
    ns = argparse.Namespace(
        num_flows=K, z_size=d, density_evaluation=True, device=dev, cuda=True, component_type=kind, num_components=C,
        rho_init="decreasing", learn_top=False, y_classes=0, y_condition=False, sample_size=4, input_size=[d], h_size=h,
        num_blocks=1, actnorm_scale=1.0, flow_permutation="shuffle", flow_coupling="affine", LU_decomposed=False,
        num_dequant_blocks=0, coupling_network="tanh", coupling_network_depth=1, batch_norm=True)
    model = BoostedFlow(ns).to(dev)
    for c, sp in enumerate(specs):
        model.load_spec(c, sp)
    model.component = C - 1
    model.all_trained = True
    model.eval()

    if len(xs) < 2:
        raise ValueError("module_evaluate_leg needs at least two distinct batches")
    turn = [0]

    def reference_loop():
        x = xs[turn[0] % len(xs)]
        turn[0] += 1
        G_ll = None
        for c in range(model.component + 1):
            z_G, _, _, ldj_G, _ = model(x=x, components=c)
            ll = torch.sum(-0.5 * math.log(2 * math.pi) - 0.5 * z_G.pow(2), dim=-1) + ldj_G
            if c == 0:
                G_ll = ll
            else:
                rho_simplex = model.rho[0:(c + 1)] / torch.sum(model.rho[0:(c + 1)])
                last_ll = torch.log(1 - rho_simplex[c]) + G_ll
                next_ll = torch.log(rho_simplex[c]) + ll
                G_ll = torch.logsumexp(torch.cat([last_ll.view(-1, 1), next_ll.view(-1, 1)], dim=1), dim=1)
        return G_ll

    def timed(fn):
        with torch.no_grad():
            for _ in range(10):
                out = fn()
            torch.cuda.synchronize()
            t0 = time.perf_counter()
            for _ in range(iters):
                out = fn()
            torch.cuda.synchronize()
        return (time.perf_counter() - t0) / iters, out

    t_loop, _ = timed(reference_loop)
    # ... taken apart: the module calls alone (the first of a batch launches all C components, the others read its table) and
    # the caller's own torch ops alone (the module's outputs precomputed): ~17 small eager launches per component
    def calls_only():
        xb = xs[turn[0] % len(xs)]
        turn[0] += 1
        return [model(x=xb, components=c) for c in range(model.component + 1)]

    pre = [(o[0], o[3]) for o in calls_only()]

    def ops_only():
        G_ll = None
        for c, (z_G, ldj_G) in enumerate(pre):
            ll = torch.sum(-0.5 * math.log(2 * math.pi) - 0.5 * z_G.pow(2), dim=-1) + ldj_G
            if c == 0:
                G_ll = ll
            else:
                rho_simplex = model.rho[0:(c + 1)] / torch.sum(model.rho[0:(c + 1)])
                last_ll = torch.log(1 - rho_simplex[c]) + G_ll
                next_ll = torch.log(rho_simplex[c]) + ll
                G_ll = torch.logsumexp(torch.cat([last_ll.view(-1, 1), next_ll.view(-1, 1)], dim=1), dim=1)
        return G_ll

    t_calls, _ = timed(calls_only)
    t_ops, _ = timed(ops_only)
    turn[0] = 0
    with torch.no_grad():
        G_loop = reference_loop()          # batch 0: what the pipeline's G0 and log_prob(x) below are compared with
    t_one, G_one = timed(lambda: model.log_prob(x))
    n = x.shape[0]
    return {"value": n / t_loop, "unit": "samples/s", "ms_per_batch": 1e3 * t_loop, "iters": iters,
            "log_prob_one_call_value": n / t_one, "log_prob_one_call_ms": 1e3 * t_one,
            "max_abs_diff_loop_vs_one_call": float((G_loop - G_one).abs().max().item()),
            "batches_cycled": len(xs),
            "module_calls_only_ms": 1e3 * t_calls, "callers_torch_ops_only_ms": 1e3 * t_ops,
            "value_if_the_callers_ops_were_free": n / t_calls,
            "bound": "the CALLER's own eager torch ops (base density + recursion: ~17 launches per component, host-bound) -- "
                     "callers_torch_ops_only_ms is this loop with the module's outputs precomputed",
            "note": "the reference's own evaluate loop through the drop-in BoostedFlow module, a different batch tensor every "
                    "iteration: C forward calls returning (z, ldj) -- the first launches all C components of the batch, the "
                    "others read its table -- + the base density and the recursion in torch ops, host time included; "
                    "log_prob_one_call = model.log_prob(x) (one flow launch + one recursion launch)"}, G_loop


def measured_traffic(config, B, C, S, math, world):
    """HBM-side bytes per launch of the dominant kernel from the PMC passes committed under profiles/ (FETCH_SIZE x 2
    + WRITE_SIZE, collected as MI355X_MICROARCH.md prescribes) -- only for the exact workload they were taken on."""
    path = os.path.join(REPO, "profiles", "headline_traffic.json")
    try:
        rec = json.load(open(path))
    except (OSError, ValueError):
        return None
    for r in [rec] + list(rec.get("other_group_sizes", [])):
        w = r.get("workload", {})
        if (w.get("config") == config and w.get("batch") == B and w.get("components") == C and w.get("group") == S
                and w.get("math") == math and w.get("n_gpus") == world):
            return float(r["traffic_bytes_per_launch"])
    return None


def traffic_source():
    """Where `roofline.traffic` comes from: NOT counted in this run -- looked up in the committed PMC passes of the same workload."""
    path = os.path.join(REPO, "profiles", "headline_traffic.json")
    try:
        rec = json.load(open(path))
    except (OSError, ValueError):
        return None
    return {"file": "profiles/headline_traffic.json", "pmc_summary": rec.get("source"), "taken": rec.get("taken"),
            "note": "looked up by exact workload (config, batch, components, group, math, n_gpus) in the committed rocprofv3 --pmc passes "
                    "(FETCH_SIZE x 2 + WRITE_SIZE, separate passes); not counted in this run -- null when this run's workload has no pass"}


def config_legs(args):
    """The other BASELINE.json configurations, each as a CHILD process that runs before this one touches the GPU (a process
    that has initialised the GPU must not start another program; the children run one after the other, alone on the device):
    configs[1] MINIBOONE Boosted-Glow C=4 batch 4096, configs[2] HEPMASS Boosted-RealNVP C=8 batch 65536, configs[3] CIFAR-10
    multi-scale Boosted-Glow C=4 (batch 256, HIP-graph replay of the whole step), and the one-component training step at
    N = 65536, and configs[4]'s per-rank load emulated on this GPU.  Each leg carries value / dtype / roofline{frac, executed_frac, traffic} / cpu_baseline from
    its own run (bounded CPU samples: ~3 s each); a leg that fails reports its error and never takes the headline down."""
    py = sys.executable
    bench = os.path.abspath(__file__)
    tools = os.path.join(REPO, "tools")
    cpu = str(min(3.0, args.cpu_seconds))
    jobs = [
        ("miniboone_glow_c4_n4096", [py, bench, "--full", "--config", "miniboone_glow", "--components", "4", "--steps", "2048", "--prewarm", "0.1",
                                     "--cpu-seconds", cpu, "--no-extra-legs", "--no-config-legs"]),
        ("hepmass_realnvp_c8_n65536", [py, bench, "--full", "--config", "hepmass_realnvp", "--steps", "256", "--warmup", "32", "--prewarm", "0.02",
                                       "--cpu-seconds", cpu, "--no-extra-legs", "--no-config-legs"]),
        ("cifar10_glow_c4_n256", [py, os.path.join(tools, "bench_image.py"), "--batch", "256", "--steps", "40", "--warmup", "5",
                                  "--cpu-seconds", cpu]),
        # ... and at the reference's own evaluation batch (image_experiment.py:64: --eval_batch_size 1024)
        ("cifar10_glow_c4_n1024", [py, os.path.join(tools, "bench_image.py"), "--batch", "1024", "--steps", "20", "--warmup", "3",
                                   "--cpu-seconds", "0"]),
        ("train_step_miniboone_c1_n65536", [py, os.path.join(tools, "bench_train.py"), "--batch", "65536", "--steps", "30", "--warmup", "5",
                                            "--cpu-steps", "2" if args.cpu_seconds > 0 else "0", "--no-torch-legs"]),
        # the other coupling networks the reference constructs (round 5: on the register-chained training kernels too)
        ("train_step_hepmass_residual_c1_n65536", [py, os.path.join(tools, "bench_train.py"), "--config", "hepmass_realnvp_residual", "--batch", "65536",
                                                   "--steps", "20", "--warmup", "5", "--cpu-steps", "0", "--no-torch-legs"]),
        ("train_step_miniboone_depth2_c1_n65536", [py, os.path.join(tools, "bench_train.py"), "--config", "miniboone_glow_depth2", "--batch", "65536",
                                                   "--steps", "20", "--warmup", "5", "--cpu-steps", "0", "--no-torch-legs"]),
        # the reference's OWN training step (density_experiment.py:606-674 at --batch_size 512: weights from the fixed components, resample,
        # recorded forward, nll, backward, Adam) through the drop-in module, and the library's share of it
        ("boosted_step_batch512", [py, os.path.join(tools, "bench_boosted_step.py"), "--batch", "512", "--steps", "200"]),
        # configs[4] (MINIBOONE C = 8 sharded one component per GPU) as far as one GPU can show it: ONE rank's share of the 8-GPU
        # run -- one component on every batch, the gather of the full (8, S N) table through the library's RCCL communicator
        # (world size 1: the copy, not the xGMI hop), the recursion -- at the driver's own --steps 20 and in steady state
        ("miniboone_glow_c8_one_rank_of_8_emulated_steps20", [py, bench, "--full", "--force-gather", "--components", "1", "--steps", "20", "--warmup", "5",
                                                              "--cpu-seconds", "0", "--no-extra-legs", "--no-config-legs"]),
        ("miniboone_glow_c8_one_rank_of_8_emulated", [py, bench, "--full", "--force-gather", "--components", "1", "--cpu-seconds", "0",
                                                      "--no-extra-legs", "--no-config-legs"]),
    ]
    keep = ("metric", "value", "unit", "dtype", "ms_per_step", "steps", "config", "roofline", "cpu_baseline", "speedup_vs_cpu",
            "max_rel_err_vs_cpu", "numerics_guard", "data", "batch", "stream_launches_value", "forward_kernel_ms", "backward_kernels_ms",
            "timing", "library_ms_per_step", "library_weights_ms", "library_forward_ms", "library_backward_ms", "ms_per_step_gpu_events")
    legs = {}
    for name, cmd in jobs:
        t0 = time.perf_counter()
        if cmd[1] == bench:
            cmd = cmd + ["--full-record", os.path.join("gpurun_out", f"bench_leg_{name}.json")]
        try:
            proc = subprocess.run(cmd, stdout=subprocess.PIPE, stderr=subprocess.PIPE, text=True, timeout=240)
            lines = [l for l in proc.stdout.splitlines() if l.startswith("{")]
            if proc.returncode != 0 or not lines:
                legs[name] = {"error": f"rc {proc.returncode}: {proc.stderr.strip()[-300:]}"}
                continue
            j = json.loads(lines[-1])
            leg = {k: j[k] for k in keep if k in j}
            rl = leg.get("roofline")
            if isinstance(rl, dict):      # the fields a reader audits; the full line of each workload is under profiles/
                leg["roofline"] = {k: rl[k] for k in ("kernel", "bound", "achieved", "peak", "unit", "frac", "executed_frac", "traffic",
                                                       "launch_ms", "flops_per_launch", "hbm_algorithmic_bytes_per_launch") if k in rl}
            leg["wall_s"] = time.perf_counter() - t0
            legs[name] = leg
        except Exception as e:
            legs[name] = {"error": f"{type(e).__name__}: {e}"}
    return legs


def self_launch(args):
    """`python bench.py --gpus N` as the driver may invoke it: start the one-process-per-GPU job as a CHILD (this parent
    has not imported torch or touched the GPU, and never replaces itself) and relay rank 0's JSON line."""
    env = dict(os.environ)
    env.setdefault("HSA_ENABLE_IPC_MODE_LEGACY", "0")
    # --standalone: the launcher binds its own free rendezvous port on the loopback address (no pick-then-reuse race)
    cmd = [sys.executable, "-m", "torch.distributed.run", "--standalone", "--local-addr", "127.0.0.1", "--nnodes=1",
           f"--nproc-per-node={args.gpus}", os.path.abspath(__file__)] + sys.argv[1:]
    proc = subprocess.run(cmd, env=env, stdout=subprocess.PIPE, text=True)
    lines = [l for l in proc.stdout.splitlines() if l.startswith("{")]
    for l in proc.stdout.splitlines():
        if not l.startswith("{"):
            print(l, file=sys.stderr)
    if lines:
        print(lines[-1], flush=True)
    return proc.returncode if proc.returncode != 0 or lines else 1


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--gpus", type=int, default=1)
    ap.add_argument("--steps", type=int, default=4096)
    ap.add_argument("--warmup", type=int, default=64)
    ap.add_argument("--prewarm", type=float, default=0.3, help="untimed launches before the warm-up steps (clock ramp): 2000 steps per unit, i.e. about this many seconds on one GPU")
    ap.add_argument("--config", default="miniboone_glow", choices=sorted(CONFIGS))
    ap.add_argument("--batch", type=int, default=None)
    ap.add_argument("--components", type=int, default=None)
    ap.add_argument("--full", action="store_true",
                    help="measure more than the headline: the CPU baseline, the extra legs, the other BASELINE configurations, "
                         "21 repetitions of a short timed region, and the full record")
    ap.add_argument("--dump-outputs", metavar="DIR", default=None,
                    help="after the timed steps, write what the last timed step computed (G of its batch) as DIR/G.npy, float32")
    ap.add_argument("--cpu-seconds", type=float, default=12.0, help="budget of the CPU baseline leg of a --full run (0 = skip)")
    ap.add_argument("--math", default="default", choices=["default", "f32", "f16x3", "bf16x6"],
                    help="matrix path: default = chosen by the library per model (probe at create time)")
    ap.add_argument("--force-gather", action="store_true",
                    help="EMULATION aid: run the RCCL all-gather leg with one rank (with --components k: the per-rank load "
                         "of an 8/k-GPU run on one GPU; the cross-GPU hop itself is not exercised)")
    ap.add_argument("--group", type=int, default=GROUP, help=f"batches per launch / all-gather (default {GROUP}, max 32)")
    ap.add_argument("--full-record", default=FULL_RECORD, help="side file (relative to the repo) for the full record of a --full run: legs, notes, probes")
    ap.add_argument("--no-extra-legs", action="store_true", help="--full: skip the f32-exact and group-1 legs of the N=1 line")
    ap.add_argument("--no-config-legs", action="store_true", help="--full: skip legs.configs (the other BASELINE configurations, run as child processes)")
    ap.add_argument("--graph-exchange", action="store_true", help="sharded runs over real ranks: capture the group (RCCL all-gather included) into a HIP graph")
    ap.add_argument("--pipeline", default="auto", choices=["auto", "library", "torch"],
                    help="sharded runs: 'library' = RCCL called from libgbnf_hip.so, one HIP graph per group; 'torch' = the "
                         "torch.distributed all-gather on a second stream; 'auto' (default) = library for the one-rank emulation, "
                         "torch across real ranks (the library form has never run on more than one rank: ADVICE r4)")
    args = ap.parse_args()

    if args.gpus > 1 and "WORLD_SIZE" not in os.environ:
        sys.exit(self_launch(args))

    cfg_legs = None
    if (args.full and args.gpus == 1 and "WORLD_SIZE" not in os.environ and not args.no_extra_legs and not args.no_config_legs
            and args.config == "miniboone_glow" and args.components is None and args.batch is None and not args.force_gather):
        cfg_legs = config_legs(args)          # children first: this process has not touched the GPU yet

    # dmabuf IPC is the only form the host driver supports (without it RCCL fails with hipIpcGetMemHandle: invalid argument)
    os.environ.setdefault("HSA_ENABLE_IPC_MODE_LEGACY", "0")
    import numpy as np
    import torch
    import torch.distributed as dist
    from gbnf_amd import native, sharded, synth

    world = int(os.environ.get("WORLD_SIZE", "1"))
    rank = int(os.environ.get("RANK", "0"))
    local_rank = int(os.environ.get("LOCAL_RANK", "0"))
    if rank != 0:          # only rank 0 reports: nothing another rank (or a library it loads) writes may follow the JSON line
        os.dup2(os.open(os.devnull, os.O_WRONLY), 1)
    if world != args.gpus:
        raise SystemExit(f"--gpus {args.gpus} but WORLD_SIZE={world}")
    if not torch.cuda.is_available():
        raise SystemExit("bench.py needs an MI355X: there is no CPU fallback for the product path")
    torch.cuda.set_device(local_rank)
    dev = torch.device("cuda", local_rank)
    gather = world > 1 or args.force_gather
    if gather:
        if world > 1:
            os.environ.setdefault("MASTER_ADDR", "127.0.0.1")
            dist.init_process_group("nccl", device_id=dev)
        else:           # one rank: a file rendezvous (no port to collide on when two benches share a box)
            import tempfile
            rdzv = tempfile.NamedTemporaryFile(prefix="gbnf_bench_rdzv_", delete=False)
            rdzv.close()
            os.unlink(rdzv.name)
            dist.init_process_group("nccl", init_method=f"file://{rdzv.name}", rank=0, world_size=1, device_id=dev)

    kind, d, h, K, C_def, B_def = CONFIGS[args.config]
    C = args.components or C_def
    B = args.batch or B_def

    # identical bytes on every rank: synthetic inputs and weights from fixed seeds
    specs = synth.synth_boosted_specs(kind, C, d, h, K, seed=1)
    x_np = synth.synth_batch(B, d, seed=0)
    rho_np = np.maximum(1.0 / np.power(2.0, np.arange(C)), 0.05).astype(np.float32)   # "decreasing"
    parts = sharded.partition(C, world)
    c0, c1 = parts[rank]
    rho = torch.from_numpy(rho_np).to(dev)
    S = max(1, min(args.group, 32, args.steps))      # a run shorter than one group times one launch of that size
    if gather and args.steps >= 4 * S:
        # Sharded steady-state runs: a rank's launch should be a whole number of rounds of workgroups (512 slots x 128 rows
        # = 65536 row-components: two 4-wave workgroups per CU) -- a launch of 1.25 rounds takes as long as one of 1.5.
        # (A SHORT sharded run stays ONE group: measured at --steps 20, one component per rank, profiles/
        # r3_emulated_steps20_timeline.txt: 16 + 4 batches in two groups take 338 us against 240 us for one launch of 20 --
        # the host needs ~50 us per group for the RCCL call and the stream bookkeeping, which only a longer kernel hides.)
        fit = max(1, ROWS_PER_ROUND // (B * (c1 - c0)))
        if S > fit:
            S = S // fit * fit
    xs_np = [x_np] + [synth.synth_batch(B, d, seed=100 + s) for s in range(1, S)]   # S distinct resident batches
    xs = [torch.from_numpy(a).to(dev) for a in xs_np]

    def device_idle():
        """torch.cuda.synchronize(), on one stream with a busy wait in front: the runtime's blocking wait sleeps on an
        interrupt, and its wake-up (measured on this pool: 65 us typically, 250-730 us now and then) would sit inside the
        timed region (1.1 ms at the driver's 20 steps).  With the exchange stream in use the poll yields the core between
        queries (a tight poll from this thread slows the collective's own host threads down: 112 instead of 66 us, measured)."""
        if not os.environ.get("GBNF_BENCH_BLOCKING_SYNC"):
            evs = []
            for st in [torch.cuda.current_stream(dev)] + extra_streams:
                e = torch.cuda.Event()
                e.record(st)
                evs.append(e)
            if extra_streams:       # the collective's proxy thread needs the core now and then: yield between polls
                while not all(e.query() for e in evs):
                    os.sched_yield()
            else:
                while not evs[0].query():
                    pass
        torch.cuda.synchronize()

    extra_streams = []               # the pipelines' exchange streams (registered by timed_run)
    pipeline_used = {}               # which group pipeline the main run used (reported in the line)

    def barrier():
        device_idle()
        if world > 1:          # (one rank: nothing was enqueued since the device went idle -- a second wait would only add its host time to the timed region)
            dist.barrier()
            device_idle()

    MAX_TIMED_LAUNCHES = 48      # launches bracketed by timing events (the average is reported as roofline.launch_ms): event
                                 # pairs on every group of a long run cost the host more than the group's own launches

    def timed_run(math, group, steps, warmup, prewarm, want_gather_times=False, repetitions=0, fresh=False, graph_slots=False):
        """The pipeline on this rank's components in `math` mode, groups of `group` batches: returns timing + the handles' info."""
        flows = [native.NativeFlow(specs[c], math=math) for c in range(c0, c1)]
        mix = native.NativeMixture(flows)
        info = flows[0].info()
        # one group in the whole run: nothing to overlap the exchange with, so it stays on the kernel's stream (a cross-stream
        # event hand-over costs ~20 us of latency on this stack)
        pipe = None
        want_library = args.pipeline == "library" or (args.pipeline == "auto" and world == 1)
        # (the ranks agree inside native.Comm.from_torch_distributed -- a local probe on every rank, the flags meet in one all_reduce(MIN)
        #  before anything of the communicator set-up can block, and a refusal raises on EVERY rank: no second hand-shake here)
        # graph_slots (one rank, no exchange): every group as ONE HIP graph {flow launch, repair launch, recursion} on two alternating
        # streams -- what pays for SMALL groups, whose launches are as long as the gaps between them (one batch per launch: 62.3 against
        # 58.1 M samples/s, 640 batches, one box, alternating x 3; 2 and 4 batches per launch: 69.7 / 73.6 against 70.3 / 74.3 M -- no
        # gain from two batches on, so the headline's groups of 20 stay plain stream launches)
        if (gather and want_library) or (not gather and (args.pipeline == "library" or graph_slots)):
            # round 4: the exchange inside the library -- per group ONE hipGraphLaunch of {flow, repair, ncclAllGather, recursion}
            # (sharded.LibraryGroupPipeline); a refused communicator / capture falls back to the torch.distributed pipeline
            try:
                # the group as ONE HIP graph where that is proven on this stack: the single-rank emulation (captured and replayed in
                # the GPU tests).  Across real ranks the library issues the same launches and ncclAllGather directly, one call per
                # group (a multi-rank RCCL capture has never run on hardware available to this build: --graph-exchange opts in)
                use_graph = world == 1 or args.graph_exchange
                pipe = sharded.LibraryGroupPipeline(mix, C, c0, c1, rho, B, group, gather, graph=use_graph, overlap=steps > group)
                pipeline_used["kind"] = "library"
                pipeline_used["group_graph"] = bool(use_graph)
            except Exception as e:          # (GbnfError, ValueError, RuntimeError, OSError: every rank raises or none -- see Comm.from_torch_distributed)
                pipeline_used["fallback_reason"] = f"{type(e).__name__}: {e}"
                pipe = None
            if world > 1:
                # every rank or none: a rank that could not build the library pipeline takes all of them to the torch.distributed form
                # (two forms in one job would wait for each other's collectives forever)
                okt = torch.tensor([1 if pipe is not None else 0], dtype=torch.int32, device=dev)
                dist.all_reduce(okt, op=dist.ReduceOp.MIN)
                if pipe is not None and int(okt.item()) == 0:
                    pipeline_used["fallback_reason"] = "another rank could not build the library pipeline"
                    pipe = None
        if pipe is None:
            pipe = sharded.GroupPipeline(mix, C, c0, c1, rho, B, group, gather, overlap=steps > group)
            pipeline_used["kind"] = "torch.distributed" if gather else "single rank"
        for st_ in getattr(pipe, "streams", [pipe.post]):
            if st_ is not pipe.main and st_ not in extra_streams:
                extra_streams.append(st_)

        bound = {}                       # group size -> launches bound to the resident batches (host work outside the timed region)
        event_pool = [(torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)) for _ in range(MAX_TIMED_LAUNCHES)]

        def run(n_steps, events=None):
            done = gi = 0
            last = tail = None
            while done < n_steps:
                k = min(group, n_steps - done)
                if k not in bound and not fresh:
                    bound[k] = pipe.bind(xs[:k])
                ev = None
                if events is not None and k == group and len(events) < MAX_TIMED_LAUNCHES:
                    ev = event_pool[len(events)]
                    events.append(ev)
                # (fresh: the group's tensors are handed over as a new list every time -- the per-group host work of a caller whose
                #  batches come from a loader stays INSIDE the timed region: legs.fresh_batches)
                res = pipe.submit(list(xs[:k]) if fresh else bound[k], ev)
                if k == group:
                    last = res               # (G tensor of the slot, slot) of the last FULL group
                tail = (res[0], k)           # the last group submitted, full or not: its last batch is the run's last step
                done += k
                gi += 1
            return last, tail

        # clock settle phase (untimed, on top of the W warm-up steps, reported as "prewarm_s"): a cold MI355X runs the
        # first few hundred steps ~10 % slower while its clocks ramp up (a FIXED number of steps: every rank must issue
        # the same collectives)
        run(int(prewarm * 2000) // group * group)
        run(warmup)
        if steps % group:           # the timed loop ends on a partial group: bind and run that launch shape now (untimed), every rank alike
            run(steps % group)
        # --full: a run shorter than 4 groups is repeated (same K steps, each repetition between barriers + device
        # synchronisations, MAX over ranks per repetition): `value` comes from the MEDIAN repetition, so the driver's --steps 20
        # is not a sample of one ~1 ms launch (>= 20 timed iterations, median and min).  A plain run times K steps.
        reps = repetitions if repetitions else (21 if args.full and steps < 4 * group else 1)
        events = []
        if want_gather_times and gather:
            pipe.gather_events = []
        all_elapsed = []
        last_full = tail = None
        for rep in range(reps):
            barrier()
            t0 = time.perf_counter()
            last, tail = run(steps, events)
            barrier()
            all_elapsed.append(time.perf_counter() - t0)
            last_full = last if steps >= group else last_full
        if world > 1:
            t = torch.tensor(all_elapsed, dtype=torch.float64, device=dev)
            dist.all_reduce(t, op=dist.ReduceOp.MAX)
            all_elapsed = [float(v) for v in t.cpu()]
        elapsed = sorted(all_elapsed)[len(all_elapsed) // 2]
        per_launch = sorted(a.elapsed_time(b) for a, b in events)
        kern_ms = sum(per_launch) / max(1, len(per_launch))      # per full-group launch (flow launch + its repair launch)
        gather_us = None
        if pipe.gather_events:
            gather_us = 1e3 * sum(a.elapsed_time(b) for a, b in pipe.gather_events) / len(pipe.gather_events)
        # batch 0 of the last full group of the timed region (the tensor its submit returned)
        G0 = last_full[0][:B].cpu().numpy() if last_full is not None else None
        # G of the last timed step: the last batch of the last group (batch b of a group is rows [b*B, (b+1)*B) of its G)
        G_last = tail[0][(tail[1] - 1) * B: tail[1] * B].cpu().numpy() if tail is not None else None
        st = mix.numerics()              # the mode the mixture runs in NOW (a failed on-device check demotes f16x3 -> bf16x6)
        modes = [int(st.math_mode)]
        if world > 1:
            mt = torch.tensor([int(st.math_mode)], dtype=torch.int32, device=dev)
            ml = [torch.zeros_like(mt) for _ in range(world)]
            dist.all_gather(ml, mt)
            modes = [int(v.item()) for v in ml]
        return {"elapsed": elapsed, "elapsed_all": all_elapsed, "kern_ms": kern_ms, "info": info, "G0": G0, "G_last": G_last, "gather_us": gather_us,
                "modes": modes, "guard": {"checks": int(st.checks), "worst_rel_err": float(st.worst_rel_err),
                                          "demoted": bool(st.demoted), "tolerance": float(st.tolerance)},
                "kern_ms_min": per_launch[0] if per_launch else None,
                "kern_ms_median": per_launch[len(per_launch) // 2] if per_launch else None, "timed_launches": len(per_launch),
                "name": MATH_NAME[max(modes)] if len(set(modes)) == 1 else "mixed", "keep": (flows, mix, pipe)}

    def roofline(r, group):
        info, math = r["info"], (r["name"] if r["name"] != "mixed" else "bf16x6")     # ranks disagree: priced as the slower mode
        flops = 2.0 * info.macs_per_sample * (c1 - c0) * B * group            # one launch serves `group` batches
        achieved = flops / (r["kern_ms"] * 1e-3) / 1e12
        executed = achieved * info.padded_macs_per_sample / info.macs_per_sample * PRODUCTS[math]
        peak = F32_MFMA_PEAK_TFLOPS if math == "f32" else F16_MFMA_PEAK_TFLOPS
        alg_bytes = (4.0 * d + 4.0 * (c1 - c0)) * B * group                   # read x once, write ll per component
        return {
            "kernel": "gbnf::flow_kernel" if math == "f32" else "gbnf::flow_kernel_hx3",
            "bound": "mfma", "achieved": achieved, "peak": peak, "unit": "TFLOP/s", "frac": achieved / peak,
            "traffic": measured_traffic(args.config, B, C, group, math, world), "traffic_source": traffic_source(),
            "launch_ms": r["kern_ms"], "launch_ms_median": r["kern_ms_median"], "launch_ms_min": r["kern_ms_min"],
            "timed_launches": r["timed_launches"],
            # SURVEY 8(d) "flows only": the ll (C, N) tables without the recursion / exchange, from the launch times
            "flows_only_samples_per_s": B * group / (r["kern_ms"] * 1e-3) if r["kern_ms"] else None,
            "flops_per_launch": flops, "batches_per_launch": group,
            "executed_mfma_tflops": executed, "executed_frac": executed / peak,
            "vs_f32_mfma_peak": achieved / F32_MFMA_PEAK_TFLOPS,
            "hbm_algorithmic_bytes_per_launch": alg_bytes,
            "hbm_algorithmic_GBs": alg_bytes / (r["kern_ms"] * 1e-3) / 1e9,
            "hbm_frac": alg_bytes / (r["kern_ms"] * 1e-3) / 1e9 / HBM_PEAK_GBS,
        }

    main_run = timed_run(args.math, S, args.steps, args.warmup, args.prewarm, want_gather_times=True)
    ranks_seen = None
    if dist.is_initialized():
        seen = torch.zeros(world, dtype=torch.int32, device=dev)
        seen[rank] = 1 + torch.cuda.current_device()
        dist.all_reduce(seen)
        ranks_seen = [int(v) - 1 for v in seen.cpu()]       # local device index of every rank, -1 = a rank that did not answer

    if rank == 0 and args.dump_outputs and main_run["G_last"] is not None:
        G_last = main_run["G_last"].astype(np.float32)
        if G_last.nbytes > 64 << 20:        # the dump stays within 64 MB: a fixed, seeded sample of the rows
            G_last = G_last[np.sort(np.random.default_rng(0).choice(G_last.size, (64 << 20) // 4, replace=False))]
        os.makedirs(args.dump_outputs, exist_ok=True)
        np.save(os.path.join(args.dump_outputs, "G.npy"), G_last)

    if rank == 0:
        value = B * args.steps / main_run["elapsed"]
        math = main_run["name"]
        rl = roofline(main_run, S)
        if pipeline_used.get("kind") == "library":
            rl["kernel"] += " + exchange + recursion (library pipeline: the events bracket the whole group; the two slots' groups overlap)"
        rl["note"] = ("achieved = ALGORITHMIC f32 flops / launch time (HIP events around the launch); the split paths run "
                      "3x / 6x (+padding) that on the f16 pipe (executed_*). Measured model (profiles/r4_ubench_balance.txt, "
                      "r4_ablation_upper_bounds.txt): a SIMD spends 17.6 cycles per MFMA on the matrix pipe + weight-fragment "
                      "reads and ~0.5 cycle per issue cycle of vector work next to it (tanh + hi/mid split: 5 cycles per MFMA in "
                      "a hidden pass -> 20.0, a whole flow step's mix -> 22.2, layer 0 52.7), at 2, 3 or 4 waves per SIMD alike; "
                      "moving the weights (L2 -> LDS DMA 11 %, LDS -> register fragments 12 %) is the rest. Bias reads and the "
                      "stage barrier are worth 0.9 % / 0.5 % end to end. See DESIGN.md section 4")
        out = {
            "metric": "density-eval samples/sec, Boosted-Glow C=8 MINIBOONE d=43" if args.config == "miniboone_glow"
                      else f"density-eval samples/sec, {args.config}",
            "value": value, "unit": "samples/s", "n_gpus": world, "steps": args.steps, "warmup": args.warmup,
            "ms_per_step": 1e3 * main_run["elapsed"] / args.steps, "prewarm_s": args.prewarm, "higher_is_better": True,
            "timing": {"repetitions": len(main_run["elapsed_all"]), "value_from": "median repetition",
                       "elapsed_ms_median": 1e3 * main_run["elapsed"], "elapsed_ms_min": 1e3 * min(main_run["elapsed_all"]),
                       "elapsed_ms_max": 1e3 * max(main_run["elapsed_all"]),
                       "value_at_min": B * args.steps / min(main_run["elapsed_all"])},
            "numerics_guard": main_run["guard"], "math_modes_by_rank": [MATH_NAME[m] for m in main_run["modes"]],
            "scaling": "strong", "vs_baseline": None, "dtype": math, "data": "synthetic",
            "config": {"workload": f"{args.config}: d={d} h={h} K={K} C={C} batch={B}, x ~ N(0,1), synthetic weights",
                       "global_batch": B, "components": C, "math": MATH_TEXT.get(math, math), "group": S,
                       "group_note": f"{S} batches per flow launch / all-gather / recursion launch (same for every N)",
                       "parallelism": ("single GPU, all components in one launch" if world == 1 and not gather else
                                       f"components sharded {C // world}/GPU + one RCCL all-gather of ll per group"),
                       "emulated": bool(args.force_gather and world == 1)},
            "roofline": rl,
        }
        if gather:
            out["rccl"] = {"ranks_seen": ranks_seen, "allgather_us": main_run["gather_us"],
                           "allgather_bytes_per_rank": 4 * (c1 - c0) * S * B, "pipeline": dict(pipeline_used),
                           "graph_errors": list(getattr(main_run["keep"][2], "graph_errors", []))[:2],
                           "note": ("library pipeline: ncclAllGather is issued by libgbnf_hip.so inside the group's HIP graph; "
                                    "roofline.launch_ms brackets the WHOLE group (flow launch, exchange, recursion) on its slot's stream, "
                                    "and the two slots' groups overlap: launch_ms / achieved / flows_only_samples_per_s of this run are "
                                    "whole-group, overlapped times -- not the flow kernel alone (that is the N=1 line's roofline)")
                                   if pipeline_used.get("kind") == "library" else None}
        if args.full and world == 1 and not args.no_extra_legs:
            legs = {}
            n_leg = max(2 * S, min(args.steps, 320))
            try:
                r = timed_run("f32", S, n_leg, 2 * S, 0.0)
                rf = roofline(r, S)
                legs["f32_exact"] = {"value": B * n_leg / r["elapsed"], "unit": "samples/s", "dtype": "f32", "steps": n_leg,
                                     "launch_ms": r["kern_ms"], "achieved_tflops": rf["achieved"], "peak": rf["peak"],
                                     "frac": rf["frac"], "group": S}
                del r
            except native.GbnfError as e:
                legs["f32_exact"] = {"error": str(e)}
            try:       # the f32-faithful split mode (>= 24-bit operands, f32 range) on the same workload
                r = timed_run("bf16x6", S, n_leg, 2 * S, 0.0)
                rb = roofline(r, S)
                legs["bf16x6"] = {"value": B * n_leg / r["elapsed"], "unit": "samples/s", "dtype": "bf16x6", "steps": n_leg,
                                  "launch_ms": r["kern_ms"], "achieved_tflops": rb["achieved"], "peak": rb["peak"], "frac": rb["frac"],
                                  "executed_frac": rb["executed_frac"], "group": S}
                del r
            except native.GbnfError as e:
                legs["bf16x6"] = {"error": str(e)}
            if not gather:
                try:
                    # (both forms under the SAME conditions -- a short run on fresh handles without the clock-settle phase reads a few
                    #  percent below the headline whichever form it uses)
                    n_f = max(n_leg, 8 * S)
                    r = timed_run(args.math, S, n_f, 4 * S, 0.05, fresh=True)
                    rb_ = timed_run(args.math, S, n_f, 4 * S, 0.05)
                    legs["fresh_batches"] = {"value": B * n_f / r["elapsed"], "unit": "samples/s", "dtype": r["name"], "group": S, "steps": n_f,
                                             "bound_launches_same_conditions": B * n_f / rb_["elapsed"],
                                             "note": "the headline workload with every group submitted as a NEW list of batch tensors (no launches bound "
                                                     "ahead of the timed region): what a loader-fed caller of the group API pays per group -- 23 us of "
                                                     "host time per 20-batch group against 11 us bound, hidden behind the 1 ms the group runs"}
                    del r, rb_
                except Exception as e:
                    legs["fresh_batches"] = {"error": f"{type(e).__name__}: {e}"}
            # (at least 640 batches behind a short settle phase: at the driver's --steps 20 this leg used to time 40 launches -- 3 ms --
            #  straight after an idle device, and read 45 M samples/s where a second of the same calls runs at 58 M)
            n_g1 = max(n_leg, 640)
            r = timed_run(args.math, 1, n_g1, 64, 0.05, graph_slots=True)
            ms_batch = 1e3 * r["elapsed"] / n_g1
            flops_b = 2.0 * r["info"].macs_per_sample * C * B
            legs["group1"] = {"value": B * n_g1 / r["elapsed"], "unit": "samples/s", "dtype": r["name"], "steps": n_g1,
                              "launch_ms": r["kern_ms"], "ms_per_batch": ms_batch,
                              "achieved_tflops": flops_b / (ms_batch * 1e-3) / 1e12, "frac": flops_b / (ms_batch * 1e-3) / 1e12 / F16_MFMA_PEAK_TFLOPS,
                              "group": 1,
                              "note": "one batch per flow launch + one recursion launch (BASELINE's literal 'batch 4096' call), every batch a HIP graph "
                                      "{flow, repair, recursion} on one of two alternating streams: consecutive (independent) batches overlap. launch_ms "
                                      "brackets a whole batch on its slot (two slots overlap); frac = algorithmic FLOP per batch / ms_per_batch / peak"}
            del r
            try:
                # the reference's OWN batch sizes (density_experiment.py:80-81: 512 rows per training batch, 1024 per evaluation
                # batch), one log_prob call per batch: flow launch + its repair launch + recursion launch, plain stream launches
                flows_s = [native.NativeFlow(specs[c], math=args.math) for c in range(C)]
                mix_s = native.NativeMixture(flows_s)
                small = {}
                for nb in (512, 1024):
                    xb = xs[0][:nb].contiguous()
                    llb = torch.empty((C, nb), dtype=torch.float32, device=dev)
                    Gb = torch.empty(nb, dtype=torch.float32, device=dev)
                    for _ in range(20):
                        mix_s.log_prob(xb, rho, ll_out=llb, out=Gb)
                    torch.cuda.synchronize()
                    t0 = time.perf_counter()
                    for _ in range(300):
                        mix_s.log_prob(xb, rho, ll_out=llb, out=Gb)
                    torch.cuda.synchronize()
                    dt = (time.perf_counter() - t0) / 300
                    small[str(nb)] = {"value": nb / dt, "unit": "samples/s", "us_per_call": 1e6 * dt}
                legs["reference_batch_sizes"] = dict(small, note="one model.log_prob(x) call per batch of 512 / 1024 rows (the reference's "
                                                     "--batch_size / --eval_batch_size defaults): latency-bound, one wave's serial pass "
                                                     "through the flow; tools/bench_latency.py, profiles/r5_latency_small_batches.txt")
                del flows_s, mix_s
            except native.GbnfError as e:
                legs["reference_batch_sizes"] = {"error": str(e)}
            try:
                leg, G_mod = module_evaluate_leg(specs, kind, d, h, K, C, xs)
                if main_run["G0"] is not None:
                    g0 = main_run["G0"].astype(np.float64)
                    leg["max_rel_err_vs_pipeline"] = float(np.max(np.abs(G_mod.cpu().numpy() - g0) / np.maximum(np.abs(g0), 1.0)))
                legs["module_evaluate_loop"] = leg
            except Exception as e:                  # (a leg never takes the headline down)
                legs["module_evaluate_loop"] = {"error": f"{type(e).__name__}: {e}"}
            if cfg_legs is not None:
                legs["configs"] = cfg_legs
            out["legs"] = legs
        if args.full and args.cpu_seconds > 0 and world == 1:
            cb, G_cpu, n_cpu = cpu_baseline(specs, rho_np, x_np, args.cpu_seconds)
            out["cpu_baseline"] = cb
            out["speedup_vs_cpu"] = value / cb["value"]
            if main_run["G0"] is not None:
                err = float(np.max(np.abs(main_run["G0"][:n_cpu].astype(np.float64) - G_cpu) / np.maximum(np.abs(G_cpu), 1.0)))
                out["max_rel_err_vs_cpu"] = err
        elif args.cpu_seconds > 0:
            out["cpu_baseline"] = None     # reported on the N=1 --full run only
        if args.full:
            emit_full_record(out, args.full_record)
        line = compact_line(out, args.full_record if args.full else None)
    else:
        line = None

    # RCCL writes a version banner to (C-level, buffered) stdout: tear the process group down and flush that buffer first,
    # so that the JSON line is the LAST line on stdout
    if dist.is_initialized():
        dist.barrier()
        dist.destroy_process_group()
    sys.stdout.flush()
    try:
        ctypes.CDLL(None).fflush(None)       # ... its banner sits in the C library's stdout buffer until then
    except OSError:
        pass
    if line is not None:
        print(line, flush=True)


if __name__ == "__main__":
    main()
