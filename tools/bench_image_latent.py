#!/usr/bin/env python3
"""Full-latent direction of the image path: images/s of forward, encode (forward + the Split2d halves stored) and encode + inverse
(the round trip), CIFAR-shaped Boosted-Glow C = 4 (K = 8, L = 2, h = 256), all components one after the other on one stream, plain
stream launches, device events around each repeat.  Prints one JSON line.

    python tools/bench_image_latent.py [--batch 256 --components 4 --steps 20 --warmup 3 --repeats 5]
"""
import argparse
import json
import os
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

import torch


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--batch", type=int, default=256)
    ap.add_argument("--components", type=int, default=4)
    ap.add_argument("--K", type=int, default=8)
    ap.add_argument("--L", type=int, default=2)
    ap.add_argument("--hidden", type=int, default=256)
    ap.add_argument("--input", type=int, nargs=3, default=[3, 32, 32], metavar=("C", "H", "W"))
    ap.add_argument("--steps", type=int, default=20)
    ap.add_argument("--warmup", type=int, default=3)
    ap.add_argument("--repeats", type=int, default=5, help="timed windows per call; the legs alternate inside a repeat")
    a = ap.parse_args()
    from gbnf_amd import native, synth
    if not torch.cuda.is_available():
        raise SystemExit("bench_image_latent.py needs the GPU: a CPU run measures nothing")
    dev = torch.device("cuda:0")
    size = tuple(a.input)
    flows = [native.NativeImageFlow(synth.synth_image_glow_spec(size, a.hidden, a.K, a.L, seed=100 + c)) for c in range(a.components)]
    x_np, noise_np = synth.synth_image_batch(a.batch, size, seed=0)
    x, noise = torch.from_numpy(x_np).to(dev), torch.from_numpy(noise_np).to(dev)

    def forward():
        for f in flows:
            f.forward(x, noise)

    def encode():
        for f in flows:
            f.encode(x, noise)

    def round_trip():
        for f in flows:
            z, eps, _, _ = f.encode(x, noise)
            f.inverse(z, eps, 1.0)

    legs = {"forward": forward, "encode": encode, "encode+inverse": round_trip}
    for fn in legs.values():
        for _ in range(a.warmup):
            fn()
    torch.cuda.synchronize()
    rates = {k: [] for k in legs}
    for _ in range(a.repeats):
        for name, fn in legs.items():
            ev0, ev1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
            ev0.record()
            for _ in range(a.steps):
                fn()
            ev1.record()
            torch.cuda.synchronize()
            rates[name].append(a.batch / (ev0.elapsed_time(ev1) * 1e-3 / a.steps))
    u = (255.0 * x + noise) / 256.0
    z, eps, _, _ = flows[0].encode(x, noise)
    err = float((flows[0].inverse(z, eps, 1.0) - u).abs().max())
    med = lambda v: sorted(v)[len(v) // 2]
    print(json.dumps({
        "metric": f"images/s through all {a.components} components, {size[0]}x{size[1]}x{size[2]} Boosted-Glow", "unit": "images/s",
        "config": {"batch": a.batch, "components": a.components, "K": a.K, "L": a.L, "hidden": a.hidden, "steps": a.steps,
                   "repeats": a.repeats, "launch": "stream launches, one stream"},
        **{name: {"median": med(v), "min": min(v), "max": max(v)} for name, v in rates.items()},
        "encode_over_forward": med(rates["encode"]) / med(rates["forward"]),
        "round_trip_max_abs_err": err}))


if __name__ == "__main__":
    main()
