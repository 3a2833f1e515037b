"""Shared by tests/test_hip_image_actnorm_init.py (GPU) and tests/test_image_actnorm_init_host.py (CPU): the synthetic geometries the
g20 fixtures lack, for the one-pass ActNorm2d initialisation (gbnf_image_trainer_actnorm_init), and their float64 oracle answers.

Each case is the smallest shape at which its path can go wrong (model seed 11, batch seed 3, every an_bias / an_logs zeroed):
  1x28x20      14x10 and 7x5 maps in the corner of 16- and 8-wide storage, Permute2d steps, additive coupling
  3x32x32_L3   a 4x4 map in 8-wide storage, a 48-channel third level
  1x28x28_d0   coupling_network_depth 0: one ActNorm'd convolution per net; a reversing permutation; one level
  3x32x32_d2   depth 2: three ActNorm'd convolutions per net, hidden width (48) not a multiple of 32
  1x28x28_h272 more than 256 hidden channels, a batch of one image
"""
import copy

import numpy as np

CASES = {
    "1x28x20": ((1, 28, 20), 3, dict(L=2, K=2, h=32, coupling="additive", permutation="shuffle")),
    "3x32x32_L3": ((3, 32, 32), 2, dict(L=3, K=2, h=32)),
    "1x28x28_d0": ((1, 28, 28), 3, dict(L=1, K=2, h=64, depth=0, permutation="reverse")),
    "3x32x32_d2": ((3, 32, 32), 2, dict(L=2, K=1, h=48, depth=2)),
    "1x28x28_h272": ((1, 28, 28), 1, dict(L=2, K=1, h=272)),
}
MODEL_SEED, BATCH_SEED = 11, 3
BAR = 1e-5            # |bias - ref|, |logs - ref| <= BAR * max(1, max|ref|): the bar of test_image_actnorm_data_init_matches_reference
MARGIN = 1e-6         # the float32 oracle stays this close to the float64 one on every case (checked on the host): BAR is 10x that


def zeroed(spec):
    """A deep copy of an image flow spec with every ActNorm2d (the steps' own, the ones behind the nets' Conv2d layers) at zero."""
    spec = copy.deepcopy(spec)
    for lv in spec["levels"]:
        for st in lv["steps"]:
            st["an_bias"], st["an_logs"] = np.zeros_like(st["an_bias"]), np.zeros_like(st["an_logs"])
            for c in st["convs"]:
                if c["an_bias"] is not None:
                    c["an_bias"], c["an_logs"] = np.zeros_like(c["an_bias"]), np.zeros_like(c["an_logs"])
    return spec


def make(name, n=None):
    """-> (spec with the ActNorm2d arrays zeroed, x, noise) of a listed case; ``n`` overrides the batch size."""
    from gbnf_amd import synth
    size, n0, kw = CASES[name]
    spec = zeroed(synth.synth_image_glow_spec(size, seed=MODEL_SEED, **kw))
    x, noise = synth.synth_image_batch(n0 if n is None else n, size, seed=BATCH_SEED)
    return spec, x, noise


_cache = {}


def oracle_init(name, dtype_name="float64", n=None, scale=1.0):
    """-> (the spec after oracle.image_actnorm_init, [(bias, logs) per ActNorm2d in module order]); computed once, shared, not to be
    modified."""
    import torch
    from oracle import gbnf_oracle as oracle
    key = (name, dtype_name, n, scale)
    if key not in _cache:
        spec, x, noise = make(name, n)
        _cache[key] = (spec, oracle.image_actnorm_init(spec, x, noise, scale=scale, dtype=getattr(torch, dtype_name)))
    return _cache[key]


def worst(got, ref):
    """max over the layers of |got - ref| / max(1, max|ref|), bias and logs alike.  got, ref: [(bias, logs)] in module order."""
    assert len(got) == len(ref)
    w = 0.0
    for (gb, gl), (rb, rl) in zip(got, ref):
        for g, r in ((gb, rb), (gl, rl)):
            g, r = np.asarray(g, dtype=np.float64).reshape(-1), np.asarray(r, dtype=np.float64).reshape(-1)
            assert g.shape == r.shape and np.all(np.isfinite(g))
            w = max(w, float(np.abs(g - r).max()) / max(1.0, float(np.abs(r).max())))
    return w


def spec_actnorms(spec):
    """[(bias, logs)] of a spec (numpy arrays or tensors) in module order."""
    out = []
    for lv in spec["levels"]:
        for st in lv["steps"]:
            out.append((st["an_bias"], st["an_logs"]))
            out += [(c["an_bias"], c["an_logs"]) for c in st["convs"] if c["an_bias"] is not None]
    return out
