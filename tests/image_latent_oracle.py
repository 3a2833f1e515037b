"""Test-only yardstick of the full-latent direction x -> (z, eps) of an image Glow component (gbnf_image_flow_encode):
``oracle.image_component_forward`` with the half each Split2d level drops KEPT, standardised --
eps_l = (z2 - mean) * exp(-log-var) with (mean, log-var) = split_prior(z1) (models/layers.py:689-703), the algebraic inverse of
Split2d's reverse at temperature 1 (models/layers.py:695-699: z2 = mean + exp(log-var) * temperature * eps).  Built from the
oracle's own image_squeeze / image_flow_step / image_conv, float64 unless told otherwise."""
import math

import numpy as np
import torch

from oracle import gbnf_oracle as oracle


def encode(spec, x, noise=None, dtype=torch.float64):
    """-> (z (N,Cz,Hz,Wz), [eps_l (N, C_l/2, H_l, W_l), first level first], ldj (N,), u (N,C,H,W) = (255 x + noise) / 256), numpy."""
    x = oracle._t(x, dtype).clone()
    B, C, H, W = x.shape
    u = (255.0 * x + (oracle._t(noise, dtype) if noise is not None else 0.0)) / 256.0
    ld = torch.full((B,), -math.log(256.0) * C * H * W, dtype=dtype)
    bounds = torch.tensor(spec["bounds"], dtype=dtype)
    v = ((u * 2.0 - 1.0) * bounds + 1.0) / 2.0
    logit = torch.log(v) - torch.log(1.0 - v)
    sp = torch.nn.functional.softplus
    ld = ld + (sp(logit) + sp(-logit) - sp((1.0 - bounds).log() - bounds.log())).flatten(1).sum(-1)
    z, eps = logit, []
    for lvl in spec["levels"]:
        z = oracle.image_squeeze(z)
        for st in lvl["steps"]:
            z, ld = oracle.image_flow_step(spec, st, z, ld, dtype)
        if lvl["split"] is not None:
            Cz = z.shape[1]
            z1, z2 = z[:, : Cz // 2], z[:, Cz // 2:]
            hh = oracle.image_conv(lvl["split"], z1, dtype)
            mu, lv = hh[:, 0::2], hh[:, 1::2]
            ld = ld + (-0.5 * (lv + (z2 - mu) ** 2 * torch.exp(-lv))).sum(dim=[1, 2, 3])
            eps.append(((z2 - mu) * torch.exp(-lv)).numpy())
            z = z1
    return z.numpy(), eps, ld.numpy(), u.numpy()


# the geometries both test files cover: (input size, synth_image_glow_spec keywords)
GEOMETRIES = {
    "3x32x32_L2": ((3, 32, 32), dict(h=32, K=2, L=2)),                       # the fused split-f16 path
    "3x32x32_L3": ((3, 32, 32), dict(h=32, K=2, L=3)),                       # two Split2d levels, the 4 x 4 map in 8-wide storage
    "1x28x28_L2": ((1, 28, 28), dict(h=16, K=2, L=2)),                       # the 14 x 14 map in 16-wide storage
    "1x28x20_add_shuffle": ((1, 28, 20), dict(h=16, K=2, L=2, coupling="additive", permutation="shuffle")),   # non-square small map
    "3x32x32_depth2": ((3, 32, 32), dict(h=32, K=2, L=2, depth=2)),          # (exact-f32 convolutions where the fused kernel is not built)
}


def geometry(name, n, seed=21):
    from gbnf_amd import synth
    size, kw = GEOMETRIES[name]
    sp = synth.synth_image_glow_spec(size, seed=seed, **kw)
    x, noise = synth.synth_image_batch(n, size, seed=seed + 1)
    return sp, size, x, noise


def max_abs(a, b):
    a, b = np.asarray(a, dtype=np.float64), np.asarray(b, dtype=np.float64)
    return float(np.abs(a - b).max()) if a.size else 0.0
