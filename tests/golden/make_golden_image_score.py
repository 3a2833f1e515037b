#!/usr/bin/env python3
"""Generate the g24 fixtures (tests/golden/image_score/): the REFERENCE's own input gradient of one image Glow component.

Run in the build container only (needs the reference, torch CPU), like make_golden_image_grads.py whose three configurations,
x, noise and parameters (the g21 files) it reuses:

    PYTHONDONTWRITEBYTECODE=1 python tests/golden/make_golden_image_score.py

For each g21 file it builds the reference's BoostedFlow of that configuration, loads the file's state_dict and permutations, runs
``model(x=x, components=0)`` with ``x.requires_grad_(True)`` and the file's dequantisation noise injected, and stores
``d sum_i ll_i / d x`` with ``ll = log_normal_diag(z, z_mu, z_var) + logdet`` (image_experiment.py:227) as ``gx`` next to ``ll``.
Only data is committed.
"""
import json
import os
import sys

sys.dont_write_bytecode = True
HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, HERE)
sys.path.insert(0, os.path.dirname(HERE))

import numpy as np  # noqa: E402
import torch  # noqa: E402

import make_golden as mg  # noqa: E402  (puts the repository and the reference on sys.path)
import image_grad_oracle as igo  # noqa: E402


def score_case(g21_name):
    from models.glow import FlowStep
    from utils.distributions import log_normal_diag
    cfg, data = igo.g21_load(g21_name)
    a = mg.ref_args("glow", int(np.prod(cfg["input_size"])), cfg["h"], cfg["K"], 1, depth=cfg["depth"], coupling=cfg["coupling"],
                    permutation=cfg["permutation"])
    a.input_size = list(cfg["input_size"]); a.num_blocks = cfg["L"]; a.learn_top = cfg["learn_top"]; a.LU_decomposed = cfg["LU"]
    torch.manual_seed(7)
    model = mg.RefBoostedFlow(a)
    comp = model.flows[0]
    comp.load_state_dict({k[len("param."):]: torch.from_numpy(data[k]) for k in data.files if k.startswith("param.")})
    k = 0
    for layer in comp.flow.layers:
        if isinstance(layer, FlowStep):
            if not hasattr(layer, "invconv"):
                pm = layer.shuffle if hasattr(layer, "shuffle") else layer.reverse
                pm.indices = torch.from_numpy(data[f"perm.{k}"]).long()
                for i in range(pm.num_dim):
                    pm.indices_inverse[pm.indices[i]] = i
            k += 1
    for m in comp.modules():
        if hasattr(m, "inited"):
            m.inited = True
    model.train()
    orig = torch.Tensor.uniform_
    noise_t = torch.from_numpy(data["noise"])

    def injected(self, a=0.0, b=1.0):
        self.copy_(noise_t)
        return self
    x = torch.from_numpy(data["x"]).clone().requires_grad_(True)
    try:
        torch.Tensor.uniform_ = injected
        z, mu, var, ldj, _ = model(x=x, components=0)
    finally:
        torch.Tensor.uniform_ = orig
    assert np.abs(z.detach().numpy() - data["z"]).max() == 0.0, "the g21 forward is not reproduced"
    ll = log_normal_diag(z, mu, var, dim=[1, 2, 3]) + ldj
    ll.sum().backward()
    name = g21_name.replace("g21_image_grads", "g24_image_score")
    out = dict(config=np.frombuffer(json.dumps(dict(case="image_score", g21=g21_name)).encode(), dtype=np.uint8),
               ll=ll.detach().numpy().copy(), gx=x.grad.numpy().copy())
    os.makedirs(os.path.join(HERE, "image_score"), exist_ok=True)
    path = os.path.join(HERE, "image_score", name + ".npz")
    np.savez_compressed(path, **out)
    print(f"{name}: max|gx|={np.abs(out['gx']).max():.4f} {os.path.getsize(path)} bytes")


def main():
    for name in igo.G21:
        score_case(name)


if __name__ == "__main__":
    main()
