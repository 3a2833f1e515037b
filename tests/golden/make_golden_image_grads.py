#!/usr/bin/env python3
"""Generate the g21 fixtures (tests/golden/image_grads/): the REFERENCE's own parameter gradients of one image Glow component.

Run in the build container only (needs the reference, torch CPU), like make_golden.py whose helpers it reuses:

    PYTHONDONTWRITEBYTECODE=1 python tests/golden/make_golden_image_grads.py

For each case it builds the reference's BoostedFlow with ONE image component (input [1,16,16], h = 32, K = 2, L = 2), installs the
parameters of gbnf_amd.synth (an LU case keeps the reference's own factors), runs ``model(x=x, components=0)`` in train mode with the
fixture's dequantisation noise injected, and ``nll = -mean(log_normal_diag(z, z_mu, z_var) + logdet)`` (image_experiment.py:227,
:398-419), ``nll.backward()``.  Stored: config and seeds, x, noise, z, ldj, nll, the component's state_dict (``param.<name>``), the
permutations (``perm.<k>``) and every parameter's gradient (``grad.<name>``), keyed by state_dict name.  Only data is committed.
The kink margin (no ReLU pre-activation within 1e-5 max|y| of zero in float64; tests/image_grad_oracle.py) is asserted before writing.
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
from gbnf_amd import synth  # noqa: E402

INPUT, H, K, L, N = (1, 16, 16), 32, 2, 2, 3


def grads_case(name, seed, coupling="affine", permutation="invconv", LU=False, depth=1, learn_top=True):
    """``seed``: the first of seed, seed + 1, ... whose synthetic case is clear of the kink margin is used (and recorded)."""
    from utils.distributions import log_normal_diag
    kw = dict(depth=depth, coupling=coupling, permutation=permutation, learn_top=learn_top)
    if not LU:          # (an LU case's 1x1 matrices are the reference's own: checked below, after they are installed)
        seed = next(s for s in range(seed, seed + 40)
                    if all(inside == 0 for inside, _ in igo.kink_report(synth.synth_image_glow_spec(INPUT, H, K, L, seed=s, **kw),
                                                                        *synth.synth_image_batch(N, INPUT, seed=100 + s))))
    a = mg.ref_args("glow", int(np.prod(INPUT)), H, K, 1, depth=depth, coupling=coupling, permutation=permutation)
    a.input_size = list(INPUT); a.num_blocks = L; a.learn_top = learn_top; a.LU_decomposed = LU
    torch.manual_seed(7)
    model = mg.RefBoostedFlow(a)
    sp = synth.synth_image_glow_spec(INPUT, H, K, L, depth=depth, coupling=coupling, permutation=permutation, learn_top=learn_top, seed=seed)
    mg.install_image_spec(model.flows[0], sp, keep_invconv=LU)
    x, noise = synth.synth_image_batch(N, INPUT, seed=100 + seed)
    rows = igo.kink_report(sp, x, noise)
    assert rows and all(inside == 0 for inside, _ in rows), f"{name}: seed {seed} has a ReLU unit inside the kink margin: {rows}"
    model.train()
    orig = torch.Tensor.uniform_
    noise_t = torch.from_numpy(noise)

    def injected(self, a=0.0, b=1.0):
        self.copy_(noise_t)
        return self
    try:
        torch.Tensor.uniform_ = injected
        z, mu, var, ldj, _ = model(x=torch.from_numpy(x).clone(), components=0)
    finally:
        torch.Tensor.uniform_ = orig
    nll = -(log_normal_diag(z, mu, var, dim=[1, 2, 3]) + ldj).mean()
    nll.backward()
    out = dict(config=np.frombuffer(json.dumps(dict(case="image_grads", h=H, K=K, L=L, N=N, depth=depth, coupling=coupling,
                                                    permutation=permutation, learn_top=learn_top, LU=LU, w_seed=seed, x_seed=100 + seed,
                                                    input_size=list(INPUT))).encode(), dtype=np.uint8),
               x=x, noise=noise, z=z.detach().numpy().copy(), ldj=ldj.detach().numpy().copy(), nll=np.float64(nll.item()))
    comp = model.flows[0]
    for k, v in comp.state_dict().items():
        out["param." + k] = v.detach().numpy().copy()
    for k, p in comp.named_parameters():
        out["grad." + k] = (p.grad if p.grad is not None else torch.zeros_like(p)).numpy().copy()
    k = 0
    for lv in sp["levels"]:
        for st in lv["steps"]:
            if st["perm"] is not None:
                out[f"perm.{k}"] = np.asarray(st["perm"], dtype=np.int64)
            k += 1
    os.makedirs(os.path.join(HERE, "image_grads"), exist_ok=True)
    path = os.path.join(HERE, "image_grads", name + ".npz")       # (a directory of their own: the generic fixture tests take every tests/golden/*.npz for a tabular case)
    np.savez_compressed(path, **out)
    print(f"{name}: nll={nll.item():.6f} {os.path.getsize(path)} bytes, {sum(1 for q in out if q.startswith('grad.'))} gradients")


def main():
    grads_case("g21_image_grads_invconv_affine", seed=1)
    grads_case("g21_image_grads_lu", seed=1, LU=True)
    grads_case("g21_image_grads_shuffle_additive", seed=1, coupling="additive", permutation="shuffle", learn_top=False, depth=2)


if __name__ == "__main__":
    main()
