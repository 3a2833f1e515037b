#!/usr/bin/env python3
"""Generate the g22 fixtures (tests/golden/image_ycond/): the REFERENCE's own class-conditional image Glow component.

Run in the build container only (needs the reference, torch CPU), like make_golden_image_grads.py whose recipe it follows:

    PYTHONDONTWRITEBYTECODE=1 python tests/golden/make_golden_image_ycond.py

For each case it builds the reference's BoostedFlow with ONE image component and ``y_condition`` (input [1,16,16], h = 32, K = 2,
L = 2), installs the parameters of gbnf_amd.synth -- ``synth_ycond`` for project_ycond / project_class, which the reference starts at
zero; an LU case keeps the reference's own factors --, and runs the COMPONENT, ``model.flows[0](x=x, y_onehot=y)``, in train mode with
the fixture's dequantisation noise injected (the boosted wrapper drops y_onehot, models/boosted_flow.py:222).  The loss is the
reference's compute_loss (image_experiment.py:223-244, cross_entropy branch): bpd = mean(nll) / (ln 2 * C H W),
total = bpd + 0.01 * cross_entropy(y_logits, argmax y); ``total.backward()``.  Stored: config and seeds, x, noise, y, z, z_mu, z_var,
ldj, y_logits, nll, loss_classes, total, the component's state_dict (``param.<name>``), the permutations (``perm.<k>``) and every
parameter's gradient (``grad.<name>``), keyed by state_dict name.  Only data is committed.  The kink margin (no ReLU pre-activation
within 1e-5 max|y| of zero in float64; tests/image_grad_oracle.py) is asserted before writing.
"""
import json
import math
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
import image_ycond_oracle as iyo  # noqa: E402
from gbnf_amd import synth  # noqa: E402

INPUT, H, K, L = (1, 16, 16), 32, 2, 2
Y_WEIGHT = 0.01


def ycond_case(name, seed, Y, N, coupling="affine", permutation="invconv", LU=False, depth=1, learn_top=True, soft_row=None,
               repeat_class=False):
    """``seed``: the first of seed, seed + 1, ... whose synthetic case is clear of the kink margin is used (and recorded)."""
    from utils.distributions import log_normal_diag
    kw = dict(depth=depth, coupling=coupling, permutation=permutation, learn_top=learn_top)
    if not LU:
        seed = next(s for s in range(seed, seed + 40)
                    if all(inside == 0 for inside, _ in igo.kink_report(synth.synth_image_glow_spec(INPUT, H, K, L, seed=s, **kw),
                                                                        *synth.synth_image_batch(N, INPUT, seed=100 + s))))
    a = mg.ref_args("glow", int(np.prod(INPUT)), H, K, 1, depth=depth, coupling=coupling, permutation=permutation)
    a.input_size = list(INPUT); a.num_blocks = L; a.learn_top = learn_top; a.LU_decomposed = LU
    a.y_condition = True; a.y_classes = Y
    torch.manual_seed(7)
    model = mg.RefBoostedFlow(a)
    comp = model.flows[0]
    sp = synth.synth_image_glow_spec(INPUT, H, K, L, depth=depth, coupling=coupling, permutation=permutation, learn_top=learn_top, seed=seed,
                                     y_classes=Y)
    mg.install_image_spec(comp, sp, keep_invconv=LU)
    with torch.no_grad():
        for lin, pre in ((comp.project_ycond, "cond"), (comp.project_class, "class")):
            lin.linear.weight.copy_(torch.from_numpy(sp["ycond"][pre + "_w"]))
            lin.linear.bias.copy_(torch.from_numpy(sp["ycond"][pre + "_b"]))
            lin.logs.copy_(torch.from_numpy(sp["ycond"][pre + "_logs"]))
    x, noise = synth.synth_image_batch(N, INPUT, seed=100 + seed)
    y = iyo.synth_y(N, Y, seed, soft_row=soft_row)
    if repeat_class:                                   # two rows of one class
        y[1] = y[0]
    t = np.argmax(y, axis=1)
    if soft_row is not None:
        srt = np.sort(y[soft_row])
        assert srt[-1] > srt[-2] and abs(y[soft_row].sum() - 1.0) < 1e-5 and (y[soft_row] > 0).all(), "the soft row must have no tie"
    if repeat_class:
        assert len(set(t.tolist())) < N
    rows = igo.kink_report(sp, x, noise)
    assert rows and all(inside == 0 for inside, _ in rows), f"{name}: seed {seed} has a ReLU unit inside the kink margin: {rows}"
    model.train()
    orig = torch.Tensor.uniform_
    noise_t = torch.from_numpy(noise)

    def injected(self, a=0.0, b=1.0):
        self.copy_(noise_t)
        return self
    y_t = torch.from_numpy(y)
    try:
        torch.Tensor.uniform_ = injected
        z, mu, var, ldj, y_logits = comp(x=torch.from_numpy(x).clone(), y_onehot=y_t)
    finally:
        torch.Tensor.uniform_ = orig
    nll_i = -(log_normal_diag(z, mu, var, dim=[1, 2, 3]) + ldj)
    bpd = (nll_i / (math.log(2.0) * float(np.prod(INPUT)))).mean()
    loss_classes = torch.nn.functional.cross_entropy(y_logits, torch.argmax(y_t, dim=1), reduction="mean")
    total = bpd + Y_WEIGHT * loss_classes
    total.backward()
    out = dict(config=np.frombuffer(json.dumps(dict(case="image_ycond", h=H, K=K, L=L, N=N, Y=Y, depth=depth, coupling=coupling,
                                                    permutation=permutation, learn_top=learn_top, LU=LU, w_seed=seed, x_seed=100 + seed,
                                                    y_weight=Y_WEIGHT, input_size=list(INPUT))).encode(), dtype=np.uint8),
               x=x, noise=noise, y=y, z=z.detach().numpy().copy(), z_mu=mu.detach().numpy().copy(), z_var=var.detach().numpy().copy(),
               ldj=ldj.detach().numpy().copy(), y_logits=y_logits.detach().numpy().copy(), nll=np.float64(nll_i.mean().item()),
               loss_classes=np.float64(loss_classes.item()), total=np.float64(total.item()))
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
    os.makedirs(os.path.join(HERE, "image_ycond"), exist_ok=True)
    path = os.path.join(HERE, "image_ycond", name + ".npz")       # (a directory of their own: the generic fixture tests take every tests/golden/*.npz for a tabular case)
    np.savez_compressed(path, **out)
    print(f"{name}: nll={nll_i.mean().item():.6f} ce={loss_classes.item():.6f} {os.path.getsize(path)} bytes, "
          f"{sum(1 for q in out if q.startswith('grad.'))} gradients")


def main():
    ycond_case("g22_image_ycond_invconv_affine", seed=1, Y=10, N=3)
    ycond_case("g22_image_ycond_lu", seed=1, Y=10, N=3, LU=True)
    ycond_case("g22_image_ycond_shuffle_additive", seed=1, Y=3, N=5, coupling="additive", permutation="shuffle", learn_top=False, depth=2,
               soft_row=2, repeat_class=True)


if __name__ == "__main__":
    main()
