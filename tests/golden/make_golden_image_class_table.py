#!/usr/bin/env python3
"""Generate the g23 fixture (tests/golden/image_ycond/g23_image_class_table.npz): the REFERENCE's own class-conditional image Glow
component evaluated under EVERY class.

Run in the build container only (needs the reference, torch CPU), like make_golden_image_ycond.py whose recipe it follows:

    PYTHONDONTWRITEBYTECODE=1 python tests/golden/make_golden_image_class_table.py

It builds the reference's BoostedFlow with one image component and ``y_condition`` the way make_golden_image_ycond.py does for
g22_image_ycond_invconv_affine, loads the parameters that fixture stores (``param.<name>``), and for every class k runs the COMPONENT
``model.flows[0](x=x, y_onehot=e_k)`` on the fixture's x with its dequantisation noise injected.  Stored: the name of the source fixture
and ``table`` (n, Y) float64 = log_normal_diag(z, z_mu, z_var, dim=[1,2,3]) + logdet (image_experiment.py:227) -- the log-density of
every image under every class, the reference's float32 arithmetic.  The diagonal under the fixture's own labels must reproduce its
``nll``; that is asserted before writing.  Only data is committed.
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
import image_ycond_oracle as iyo  # noqa: E402
from gbnf_amd import synth  # noqa: E402

SOURCE = "g22_image_ycond_invconv_affine"
NAME = "g23_image_class_table"


def main():
    from utils.distributions import log_normal_diag
    cfg, data = iyo.g22_load(SOURCE)
    size, Y = tuple(cfg["input_size"]), cfg["Y"]
    a = mg.ref_args("glow", int(np.prod(size)), cfg["h"], cfg["K"], 1, depth=cfg["depth"], coupling=cfg["coupling"],
                    permutation=cfg["permutation"])
    a.input_size = list(size); a.num_blocks = cfg["L"]; a.learn_top = cfg["learn_top"]; a.LU_decomposed = cfg["LU"]
    a.y_condition = True; a.y_classes = Y
    torch.manual_seed(7)
    model = mg.RefBoostedFlow(a)
    comp = model.flows[0]
    # (install_image_spec marks every ActNorm2d initialised; the values then come from the fixture)
    mg.install_image_spec(comp, synth.synth_image_glow_spec(size, cfg["h"], cfg["K"], cfg["L"], depth=cfg["depth"], coupling=cfg["coupling"],
                                                            permutation=cfg["permutation"], learn_top=cfg["learn_top"], seed=cfg["w_seed"],
                                                            y_classes=Y))
    comp.load_state_dict({k[len("param."):]: torch.from_numpy(data[k]) for k in data.files if k.startswith("param.")})
    x, noise, y = data["x"], data["noise"], data["y"]
    n = x.shape[0]
    model.train()
    orig = torch.Tensor.uniform_
    noise_t = torch.from_numpy(noise)

    def injected(self, a=0.0, b=1.0):
        self.copy_(noise_t)
        return self

    table = np.zeros((n, Y), dtype=np.float64)
    try:
        torch.Tensor.uniform_ = injected
        with torch.no_grad():
            for k in range(Y):
                e_k = torch.zeros((n, Y), dtype=torch.float32)
                e_k[:, k] = 1.0
                z, mu, var, ldj, _ = comp(x=torch.from_numpy(x).clone(), y_onehot=e_k)
                table[:, k] = (log_normal_diag(z, mu, var, dim=[1, 2, 3]) + ldj).double().numpy()
    finally:
        torch.Tensor.uniform_ = orig
    t = np.argmax(y, axis=1)
    nll = float(-table[np.arange(n), t].mean())
    assert abs(nll - float(data["nll"])) <= 1e-6 * abs(float(data["nll"])), (nll, float(data["nll"]))
    path = os.path.join(HERE, "image_ycond", NAME + ".npz")
    np.savez_compressed(path, config=np.frombuffer(json.dumps(dict(case="image_class_table", source=SOURCE, N=n, Y=Y)).encode(), dtype=np.uint8),
                        table=table)
    print(f"{NAME}: table {table.shape}, nll on the fixture's labels {nll:.6f} vs {float(data['nll']):.6f}, {os.path.getsize(path)} bytes")


if __name__ == "__main__":
    main()
