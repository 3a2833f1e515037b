"""The float64 yardstick of the joint mixture step: the mixture NLL  L = -1/n sum_i G_i,  G_i = LSE_c(log w_c + ll_c(x_i)),
w_c = rho_c / sum(rho[:C]),  and its gradient with respect to every component's parameters, built only from
tests/score_oracle.py (the forward half) and oracle.component_grads.

    step64(specs, rho, x, r=None) -> (nll, G (N,), r (C,N), rbar (C,), [gradients of component c per entry of param_arrays(spec_c)])

dL/dtheta_c = -1/n sum_i r_ic d ll_c(x_i)/dtheta_c with r = softmax_c(log w + ll), and d ll_c / dtheta_c is the vector-Jacobian
product of component c's forward with the seeds  g_z = -z_c, g_ldj = 1  per row: so component c's gradient is
component_grads(spec_c, x, r_c[:, None] * z_c / n, -r_c / n)[1].  r given: a test hands in the device's r to judge the backward on
its own seeds (the gradient is linear in r).  rbar_c = mean_i r_ic is the EM update of the weights on this batch.
"""
import numpy as np

from oracle import gbnf_oracle as oracle
import score_oracle


def flat64(spec, grads):
    """The per-tensor gradients of one component in the library's flat layout (reserved regions: zeros of d entries)."""
    out = []
    for a, g in zip(oracle.param_arrays(spec), grads):
        out.append(np.zeros(spec["d"]) if a is None else np.asarray(g, dtype=np.float64).reshape(-1))
    return np.concatenate(out)


def step64(specs, rho, x, r=None, forward=None):
    """``forward``: score_oracle.mixture64(specs, rho, x) if the caller has it already (computed once, shared)."""
    specs = list(specs)
    x = np.asarray(x, dtype=np.float64)
    n = x.shape[0]
    zs, ll, r64, G = score_oracle.mixture64(specs, rho, x) if forward is None else forward
    r = r64 if r is None else np.asarray(r, dtype=np.float64)
    grads = [oracle.component_grads(sp, x, r[c][:, None] * zs[c] / n, -r[c] / n)[1] for c, sp in enumerate(specs)]
    return -float(G.mean()), G, r, r.mean(axis=1), grads


def nll64(specs, rho, x):
    """The loss alone (central differences walk it)."""
    return -float(score_oracle.mixture64(list(specs), rho, np.asarray(x, dtype=np.float64))[3].mean())
