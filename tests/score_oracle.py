"""The float64 yardstick of the tabular score: grad_x log p(x) of the boosted mixture  log p(x) = LSE_c(log w_c + ll_c(x)),
w_c = rho_c / sum(rho[:C]),  built only from oracle.component_forward(..., backend="numpy64") and oracle.component_grads.

    score64(specs, rho, x, base=None, r=None) -> (g_x (N,d), G (N,), r (C,N), ll (C,N))

ll_c = log N(z_c; base) + ldj_c (the 2 pi term included: oracle.log_normal_standard_sum / log_normal_base_sum),
r = softmax_c(log w + ll) unless given (a test hands in the device's r to judge the backward on its own seeds), and
g_x = sum_c component_grads(spec_c, x, g_z = -r_c (z_c - mean) / std^2, g_ldj = r_c)[0]: the backward is linear in its seeds.
"""
import numpy as np

from oracle import gbnf_oracle as oracle


def component_ll64(spec, x, base=None):
    """(z (N,d), ldj (N,), ll (N,)) of one component in float64."""
    z, ldj = oracle.component_forward(spec, x, backend="numpy64")
    z = np.asarray(z, dtype=np.float64)
    ldj = np.asarray(ldj, dtype=np.float64)
    ops = oracle._ops("numpy64")
    if base is None:
        ll = np.asarray(oracle.log_normal_standard_sum(ops, z), dtype=np.float64) + ldj
    else:
        ll = np.asarray(oracle.log_normal_base_sum(ops, z, np.asarray(base[0], np.float64), np.asarray(base[1], np.float64)),
                        dtype=np.float64) + ldj
    return z, ldj, ll


def log_weights64(rho, n_components):
    rho = np.asarray(rho, dtype=np.float64)[:n_components]
    return np.log(rho / rho.sum())


def responsibilities64(ll, log_w):
    """(r (C,N), G (N,)) from ll (C,N) and log_w (C,): the softmax over components and its log-sum-exp."""
    a = np.asarray(ll, dtype=np.float64) + np.asarray(log_w, dtype=np.float64)[:, None]
    m = a.max(axis=0)
    e = np.exp(a - m)
    s = e.sum(axis=0)
    return e / s, m + np.log(s)


def mixture64(specs, rho, x, base=None):
    """The forward half: (zs [C x (N,d)], ll (C,N), r (C,N), G (N,)) in float64."""
    fwd = [component_ll64(sp, x, base) for sp in specs]
    ll = np.stack([f[2] for f in fwd], axis=0)
    r, G = responsibilities64(ll, log_weights64(rho, len(fwd)))
    return [f[0] for f in fwd], ll, r, G


def score_terms64(specs, x, zs, r, base=None):
    """(C,N,d): term c = r_c[:, None] * grad_x ll_c(x), through the oracle's vector-Jacobian product with the seeds
    g_z = -r_c (z_c - mean) / std^2 and g_ldj = r_c.  Their sum over c is the mixture's score."""
    x = np.asarray(x, dtype=np.float64)
    r = np.asarray(r, dtype=np.float64)
    mean = np.zeros(x.shape[1]) if base is None else np.asarray(base[0], dtype=np.float64)
    std = np.ones(x.shape[1]) if base is None else np.asarray(base[1], dtype=np.float64)
    return np.stack([oracle.component_grads(sp, x, -r[c][:, None] * (zs[c] - mean) / (std * std), r[c])[0]
                     for c, sp in enumerate(specs)], axis=0)


def score64(specs, rho, x, base=None, r=None):
    specs = list(specs)
    x = np.asarray(x, dtype=np.float64)
    zs, ll, r64, G = mixture64(specs, rho, x, base)
    r = r64 if r is None else np.asarray(r, dtype=np.float64)
    return score_terms64(specs, x, zs, r, base).sum(axis=0), G, r, ll
