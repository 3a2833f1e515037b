"""Cases and float64 yardsticks of the all-class density table (gbnf_image_flow_forward_classes, gbnf_class_posterior): helper, not a
test.

The cases are tests/image_ycond_oracle.py's (g22: Y = 10 on a 4x4 map; G: Y = 256, Cz = 64 on a 2x2 map; D: three levels; S1: n = 1,
Y = 1; S70: n = 70) and one more, W: a (1, 32, 32) input with one level -- a 16x16 top map of 256 pixels, more than a wave has lanes and
several of its strides -- with 70 classes, more than 64 and no multiple of it.

The table's yardstick is ``image_ycond_oracle.forward(spec, P, x, noise, e_k)["ll"]`` for every class k.  For more than 100 classes
(G) the flow runs once and the prior of every class is restated in numpy on the yardstick's own z and ldj (``np_table`` with
``image_ycond_oracle.np_prior``): the flow does not see y, so this is the same number at a 256th of the time."""
import functools
import os

import numpy as np
import torch

import image_ycond_oracle as iyo

CASES = dict(iyo.YC_CASES)
CASES["W"] = ((1, 32, 32), dict(h=16, K=1, L=1), 2, 3, 70)
FORWARD_PER_CLASS_UP_TO = 100


def geometry(name):
    """(n, Y, Cz, HW) of a case: each level squeezes (C, H, W) to (4C, H/2, W/2) and every level but the last drops half the channels."""
    (c, h, w), kw, n, _, Y = CASES[name]
    for level in range(kw["L"]):
        c, h, w = c * 4, h // 2, w // 2
        if level < kw["L"] - 1:
            c //= 2
    return n, Y, c, h * w


def make_case(name):
    """-> (spec with "ycond", x, noise) of a case (image_ycond_oracle.make_case's recipe, without labels)."""
    from gbnf_amd import synth
    size, kw, N, seed, Y = CASES[name]
    x, noise = synth.synth_image_batch(N, size, seed=100 + seed)
    return synth.synth_image_glow_spec(size, seed=seed, y_classes=Y, **kw), x, noise


def top_of(spec):
    """(bias, logs) of the spec's learn_top, or None: what image_ycond_oracle.np_prior takes."""
    lt = spec["learn_top"]
    return None if lt is None else (np.asarray(lt["b"]).reshape(-1), np.asarray(lt["logs"]).reshape(-1))


def np_table(z, ldj, h):
    """The closed form of csrc/gbnf_image_ycond.hip's table kernel in numpy float64: z (n, Cz, Hz, Wz), ldj (n,), h (Y, 2 Cz) the prior
    of every class (mean half, log-variance half) -> table[i, k] = sum_{c,p} -0.5 (lv + (z - mu)^2 e^-lv) + ldj[i]."""
    z, ldj, h = (np.asarray(a, dtype=np.float64) for a in (z, ldj, h))
    n, Cz = z.shape[:2]
    zf = z.reshape(n, 1, Cz, -1)
    mu, lv = h[None, :, :Cz, None], h[None, :, Cz:, None]
    return (-0.5 * (lv + (zf - mu) ** 2 * np.exp(-lv))).sum(axis=(2, 3)) + ldj[:, None]


def class_priors(spec, top_h=None):
    """(Y, 2 Cz) float64: h of y = e_k for every k (image_ycond_oracle.np_prior on the identity).  ``top_h`` (2 Cz,): the y-free part as
    the caller has it (an evaluation handle keeps float32(bias e^{3 logs})); None: from the spec's learn_top in float64."""
    yc = spec["ycond"]
    Y = np.asarray(yc["cond_w"]).shape[1]
    u, h = iyo.np_prior(top_of(spec), yc, np.eye(Y))
    if top_h is not None:
        h = np.asarray(top_h, dtype=np.float64)[None, :] + u * np.exp(3.0 * np.asarray(yc["cond_logs"], dtype=np.float64))[None, :]
    return h


def handle_top_h(spec):
    """The y-free prior as gbnf_image_flow_create packs it: float32(bias * exp(3 logs)) formed in double precision; zeros without learn_top."""
    top = top_of(spec)
    Cz2 = np.asarray(spec["ycond"]["cond_w"]).shape[0]
    if top is None:
        return np.zeros(Cz2)
    return (top[0].astype(np.float64) * np.exp(3.0 * top[1].astype(np.float64))).astype(np.float32).astype(np.float64)


@functools.lru_cache(maxsize=None)
def yardstick(name):
    """-> (spec, x, noise, dict(z, ldj, table, y_logits) float64 numpy): computed once, shared, left unchanged."""
    sp, x, noise = make_case(name)
    n, Y = x.shape[0], CASES[name][4]
    P = iyo.leaf_params(sp)
    eye = np.eye(Y, dtype=np.float32)
    with torch.no_grad():
        out = iyo.forward(sp, P, x, noise, np.repeat(eye[:1], n, axis=0))
        z, ldj, logits = out["z"].numpy(), out["ldj"].numpy(), out["y_logits"].numpy()
        if Y > FORWARD_PER_CLASS_UP_TO:
            table = np_table(z, ldj, class_priors(sp))
        else:
            table = np.stack([iyo.forward(sp, P, x, noise, np.repeat(eye[k:k + 1], n, axis=0))["ll"].numpy() for k in range(Y)], axis=1)
    return sp, x, noise, {"z": z, "ldj": ldj, "table": table, "y_logits": logits}


def np_posterior(table, log_prior=None):
    """float64 (log_px (n,), log_post (n, Y)) with torch.logsumexp's treatment of infinities; log_prior None: uniform."""
    table = np.asarray(table, dtype=np.float64)
    Y = table.shape[1]
    a = table + (np.full(Y, -np.log(Y)) if log_prior is None else np.asarray(log_prior, dtype=np.float64))[None, :]
    with np.errstate(all="ignore"):
        m = a.max(axis=1)
        m = np.where(np.isinf(m), 0.0, m)
        lpx = m + np.log(np.exp(a - m[:, None]).sum(axis=1))
        return lpx, a - lpx[:, None]


def np_mixture(tables, rho):
    """float64 recursion of gbnf_mixture_lse over axis 0 of ``tables`` (C, ...): r_c = rho_c / sum(rho[0..c])."""
    rho = np.asarray(rho, dtype=np.float64)
    G = np.asarray(tables[0], dtype=np.float64)
    for c in range(1, len(tables)):
        r = rho[c] / rho[:c + 1].sum()
        G = np.logaddexp(np.log1p(-r) + G, np.log(r) + np.asarray(tables[c], dtype=np.float64))
    return G


def g23_load():
    data = np.load(os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden", "image_ycond", "g23_image_class_table.npz"))
    return np.asarray(data["table"], dtype=np.float64)
