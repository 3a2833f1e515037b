"""The float64 yardstick of gbnf_weights_em / gbnf_weights_to_rho (include/gbnf.h), in numpy: EM for the weights of a mixture whose
components are fixed, over a (C, n) table of per-component log-likelihoods, with the library's contract -- the start from rho, the
row exclusion, the stopping rule, the bad start -- restated line by line.  ``dtype`` and ``reverse`` exist for the sensitivity test:
the same iteration with np.longdouble sums, or with the rows of the data taken in the opposite order."""
import numpy as np

MAX_COMPONENTS = 64
STATE_DOUBLES = 8 + MAX_COMPONENTS


def used_rows(ll):
    """The rows that count: no NaN, no +inf, not -inf under every component."""
    ll = np.asarray(ll)
    bad = np.isnan(ll).any(axis=0) | (ll == np.inf).any(axis=0) | (ll == -np.inf).all(axis=0)
    return ~bad


def start_weights(rho, C, dtype=np.float64):
    """(w^(0), bad): rho[:C] / sum in index order from the float32 entries; bad when an entry is not finite or < 0 or the sum <= 0."""
    r = np.asarray(rho, dtype=np.float32)[:C].astype(dtype)
    total = dtype(0.0)
    for v in r:
        total = total + v
    bad = bool((~np.isfinite(r)).any() or (r < 0).any() or not total > 0)
    with np.errstate(all="ignore"):
        return r / total, bad


def evaluate(ll, w):
    """One evaluation at weights w on the used rows ll (C, N) -> (G (N,), sum of G, S (C,)).  A row whose every finite entry belongs
    to a component of weight 0 has G = -inf and adds nothing to S."""
    dtype = w.dtype.type
    with np.errstate(all="ignore"):
        a = np.log(w)[:, None] + ll
        m = a.max(axis=0)
        live = m > -np.inf
        ms = np.where(live, m, dtype(0.0))
        G = np.where(live, ms + np.log(np.exp(a - ms).sum(axis=0)), -np.inf)
        r = np.where(live[None, :], np.exp(a - np.where(live, G, dtype(0.0))), dtype(0.0))
    return G, G.sum(), r.sum(axis=1)


def em(ll, rho, max_iters, tol, dtype=np.float64, reverse=False, history=None):
    """-> state (STATE_DOUBLES float64, the layout of include/gbnf.h).  ``history``: a list that receives every L_t."""
    ll = np.asarray(ll)
    C, n = ll.shape
    keep = used_rows(ll)
    data = ll[:, keep].astype(dtype)
    if reverse:
        data = data[:, ::-1]
    N = int(keep.sum())
    w, bad = start_weights(rho, C, dtype)
    bad = bad or N == 0
    state = np.zeros(STATE_DOUBLES, dtype=np.float64)
    state[2], state[3] = N, n - N
    t, L_prev, L0, delta, conv = 0, None, None, 0.0, False
    while True:
        _, sG, S = evaluate(data, w)
        with np.errstate(all="ignore"):
            L = sG / dtype(N)
        if history is not None:
            history.append(float(L))
        if t == 0:
            L0 = L
        else:
            delta = abs(L - L_prev)
            conv = bool(tol > 0 and delta <= tol)
        if bad or conv or t == max_iters:
            break
        w = S / dtype(N)
        L_prev = L
        t += 1
    state[0], state[1] = t, float(conv and not bad)
    state[4], state[5], state[6], state[7] = L0, L, delta, float(bad)
    state[8:8 + C] = w
    return state


def mixture_G(ll, w):
    """Per-row log of the flat mixture at weights w, float64, on every row of ll (no exclusion)."""
    return evaluate(np.asarray(ll, dtype=np.float64), np.asarray(w, dtype=np.float64))[0]


def to_rho(state, rho, C, rho_min=0.01, rho_max=100.0):
    """gbnf_weights_to_rho -> (new rho float32, flags word): rho[c] = clamp(float32(w_c * sum(rho[:C])), rho_min, rho_max); nothing after
    a bad start; twice the number of clamped entries added to state[7]."""
    rho = np.array(rho, dtype=np.float32)
    flags = float(state[7])
    if flags % 2:
        return rho, flags
    S = 0.0
    for v in rho[:C]:
        S += float(v)
    v = (np.asarray(state[8:8 + C], dtype=np.float64) * S).astype(np.float32)
    clamped = int(((v < np.float32(rho_min)) | (v > np.float32(rho_max))).sum())
    rho[:C] = np.minimum(np.maximum(v, np.float32(rho_min)), np.float32(rho_max))
    return rho, flags + 2.0 * clamped
