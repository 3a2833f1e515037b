"""Float64 numpy restatement of what the reference's two ``evaluate`` functions compute -- the yardstick of tests/test_eval_host.py and
tests/test_hip_eval.py:

  mixture_G          the prefix-normalised recursion of density_experiment.py:561-573
  summary            nll / g_nll / ratio of density_experiment.py:581-591 (and the batch-mean form of :594)
  cross_entropy      F.cross_entropy(y_logits, argmax(y)) of image_experiment.py:236, per row, and the prediction
and, on top of them, the 16 doubles of the device's evaluation state (include/gbnf.h) for a list of batches.

Everything is elementwise IEEE double arithmetic in index order over the components, so a device that rounds every product and sum on
its own gives the same per-row values; sums over rows are exact (math.fsum) and compared within a summation bound."""
import math

import numpy as np

STATE_DOUBLES = 16


def _lse2(a, b):
    """torch.logsumexp over two terms: an infinite maximum is replaced by 0 before the subtraction; a NaN term gives NaN."""
    with np.errstate(invalid="ignore", divide="ignore", over="ignore"):
        m = np.fmax(a, b)
        m = np.where(np.isinf(m), 0.0, m)
        out = m + np.log(np.exp(a - m) + np.exp(b - m))
    return np.where(np.isnan(a) | np.isnan(b), np.nan, out)


def mixture_G(ll, rho, dtype=np.float64):
    """G (n,) of a (n_used, n) table: G_0 = ll_0; r_c = rho_c / sum(rho[0..c]); G_c = LSE(log(1 - r_c) + G_{c-1}, log(r_c) + ll_c).
    ``dtype=np.float32`` replays the recursion in the reference's own precision (rho's prefix sums included)."""
    ll = np.asarray(ll, dtype=dtype)
    rho = np.asarray(rho, dtype=dtype)
    G = ll[0].copy()
    with np.errstate(invalid="ignore", divide="ignore"):
        for c in range(1, ll.shape[0]):
            r = rho[c] / np.sum(rho[0:c + 1], dtype=dtype)
            G = _lse2((np.log(dtype(1) - r) + G).astype(dtype), (np.log(r) + ll[c]).astype(dtype)).astype(dtype)
    return G


def weights(rho, n_used):
    """w_c = rho[c] / sum_{k < n_used} rho[k] in double, the sum in index order."""
    total = 0.0
    for k in range(n_used):
        total = total + float(rho[k])
    return np.array([float(rho[c]) / total for c in range(n_used)], dtype=np.float64)


def expected_ll(ll, rho):
    """E (n,) = sum_c w_c ll_c in double, index order, every product and sum rounded on its own."""
    ll = np.asarray(ll, dtype=np.float64)
    w = weights(rho, ll.shape[0])
    E = np.zeros(ll.shape[1], dtype=np.float64)
    with np.errstate(invalid="ignore"):
        for c in range(ll.shape[0]):
            E = E + w[c] * ll[c]
    return E


def summary(G, g, first_pass_component_zero=False):
    """density_experiment.py:581-591 on the concatenated per-row log-likelihoods: nll = mean(-G), g_nll = mean(-g),
    ratio = mean(g_nll - G_nll); with ``component == 0 and not all_trained`` g_nll = nll and ratio = 0."""
    G, g = np.asarray(G, dtype=np.float64), np.asarray(g, dtype=np.float64)
    out = {"nll": float(np.mean(-G)), "g_nll": float(np.mean(-g)), "ratio": float(np.mean((-g) - (-G)))}
    if first_pass_component_zero:
        out["g_nll"], out["ratio"] = out["nll"], 0.0
    return out


def _first_argmax(row):
    """The first largest entry; a NaN never wins; a row without a number gives 0."""
    best, at = -math.inf, 0
    for k, v in enumerate(row):
        if v > best:
            best, at = v, k
    return at


def cross_entropy(logits, y):
    """(CE (n,) float64, label (n,), prediction (n,)): CE_i = logsumexp(logits_i) - logits_i[label_i], label_i the first largest entry
    of y_i, prediction_i the first largest logit.  The exponentials are added in index order."""
    logits = np.asarray(logits, dtype=np.float64)
    y = np.asarray(y)
    n = logits.shape[0]
    ce = np.zeros(n, dtype=np.float64)
    label, pred = np.zeros(n, dtype=np.int64), np.zeros(n, dtype=np.int64)
    for i in range(n):
        label[i], pred[i] = _first_argmax(y[i]), _first_argmax(logits[i])
        m = float(logits[i][pred[i]]) if not math.isnan(float(logits[i][pred[i]])) else -math.inf
        if math.isinf(m):
            m = 0.0
        s = 0.0
        with np.errstate(over="ignore", invalid="ignore"):
            for v in logits[i]:
                s = s + float(np.exp(np.float64(v) - m))
            ce[i] = (m + float(np.log(np.float64(s)))) - float(logits[i][label[i]])
    return ce, label, pred


def fsum(v):
    """The exact sum of float64 values, as numpy propagates NaN and infinities."""
    v = np.asarray(v, dtype=np.float64).ravel()
    return math.fsum(v) if np.isfinite(v).all() else float(np.sum(v))


def state_of(tables, rho, component, G_of=None):
    """The evaluation state after the batches ``tables`` (each (n_used, n), the device's own float32 values): 16 float64.
    ``G_of``: the per-batch G (float32) to use instead of this module's float64 recursion (the device's own ``G_out``).  G - g is
    formed in float32 where both are float32, as the device and the reference form it."""
    s = np.zeros(STATE_DOUBLES, dtype=np.float64)
    for b, ll in enumerate(tables):
        ll = np.asarray(ll)
        n = ll.shape[1]
        if n == 0:
            continue
        G = mixture_G(ll, rho) if G_of is None else np.asarray(G_of[b])
        g = ll[component]
        with np.errstate(invalid="ignore"):
            d = (G - g) if G.dtype == np.float32 and g.dtype == np.float32 else G.astype(np.float64) - g.astype(np.float64)
        E = expected_ll(ll, rho)
        sums = [fsum(G), fsum(g), fsum(d), fsum(E)]
        s[0] += n
        s[1] += 1
        s[2:6] += sums
        s[6] += sums[0] / n
        s[7] += sums[1] / n
        s[8] += sums[3] / n
        s[9] += int(np.sum(~(np.isfinite(G.astype(np.float64)) & np.isfinite(g.astype(np.float64)) & np.isfinite(E))))
    return s


def class_state(logits, y, rho, n_used, c):
    """Entries 10 - 12 that one gbnf_eval_accumulate_class_loss call adds: (w sum CE, w mean CE, w correct)."""
    ce, label, pred = cross_entropy(logits, y)
    w = weights(rho, n_used)[c]
    S = fsum(ce)
    return np.array([w * S, w * (S / len(ce)), w * float(np.sum(label == pred))], dtype=np.float64)
