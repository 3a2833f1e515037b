"""GPU: the training kernels against the float64 oracle at the batch sizes where the trainer changes how it launches
(tests/train_large_batch_cases.py: the table, how its plans were worked out, what it covers).

Every case runs on the automatic launch policy (no tuning knob is set): the weight-gradient plan the library takes is asserted
against the table's literal through gbnf_debug_trainer_wgrad_plan, the chained kernels are asserted through
gbnf_debug_trainer_last_path, and forward, parameter gradients, g_x and the batch statistics are compared with
oracle.component_forward / component_forward_train / component_grads at the bars of tests/test_hip_train.py (ldj 1e-5 and z 2e-5 of
their scales; G_RTOL of each gradient tensor's largest entry, with the 0.05 x max floor on batch statistics; statistics atol 2e-6 /
rtol 1e-5 + atol 1e-6).  tests/test_train_large_batch_host.py shows that float32 arithmetic of these shapes meets those bars with
room to spare: a case that fails here at the bar is a kernel finding.

The oracle's results are computed once per (geometry, n, BatchNorm mode) and shared by the math modes and the deterministic twins."""
import ctypes as C

import numpy as np
import pytest

import train_large_batch_cases as T
from test_hip_fused_step import _check_flat_grads
from test_hip_train import G_RTOL, _check_grads, _dev_spec, _has_live_blob, _last_path
from test_hip_train_bounds import GUARD, NAN_BITS

pytestmark = pytest.mark.gpu

_ORACLE = {}


def _dev():
    import torch
    return torch.device("cuda:0")


def _oracle(case):
    """The case's inputs and the float64 oracle's forward, statistics and gradients, computed once per T.oracle_key."""
    key = T.oracle_key(case)
    if key not in _ORACLE:
        from oracle import gbnf_oracle as oracle
        spec, x, g_z, g_l = T.make_inputs(case)
        bs = case[8]
        if bs:
            z64, ldj64, stats = oracle.component_forward_train(spec, x)
        else:
            (z64, ldj64), stats = oracle.component_forward(spec, x, backend="numpy64"), None
        gx64, grads64 = oracle.component_grads(spec, x, g_z, g_l, train=bs)
        _ORACLE[key] = dict(spec=spec, x=x, g_z=g_z, g_l=g_l, z64=z64, ldj64=ldj64, stats=stats, gx64=gx64, grads64=grads64)
    return _ORACLE[key]


def _guarded(n_floats):
    """n_floats + GUARD words of one NaN bit pattern (tests/test_hip_train_bounds.py)."""
    import torch
    return torch.full((n_floats + GUARD,), NAN_BITS, dtype=torch.int32, device=_dev())


def _guard_untouched(buf, n_floats):
    return bool((buf[n_floats:] == NAN_BITS).all().item())


def _trainer(spec, math, deterministic, batch_stats):
    """-> (trainer, device spec, [(batch_mean buffer, batch_var buffer) per BN step]); the statistics live in the first d words of
    guarded buffers."""
    import torch
    from gbnf_amd import native
    d = spec["d"]
    dv = _dev_spec(spec, _dev())
    bufs = []
    if batch_stats:
        for st in dv["steps"]:
            if st["bn"] is not None:
                pair = (_guarded(d), _guarded(d))
                st["bn"]["batch_mean"] = pair[0][:d].view(torch.float32)
                st["bn"]["batch_var"] = pair[1][:d].view(torch.float32)
                bufs.append(pair)
    tr = native.NativeTrainer(dv, math=math, deterministic=deterministic)
    if batch_stats:
        assert tr.has_batch_stats
        tr.set_batch_stats(True)
    return tr, dv, bufs


def _plan(tr, n):
    """(list, blocks, chunk, Y) of the trainer's weight-gradient launch at n rows, as wgrad_plan decides it."""
    from gbnf_amd import native
    L = native.lib()
    L.gbnf_debug_trainer_wgrad_plan.argtypes = [C.c_void_p, C.c_int64, C.POINTER(C.c_int32)]
    L.gbnf_debug_trainer_wgrad_plan.restype = C.c_int
    out = (C.c_int32 * 4)()
    assert L.gbnf_debug_trainer_wgrad_plan(tr.handle, n, out) == 0, L.gbnf_last_error().decode(errors="replace")
    return tuple(int(v) for v in out)


def _ws_bytes(tr, n):
    from gbnf_amd import native
    nb = C.c_int64()
    assert native.lib().gbnf_trainer_workspace_bytes(tr.handle, n, C.byref(nb)) == 0
    return int(nb.value)


def _backward_guarded(tr, x, gz, gl, trace):
    """gbnf_trainer_backward with g_x in the first n d words of a guarded buffer -> (g_x, gradient views, the rows behind row n are
    untouched)."""
    import torch
    from gbnf_amd import native
    n, d = x.shape
    nb = _ws_bytes(tr, n)
    ws = torch.empty((nb + 3) // 4, dtype=torch.float32, device=x.device)
    gxbuf = _guarded(n * d)
    flat = torch.zeros(tr.grad_floats, dtype=torch.float32, device=x.device)
    ptr = lambda t: C.c_void_p(t.data_ptr())
    L = native.lib()
    rc = L.gbnf_trainer_backward(tr.handle, ptr(x), n, ptr(trace), ptr(gz), ptr(gl), ptr(gxbuf), ptr(flat), ptr(ws), nb, native._stream_ptr())
    assert rc == 0, L.gbnf_last_error().decode(errors="replace")
    torch.cuda.synchronize()
    grads, off = [], 0
    for t, size in zip(tr.params, tr._sizes):
        grads.append(None if t is None else flat[off:off + size].view(t.shape))
        off += size
    return gxbuf[:n * d].view(torch.float32).view(n, d), grads, _guard_untouched(gxbuf, n * d)


def _rel(a, b, floor=0.0):
    return float(np.abs(a - b).max()) / max(float(np.abs(b).max()), floor)


def _run(case, o, deterministic):
    """One trainer of the case's math mode: plan, path, forward, statistics, gradients and sentinels -> (g_x, gradients) on the host."""
    import torch
    kind, d, h, K, n, kw, math, _, bs, (want_list, want_chunk, want_Y) = case
    what = T.case_id(case) + ("" if deterministic == case[7] else " (mode off)")
    tr, dv, bufs = _trainer(o["spec"], math, deterministic, bs)
    assert _has_live_blob(tr)
    lst, blocks, chunk, Y = _plan(tr, n)
    print(f"[large batch] {what}: list {lst}, {blocks} blocks, chunk {chunk}, Y {Y}")
    assert (lst, chunk, Y) == (want_list, want_chunk, want_Y), what
    x, gz, gl = (torch.from_numpy(o[k]).to(_dev()) for k in ("x", "g_z", "g_l"))
    ranges = K - 1 if bs else 1                    # (a range starts at every BatchNorm step: steps 0 .. K - 2 carry one)

    z, ldj, trace = tr.forward(x, want_trace=True)
    assert _last_path(tr)[0] == ranges, what
    z64, ldj64 = o["z64"], o["ldj64"]
    e_l = float(np.abs(ldj.cpu().numpy() - ldj64).max()) / max(1.0, float(np.abs(ldj64).max()))
    e_z = float(np.abs(z.cpu().numpy() - z64).max()) / max(1.0, float(np.abs(z64).max()))
    print(f"[large batch] {what}: forward rel err ldj {e_l:.2e} z {e_z:.2e}")
    assert e_l <= 1e-5 and e_z <= 2e-5, what

    if bs:
        e_m = e_v = 0.0
        for k, (mbuf, vbuf) in enumerate(bufs):
            mean, var = (b[:d].view(torch.float32).cpu().numpy() for b in (mbuf, vbuf))
            rm, rv = o["stats"][k]
            e_m = max(e_m, float(np.abs(mean - rm).max()))
            e_v = max(e_v, float((np.abs(var - rv) / (1e-6 + 1e-5 * np.abs(rv))).max()))
            assert _guard_untouched(mbuf, d) and _guard_untouched(vbuf, d), f"{what}: BN step {k} wrote behind its d statistics"
        print(f"[large batch] {what}: batch mean abs err {e_m:.2e} (bar 2e-6), batch var err / (1e-6 + 1e-5 |var|) {e_v:.2e} (bar 1)")
        for k, (mbuf, vbuf) in enumerate(bufs):
            np.testing.assert_allclose(mbuf[:d].view(torch.float32).cpu().numpy(), o["stats"][k][0], rtol=0, atol=2e-6)
            np.testing.assert_allclose(vbuf[:d].view(torch.float32).cpu().numpy(), o["stats"][k][1], rtol=1e-5, atol=1e-6)

    gx64, grads64 = o["gx64"], o["grads64"]
    top = max(float(np.abs(g).max()) for g in grads64 if g is not None)
    floor = 0.05 * top if bs else 1e-3
    gx, grads = tr.backward(x, gz, gl, want_gx=True, trace=trace)
    torch.cuda.synchronize()
    assert _last_path(tr)[1] == ranges, what
    gx_h = gx.cpu().numpy()
    worst = max(_rel(a.cpu().numpy().reshape(b.shape), b, floor) for a, b in zip(grads, grads64) if b is not None)
    print(f"[large batch] {what}: backward rel err parameters {worst:.2e} g_x {_rel(gx_h, gx64):.2e} (bar {G_RTOL})")
    _check_grads(grads, grads64, what, floor=floor)
    assert np.abs(gx_h - gx64).max() <= G_RTOL * float(np.abs(gx64).max()), what
    # the same call with g_x in a guarded buffer: nothing behind row n is written, and the call repeats on the same trace
    gx2, grads2, clean = _backward_guarded(tr, x, gz, gl, trace)
    assert clean, f"{what}: the backward call wrote behind row {n} of g_x"
    _check_grads(grads2, grads64, what + " (guarded call)", floor=floor)
    assert np.abs(gx2.cpu().numpy() - gx64).max() <= G_RTOL * float(np.abs(gx64).max()), what
    return tr, gx, grads, (x, gz, gl, trace)


@pytest.mark.parametrize("case", T.CASES, ids=[T.case_id(c) for c in T.CASES])
def test_large_batch_against_oracle(case):
    import torch
    kind, d, h, K, n, kw, math, det, bs, plan = case
    o = _oracle(case)
    tr, gx, grads, _ = _run(case, o, det)
    if not det:
        return
    # deterministic mode: Y partials per gradient entry behind the default workspace; two fresh trainers agree bit for bit; the
    # default mode agrees to G_RTOL
    off, gx_off, grads_off, _ = _run(case, o, False)
    assert _ws_bytes(tr, n) - _ws_bytes(off, n) == plan[2] * tr.grad_floats * 4
    tr2, gx_b, grads_b, _ = _run(case, o, True)
    first = [g for g in grads if g is not None] + [gx]
    again = [g for g in grads_b if g is not None] + [gx_b]
    assert all(torch.equal(a, b) for a, b in zip(first, again)), f"{T.case_id(case)}: two fresh deterministic trainers differ"
    for k, (a, b) in enumerate(zip(grads, grads_off)):
        if a is not None:
            a, b = a.cpu().numpy(), b.cpu().numpy()
            assert np.abs(a - b).max() <= G_RTOL * max(float(np.abs(a).max()), 1e-3), f"{T.case_id(case)}: gradient {k} against the default mode"
    assert float((gx - gx_off).abs().max()) <= G_RTOL * float(gx.abs().max())


def test_fused_step_on_batch_statistics_at_the_three_launch_size():
    """gbnf_trainer_nll_step on the HEPMASS geometry in batch-statistics mode at n = 16385 (the three-launch statistics with a short
    last row chunk, probs_dev): the loss, the flat gradient and the moved running statistics against the float64 oracle, at the bars
    of tests/test_hip_fused_step.py (loss 1e-5 relative, G_RTOL per tensor with its 1e-3 floor, running statistics atol 2e-6)."""
    import torch
    from gbnf_amd import native, synth
    from oracle import gbnf_oracle as oracle
    kind, d, h, K, n, kw = T.FUSED_STEP_CASE
    spec = synth.synth_realnvp_spec(d, h, K, seed=411, flip_init=1, **kw)
    xs = synth.synth_batch(n, d, seed=412)
    # the float64 step: nll = mean(-(log N(z) + ldj)) on batch statistics, its gradient, running <- 0.9 running + 0.1 batch
    z64, ldj64, stats = oracle.component_forward_train(spec, xs)
    nll64 = float(np.mean(-(np.sum(-0.5 * np.log(2 * np.pi) - 0.5 * z64 * z64, axis=1) + ldj64)))
    _, grads64 = oracle.component_grads(spec, xs, z64 / n, np.full(n, -1.0 / n), train=True)
    flat64 = np.concatenate([np.zeros(d) if g is None else g.reshape(-1) for g in grads64])
    tr, dv, bufs = _trainer(spec, "f16x3", False, True)
    bns = [st["bn"] for st in dv["steps"] if st["bn"] is not None]
    run64 = [(0.9 * bn["running_mean"].cpu().numpy().astype(np.float64) + 0.1 * stats[k][0],
              0.9 * bn["running_var"].cpu().numpy().astype(np.float64) + 0.1 * stats[k][1]) for k, bn in enumerate(bns)]
    assert _plan(tr, n)[0] == T.BIG
    before = [None if t is None else t.clone() for t in tr.params]
    stats_dev, flat = tr.nll_step(torch.from_numpy(xs).to(_dev()), native.OptState(tr, "adamw"), lr=0.0, bn_momentum=0.9)
    torch.cuda.synchronize()
    nll = float(stats_dev[0])
    print(f"[large batch] fused step n={n}: nll {nll} vs {nll64}")
    assert abs(nll - nll64) <= 1e-5 * abs(nll64)
    _check_flat_grads(flat, flat64, tr, "fused step")
    for k, bn in enumerate(bns):
        np.testing.assert_allclose(bn["running_mean"].cpu().numpy(), run64[k][0], rtol=0, atol=2e-6)
        np.testing.assert_allclose(bn["running_var"].cpu().numpy(), run64[k][1], rtol=0, atol=2e-6)
        assert _guard_untouched(bufs[k][0], d) and _guard_untouched(bufs[k][1], d)
    for t, b in zip(tr.params, before):          # lr = 0: the parameters stay
        if t is not None:
            assert torch.equal(t, b)
