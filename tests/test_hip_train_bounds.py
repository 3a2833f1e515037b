"""GPU: the sizes the trainer reports are sufficient and no call writes outside them.

Every case runs one forward and one backward call through the C ABI on buffers of exactly gbnf_trainer_trace_floats(n) floats and
gbnf_trainer_workspace_bytes(n) bytes, each followed by a guard of 4096 floats; both buffers start out filled with one NaN bit
pattern, so a result that depended on a word the call never wrote would not meet the oracle, and a write past the reported size
changes the guard.  Shapes are the smallest that reach each path of gbnf_trainer_forward / _backward (d = 6, K <= 4; n = 1, 17, 33:
one ragged tile, a ragged second tile, two workgroups).  Tolerances are those of test_hip_train.py: 1e-5 forward, G_RTOL of the
largest entry of each gradient tensor."""
import ctypes as C
import os
import subprocess
import sys

import numpy as np
import pytest

from conftest import REPO, rel_err
from test_hip_train import G_RTOL, _check_grads, _dev_spec, _last_path

pytestmark = pytest.mark.gpu

GUARD = 4096                    # floats behind each buffer
NAN_BITS = 0x7FC0BAD5           # a quiet NaN no kernel produces


def _glow(h=30, K=3):
    from gbnf_amd import synth
    return synth.synth_glow_spec(6, h, K, seed=61)


def _glow_residual():
    """A Glow descriptor with ResidualNet coupling nets: no chained kernel has its skip connection, the per-step kernels train it
    (test_a_glow_residualnet_descriptor_keeps_the_per_step_trainer; its smallest geometry)."""
    from gbnf_amd import synth
    d, h, K = 8, 250, 2
    spec = synth.synth_glow_spec(d, h, K, seed=31)
    rng = np.random.RandomState(32)
    for st in spec["steps"]:
        st["net"] = synth._res_net(rng, d // 2, 2 * (d - d // 2), h, 1, 1.0)
    return spec


def _realnvp(d=6, h=16, K=4, **kw):
    from gbnf_amd import synth
    return synth.synth_realnvp_spec(d, h, K, seed=2, flip_init=0, **kw)


# (id, spec, math, n, batch statistics, with a trace, (forward, backward) launches of the chained kernels: _last_path)
CASES = [
    # the chained sweeps of a Glow: all three trainers (bf16x6 runs the h <= 256 variant: its operand rows are wider than f16x3's,
    # and the repairing trainer reports the larger of the two layouts)
    *[(f"glow_{math}_n{n}", _glow, math, n, False, True, (1, 1)) for math in ("f16x3", "bf16x6", "repair") for n in (1, 17, 33)],
    # the chained sweeps cut into step ranges: RealNVP on batch statistics, a range per BatchNorm step (steps 0 .. K - 2 carry one)
    ("realnvp_batch_stats_f16x3", _realnvp, "f16x3", 17, True, True, (3, 3)),
    ("realnvp_batch_stats_bf16x6", _realnvp, "bf16x6", 17, True, True, (3, 3)),
    # the per-step kernels, with and without a trace
    ("per_step_traced", _glow_residual, "f16x3", 33, False, True, (0, 0)),
    ("per_step_untraced", _glow_residual, "f16x3", 33, False, False, (0, 0)),
    # the per-step backward with the gradient state parked in the workspace: RealNVP on batch statistics with two-block ResidualNets
    # wider than 256, which have no training sweeps (`eval` lines of variants.list)
    ("per_step_batch_stats", lambda: _realnvp(6, 300, 2, coupling_network="residual", depth=2), "f16x3", 17, True, True, (0, 0)),
    # a range-safe trainer without a trace: the chained pair on the trainer's own buffer (workspace guard only)
    ("untraced_bf16x6", _glow, "bf16x6", 17, False, False, (1, 1)),
]


def _buffer(n_floats, dev):
    import torch
    return torch.full((n_floats + GUARD,), NAN_BITS, dtype=torch.int32, device=dev)


def _guard_untouched(buf, n_floats):
    return bool((buf[n_floats:] == NAN_BITS).all().item())


@pytest.mark.parametrize("name,make_spec,math,n,batch_stats,traced,path", CASES, ids=[c[0] for c in CASES])
def test_calls_stay_inside_the_reported_sizes(name, make_spec, math, n, batch_stats, traced, path):
    import torch
    from gbnf_amd import native, synth
    from oracle import gbnf_oracle as oracle
    dev = torch.device("cuda:0")
    L = native.lib()
    spec = make_spec()
    d = spec["d"]
    dv = _dev_spec(spec, dev)
    if batch_stats:
        for st in dv["steps"]:
            if st["bn"] is not None:
                st["bn"]["batch_mean"] = torch.zeros(d, device=dev)
                st["bn"]["batch_var"] = torch.zeros(d, device=dev)
    tr = native.NativeTrainer(dv, math=math)
    tr.set_batch_stats(batch_stats)
    xs = synth.synth_batch(n, d, seed=62)
    rng = np.random.RandomState(63)
    g_z = rng.standard_normal(xs.shape).astype(np.float32)
    g_l = rng.standard_normal(n).astype(np.float32)
    x, gz, gl = (torch.from_numpy(a).to(dev) for a in (xs, g_z, g_l))

    nf, nb = C.c_int64(), C.c_int64()
    assert L.gbnf_trainer_trace_floats(tr.handle, n, C.byref(nf)) == 0
    assert L.gbnf_trainer_workspace_bytes(tr.handle, n, C.byref(nb)) == 0
    assert nb.value % 4 == 0
    trace = _buffer(nf.value, dev) if traced else None
    ws = _buffer(nb.value // 4, dev)
    z, ldj, g_x = torch.empty_like(x), torch.empty(n, device=dev), torch.empty_like(x)
    flat = torch.zeros(tr.grad_floats, device=dev)
    ptr = lambda t: C.c_void_p(t.data_ptr() if t is not None else 0)
    rc = L.gbnf_trainer_forward(tr.handle, ptr(x), n, ptr(z), ptr(ldj), ptr(trace), None)
    assert rc == 0, L.gbnf_last_error().decode(errors="replace")
    rc = L.gbnf_trainer_backward(tr.handle, ptr(x), n, ptr(trace), ptr(gz), ptr(gl), ptr(g_x), ptr(flat), ptr(ws), nb.value, None)
    assert rc == 0, L.gbnf_last_error().decode(errors="replace")
    torch.cuda.synchronize()

    if traced:
        assert _guard_untouched(trace, nf.value), f"{name}: a call wrote behind the {nf.value} floats of the trace buffer"
    assert _guard_untouched(ws, nb.value // 4), f"{name}: a call wrote behind the {nb.value} bytes of the workspace"

    if batch_stats:
        z64, ldj64, _ = oracle.component_forward_train(spec, xs)
    else:
        z64, ldj64 = oracle.component_forward(spec, xs, backend="numpy64")
    gx64, grads64 = oracle.component_grads(spec, xs, g_z, g_l, train=True) if batch_stats else oracle.component_grads(spec, xs, g_z, g_l)
    e_l, e_z = rel_err(ldj.cpu().numpy(), ldj64), float(np.abs(z.cpu().numpy() - z64).max()) / max(1.0, float(np.abs(z64).max()))
    e_x = float(np.abs(g_x.cpu().numpy() - gx64).max()) / max(float(np.abs(gx64).max()), 1e-3)
    print(f"[bounds] {name}: trace {nf.value} floats, workspace {nb.value} bytes, path {_last_path(tr)}, "
          f"rel err ldj {e_l:.2e} z {e_z:.2e} g_x {e_x:.2e}")
    assert e_l < 1e-5 and e_z <= 1e-5
    assert e_x <= G_RTOL
    grads, off = [], 0
    for t, size in zip(tr.params, tr._sizes):
        grads.append(None if t is None else flat[off:off + size].view(t.shape))
        off += size
    # (batch statistics: a gradient that is zero by symmetry is judged on the scale of the largest tensor, as in
    #  test_trainer_batch_stats_against_oracle)
    floor = 0.05 * max(float(np.abs(g).max()) for g in grads64 if g is not None) if batch_stats else 1e-3
    _check_grads(grads, grads64, name, floor=floor)

    assert _last_path(tr) == path


_TWO_DEVICE_CHILD = r"""
import numpy as np, torch
from gbnf_amd import native, synth
from oracle import gbnf_oracle as oracle
spec = synth.synth_glow_spec(43, 215, 5, seed=1)          # MINIBOONE: its f16x3 kernel needs more than 64 KB of LDS
xs = synth.synth_batch(64, 43, seed=0)
z64, ldj64 = oracle.component_forward(spec, xs, backend="numpy64")
for i in (0, 1):
    torch.cuda.set_device(i)
    flow = native.NativeFlow(spec, math="f16x3")
    z, ldj, _ = flow.forward(torch.from_numpy(xs).to(f"cuda:{i}"))
    torch.cuda.synchronize()
    e_l = float(np.max(np.abs(ldj.cpu().numpy() - ldj64) / np.maximum(np.abs(ldj64), 1.0)))
    e_z = float(np.abs(z.cpu().numpy() - z64).max()) / max(1.0, float(np.abs(z64).max()))
    print(f"device {i}: rel err ldj {e_l:.2e} z {e_z:.2e}")
    assert e_l < 1e-5 and e_z <= 1e-5, f"device {i}"
print("two devices ok")
"""


def test_large_lds_kernels_launch_on_a_second_device():
    """The launchers opt in to 160 KB of dynamic LDS per device, not per process: the same kernel, first on device 0, then on
    device 1.  A fresh child process, because the opt-in flags live as long as the process."""
    import torch
    if torch.cuda.device_count() < 2:
        pytest.skip("needs two GPUs")
    env = dict(os.environ, PYTHONPATH=REPO + os.pathsep + os.environ.get("PYTHONPATH", ""))
    r = subprocess.run([sys.executable, "-c", _TWO_DEVICE_CHILD], cwd=REPO, env=env, stdout=subprocess.PIPE, stderr=subprocess.STDOUT,
                       text=True, timeout=300)
    assert r.returncode == 0 and "two devices ok" in r.stdout, r.stdout
