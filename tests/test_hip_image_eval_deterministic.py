"""GPU: the deterministic mode of an image evaluation handle (gbnf_image_flow_set_deterministic; csrc/gbnf_image.hip,
gbnf_image_net.hip, gbnf_image_hx3.hip.h) -- every log-det partial of a forward call stored to a slot of its image, an image's slots
added in slot order by one thread -- through native.NativeImageFlow / the C ABI and, at the end, through BoostedImageFlow.

Geometries: the smallest that reach each kernel that carries a log-det (GEOMETRIES below), each on a `default` and an `f32` handle.
Bars: bit equality (uint32 views) wherever the mode promises it; the project's 1e-5 relative bar against the float64 oracle
(BASELINE.json; the float32 reference arithmetic itself sits at <= 3e-7 on these shapes); 128 * 2^-24 relative
between two default-mode evaluations of ldj (the allowance of tests/test_hip_image_train.py for the atomic sums)."""
import copy
import ctypes as C
import functools
import os
import subprocess
import sys

import numpy as np
import pytest

import test_image_boost_host as host
from conftest import REPO, rel_err

pytestmark = pytest.mark.gpu

LL_RTOL = 1e-5
LR = 1e-3
# id -> (input size, synth_image_glow_spec keywords, n)
GEOMETRIES = {
    "G": ((3, 32, 32), dict(h=32, K=2, L=2), 4),          # the fused kernel on 16- and 8-wide maps, FULL instantiations
    "F": ((1, 28, 20), dict(h=32, K=2, L=2, learn_top=False, permutation="reverse"), 3),      # maps smaller than storage: masked epilogues
    "D": ((3, 32, 32), dict(h=32, K=1, L=3, depth=0), 2),  # third level: a 4 x 4 map in 8-wide storage, 7 chunks, n_mid = 0
    "C": ((3, 16, 32), dict(h=48, K=1, L=2, depth=2, coupling="additive", permutation="shuffle"), 2),      # Split2d's ordered epilogue only
    "W": ((3, 32, 32), dict(h=320, K=1, L=1), 1),          # KH = 2 halves of the fused kernel
    # 48 coupling outputs on 16-wide maps: refused by the fused kernel.  Its first 3x3 has 24 input channels = 7 chunks of the folded
    # contraction, which the two-kernel form (at most 5) refuses too: the `default` handle runs this geometry on the exact-f32
    # convolutions (asserted below).  img_last_hx3_kernel is reached through GBNF_IMG_NO_FUSE: test_the_two_kernel_form.
    "T": ((12, 32, 32), dict(h=32, K=1, L=1), 2),
}
MODES = ("default", "f32")


def _dev():
    import torch
    return torch.device("cuda:0")


def _to(a):
    import torch
    return torch.from_numpy(np.ascontiguousarray(a)).to(_dev())


def _bits(t):
    """The uint32 view of a float32 device tensor, on the host."""
    return t.detach().cpu().contiguous().numpy().view(np.uint32)


@functools.lru_cache(maxsize=None)
def _spec(gid, y_classes=0):
    from gbnf_amd import synth
    size, kw, _ = GEOMETRIES[gid]
    extra = dict(y_classes=y_classes) if y_classes else {}
    return synth.synth_image_glow_spec(size, seed=21 + sorted(GEOMETRIES).index(gid), **kw, **extra)


@functools.lru_cache(maxsize=None)
def _batch(gid, n=None, seed=300):
    from gbnf_amd import synth
    size, _, n0 = GEOMETRIES[gid]
    return synth.synth_image_batch(n or n0, size, seed=seed)


@functools.lru_cache(maxsize=None)
def _oracle64(gid):
    """(z, ldj, ll) of the float64 oracle on the geometry's batch: computed once, shared, left unchanged."""
    import torch
    from oracle import gbnf_oracle as oracle
    x, noise = _batch(gid)
    z, _, _, ld, ll = oracle.image_component_forward(_spec(gid), x, noise, dtype=torch.float64)
    return np.asarray(z, dtype=np.float64), np.asarray(ld, dtype=np.float64), np.asarray(ll, dtype=np.float64)


@functools.lru_cache(maxsize=None)
def _flow(gid, mode):
    """One handle per (geometry, math mode), shared by the tests: every test leaves its deterministic mode OFF."""
    import torch              # (before the library is loaded, as everywhere in the suite: one HIP runtime per process)
    from gbnf_amd import native
    flow = native.NativeImageFlow(_spec(gid), math=mode)
    st = flow.numerics()
    assert native.MATH_NAME[int(st.math_mode)] == ("f32" if mode == "f32" else "f16x3") and not st.demoted, (gid, mode)
    return flow


class _det:
    """with _det(flow, ...): the handles' deterministic mode on inside, off behind."""

    def __init__(self, *flows):
        self.flows = flows

    def __enter__(self):
        for f in self.flows:
            f.deterministic = True
            assert f.deterministic is True
        return self.flows[0]

    def __exit__(self, *exc):
        for f in self.flows:
            f.deterministic = False


@pytest.mark.parametrize("mode", MODES)
@pytest.mark.parametrize("gid", sorted(GEOMETRIES))
def test_repeats_are_bit_equal_and_meet_the_oracle(gid, mode):
    """1 + 3. Mode on: 24 identical calls give the same z, ldj, ll bit for bit; ll and ldj meet the float64 oracle at the project's
    bar; z is bit-identical to the same handle's z with the mode off."""
    flow = _flow(gid, mode)
    x, noise = _batch(gid)
    xd, nd = _to(x), _to(noise)
    z_off, ldj_off, ll_off = flow.forward(xd, nd)
    with _det(flow):
        first = flow.forward(xd, nd)
        want = [_bits(t) for t in first]
        for k in range(23):
            got = flow.forward(xd, nd)
            for name, a, b in zip(("z", "ldj", "ll"), got, want):
                assert np.array_equal(_bits(a), b), f"{gid}/{mode}: {name} of call {k + 2} differs from the first"
    z64, ld64, ll64 = _oracle64(gid)
    e_ld, e_ll = rel_err(first[1].cpu().numpy(), ld64), rel_err(first[2].cpu().numpy(), ll64)
    print(f"{gid}/{mode}: deterministic mode vs float64: ldj {e_ld:.3e}, ll {e_ll:.3e}")
    assert e_ld < LL_RTOL and e_ll < LL_RTOL
    assert np.array_equal(_bits(first[0]), _bits(z_off)), "the mode touched z"
    # (the mode-off values of the same handle: the same sums in another order)
    assert rel_err(ldj_off.cpu().numpy(), ld64) < LL_RTOL and rel_err(ll_off.cpu().numpy(), ll64) < LL_RTOL


def test_geometry_t_runs_on_the_exact_f32_convolutions():
    """Geometry T on a `default` handle: neither split-f16 form takes it (see GEOMETRIES), so in deterministic mode it gives the
    `f32` handle's bits -- the same launches, the same slots."""
    x, noise = _batch("T")
    xd, nd = _to(x), _to(noise)
    a, b = _flow("T", "default"), _flow("T", "f32")
    with _det(a, b):
        for u, v in zip(a.forward(xd, nd), b.forward(xd, nd)):
            assert np.array_equal(_bits(u), _bits(v))


@pytest.mark.parametrize("mode", MODES)
@pytest.mark.parametrize("gid", ("G", "F"))
def test_an_image_does_not_depend_on_the_batch(gid, mode):
    """2. Image i alone (n = 1), at position 3 of a batch of 5, at position 41 of a batch of 70 and at position 7 of ANOTHER batch of 70,
    the other images different every time: wherever z of the image is bit-equal between two of these, ldj and ll are too.
    n = 1 against n = 5 and the two batches of 70 run the same kernels and must agree in z as well.  Between n <= 5 and n = 70 the
    1x1 mixes of the 16-wide level change kernel in the unchanged default path (img_mix_kernel from 8192 pixels per launch on, the
    implicit-GEMM form below): z of the two may differ in the last bits, mode on or off -- such a pair is reported, not compared."""
    flow = _flow(gid, mode)
    xi, ni = _batch(gid, 1, seed=411)

    def embedded(n, pos, seed):
        x, noise = (a.copy() for a in _batch(gid, n, seed=seed))
        x[pos], noise[pos] = xi[0], ni[0]
        return _to(x), _to(noise), pos

    runs = {"n=1": (_to(xi), _to(ni), 0), "3 of 5": embedded(5, 3, 412), "41 of 70": embedded(70, 41, 413), "7 of 70": embedded(70, 7, 414)}
    got = {}
    with _det(flow):
        for name, (xd, nd, pos) in runs.items():
            z, ldj, ll = flow.forward(xd, nd)
            got[name] = (_bits(z[pos]), _bits(ldj[pos:pos + 1]), _bits(ll[pos:pos + 1]))
    assert tuple(got["n=1"][0].shape) == tuple(_flow(gid, mode).z_shape)
    must = {("n=1", "3 of 5"), ("41 of 70", "7 of 70")}
    names = list(runs)
    for i, a in enumerate(names):
        for b in names[i + 1:]:
            z_equal = np.array_equal(got[a][0], got[b][0])
            if (a, b) in must:
                assert z_equal, f"{gid}/{mode}: z of the image differs between '{a}' and '{b}'"
            if not z_equal:
                print(f"{gid}/{mode}: z differs between '{a}' and '{b}' (the 1x1 mixes change kernel with n): ldj / ll not compared")
                continue
            assert np.array_equal(got[a][1], got[b][1]), f"{gid}/{mode}: ldj of the image differs between '{a}' and '{b}'"
            assert np.array_equal(got[a][2], got[b][2]), f"{gid}/{mode}: ll of the image differs between '{a}' and '{b}'"


def _blow_up_hidden(sp, step=0, gain_logs=12.0):
    """The out-of-range recipe of tests/test_hip_image.py: the first convolution's ActNorm2d of one coupling net scales every hidden
    channel by e^gain_logs, the last convolution's weights shrink by the same factor -- the exact result stays ordinary."""
    sp = copy.deepcopy(sp)
    net = sp["levels"][0]["steps"][step]["convs"]
    net[0]["an_logs"] = net[0]["an_logs"] + np.float32(gain_logs)
    net[-1]["w"] = (net[-1]["w"] * np.float32(np.exp(-gain_logs))).astype(np.float32)
    return sp


@pytest.mark.parametrize("gid", ("G", "F"))
def test_repaired_images_equal_the_exact_f32_handle(gid, monkeypatch):
    """4. A split-f16 handle (probe off) whose every image leaves the fp16 range: mode on, 12 identical calls are bit-equal, the
    images were repaired in the same call, and each repaired image's ldj / ll -- and z -- equal those of an `f32` handle in
    deterministic mode bit for bit: the repair adds the exact-f32 sequence's slots in the exact-f32 handle's order."""
    import torch
    from gbnf_amd import native
    monkeypatch.setenv("GBNF_IMAGE_NO_PROBE", "1")
    native.tuning_set("check_every", -1)           # (range protocol alone, as in the recipe)
    try:
        sp = _blow_up_hidden(_spec(gid))
        flow = native.NativeImageFlow(sp)
        assert native.MATH_NAME[int(flow.numerics().math_mode)] == "f16x3"
        exact = native.NativeImageFlow(sp, math="f32")
        n = GEOMETRIES[gid][2]
        x, noise = _batch(gid)
        xd, nd = _to(x), _to(noise)
        flow.deterministic = True
        exact.deterministic = True
        first = [_bits(t) for t in flow.forward(xd, nd)]
        rc = flow.repair_counts()
        assert rc["marked_calls"] == 1 and rc["repaired_images"] == n, rc
        for k in range(11):
            for name, a, b in zip(("z", "ldj", "ll"), flow.forward(xd, nd), first):
                assert np.array_equal(_bits(a), b), f"{gid}: {name} of call {k + 2} differs from the first"
        assert flow.repair_counts()["repaired_images"] == 12 * n
        assert native.MATH_NAME[int(flow.numerics().math_mode)] == "f16x3" and not flow.numerics().demoted
        for name, a, b in zip(("z", "ldj", "ll"), exact.forward(xd, nd), first):
            assert np.array_equal(_bits(a), b), f"{gid}: {name} of the repaired images differs from the exact-f32 handle's"
    finally:
        native.tuning_set("check_every", 256)


@pytest.mark.parametrize("mode", MODES)
def test_workspace_sizes_and_the_refusal(mode):
    """5. The size query answers more while the mode is on; a call with the mode-off size is refused (GBNF_ERR_INVALID, a message
    naming the mode) and writes nothing; after switching off the smaller size is accepted again."""
    import torch
    from gbnf_amd import native
    flow, lib = _flow("G", mode), native.lib()
    x, noise = _batch("G")
    xd, nd = _to(x), _to(noise)
    n = xd.shape[0]

    def size():
        nb = C.c_int64()
        assert lib.gbnf_image_flow_workspace_bytes(flow.handle, n, C.byref(nb)) == 0
        return nb.value

    def call(ws, nbytes, ldj, ll):
        p = lambda t: C.c_void_p(t.data_ptr())
        return lib.gbnf_image_flow_forward(flow.handle, p(xd), p(nd), n, C.c_void_p(0), p(ldj), p(ll), p(ws), nbytes, native._stream_ptr())

    small = size()
    with _det(flow):
        large = size()
        assert large > small
        ws = torch.zeros((large + 3) // 4, dtype=torch.float32, device=_dev())
        ldj, ll = (torch.full((n,), 777.0, device=_dev()) for _ in range(2))
        rc = call(ws, small, ldj, ll)
        torch.cuda.synchronize()
        msg = lib.gbnf_last_error().decode(errors="replace")
        assert rc == -1 and "deterministic mode" in msg, (rc, msg)                 # GBNF_ERR_INVALID
        assert bool((ldj == 777.0).all()) and bool((ll == 777.0).all()) and bool((ws == 0).all())
        assert call(ws, large, ldj, ll) == 0
        torch.cuda.synchronize()
        want = _bits(ll)
        assert np.isfinite(ll.cpu().numpy()).all()
    assert size() == small
    ldj.fill_(777.0); ll.fill_(777.0)
    assert call(ws, small, ldj, ll) == 0
    torch.cuda.synchronize()
    assert bool((ll != 777.0).all())
    assert (np.abs(ll.cpu().numpy() - want.view(np.float32)) <= 128 * 2.0 ** -24 * np.abs(want.view(np.float32))).all()


def test_default_mode_is_unchanged():
    """6. A handle whose mode was switched on and off again gives the z of a handle that never saw the switch, and ldj inside the
    128 * 2^-24 relative allowance of the atomic sums (tests/test_hip_image_train.py)."""
    import torch
    from gbnf_amd import native
    x, noise = _batch("G")
    xd, nd = _to(x), _to(noise)
    fresh = native.NativeImageFlow(_spec("G"))
    assert fresh.deterministic is False
    z0, ldj0, ll0 = fresh.forward(xd, nd)
    flow = _flow("G", "default")
    with _det(flow):
        flow.forward(xd, nd)
    z1, ldj1, ll1 = flow.forward(xd, nd)
    assert np.array_equal(_bits(z0), _bits(z1))
    for a, b in ((ldj1, ldj0), (ll1, ll0)):
        assert bool(((a - b).abs() <= 128 * 2.0 ** -24 * b.abs()).all()), float((a - b).abs().max())


def test_forward_y_repeats_bit_equal():
    """7. A class-conditional component (G with 10 classes): ll and y_logits of gbnf_image_flow_forward_y are bit-equal over 12
    repeats with the mode on, and ll meets the mode-off value inside the atomic sums' allowance."""
    import torch
    from gbnf_amd import native
    flow = native.NativeImageFlow(_spec("G", 10))
    assert flow.y_classes == 10 and flow.has_class_head
    x, noise = _batch("G")
    xd, nd = _to(x), _to(noise)
    y = torch.zeros((xd.shape[0], 10), dtype=torch.float32, device=_dev())
    y[torch.arange(xd.shape[0]), torch.tensor([3, 0, 9, 3])] = 1.0
    _, _, ll_off, logits_off = flow.forward(xd, nd, y=y)
    flow.deterministic = True
    want = [_bits(t) for t in flow.forward(xd, nd, y=y)]
    for k in range(11):
        for name, a, b in zip(("z", "ldj", "ll", "y_logits"), flow.forward(xd, nd, y=y), want):
            assert np.array_equal(_bits(a), b), f"{name} of call {k + 2} differs from the first"
    assert np.array_equal(want[3], _bits(logits_off))                    # (the logits come from z alone)
    ll_on = torch.from_numpy(want[2].view(np.float32))
    assert bool(((ll_on - ll_off.cpu()).abs() <= 128 * 2.0 ** -24 * ll_off.cpu().abs()).all())


_TWO_KERNEL = r"""
import sys
import numpy as np, torch
sys.path.insert(0, sys.argv[1])
from gbnf_amd import native, synth
from oracle import gbnf_oracle as oracle
sp = synth.synth_image_glow_spec((3, 32, 32), seed=23, h=32, K=2, L=2)
x, noise = synth.synth_image_batch(4, (3, 32, 32), seed=300)
xd, nd = torch.from_numpy(x).cuda(), torch.from_numpy(noise).cuda()
flow = native.NativeImageFlow(sp)
assert native.MATH_NAME[int(flow.numerics().math_mode)] == "f16x3" and not flow.numerics().demoted
z_off = flow.forward(xd, nd)[0]
flow.deterministic = True
first = [t.cpu().numpy().view(np.uint32) for t in flow.forward(xd, nd)]
for k in range(23):
    for a, b in zip(flow.forward(xd, nd), first):
        assert np.array_equal(a.cpu().numpy().view(np.uint32), b), k
assert np.array_equal(first[0], z_off.cpu().numpy().view(np.uint32))
ll64 = np.asarray(oracle.image_component_forward(sp, x, noise, dtype=torch.float64)[4], dtype=np.float64)
err = float(np.max(np.abs(first[2].view(np.float32) - ll64) / np.maximum(np.abs(ll64), 1.0)))
assert err < 1e-5, err
print("two-kernel form ok", err)
"""


def test_the_two_kernel_form():
    """img_last_hx3_kernel's slot store.  No geometry reaches the two-kernel form (img_mid_hx3 + img_last_hx3) while the fused kernel
    takes it; the library's diagnostic switch GBNF_IMG_NO_FUSE, read once per process, sends geometry G there -- hence a process of
    its own: mode on, 24 identical calls bit-equal, z untouched, ll at the project's bar."""
    env = dict(os.environ, GBNF_IMG_NO_FUSE="1")
    r = subprocess.run([sys.executable, "-c", _TWO_KERNEL, REPO], env=env, stdout=subprocess.PIPE, stderr=subprocess.STDOUT, text=True, timeout=300)
    assert r.returncode == 0 and "two-kernel form ok" in r.stdout, r.stdout[-2000:]


# ---- the module, end to end -------------------------------------------------------------------------------------------------------
MODULE_SIZE, MODULE_KW = (1, 16, 16), dict(h=32, K=2, L=2)


def _module(**flags):
    """A freshly constructed 2-component BoostedImageFlow with fixed parameters, at component 1."""
    import torch
    from gbnf_amd import BoostedFlow, image_glow, synth
    torch.manual_seed(0)
    m = BoostedFlow(host.image_args(MODULE_SIZE, MODULE_KW["h"], MODULE_KW["K"], MODULE_KW["L"], _dev(), C_=2, rho_iters=12, rho_lr=0.01))
    for c in range(2):
        image_glow.load_image_spec(m.flows[c], synth.synth_image_glow_spec(MODULE_SIZE, seed=31 + c, **MODULE_KW))
    m.component = 1
    for k, v in flags.items():
        setattr(m, k, v)
    return m


def _boosted_run(m):
    """3 boosted training steps on component 1, update_rho over a 2-batch loader, the rho gradients of both batches: every number
    the run reports, as uint32 views."""
    import torch
    from gbnf_amd import synth
    out = []
    xs = [synth.synth_image_batch(5, MODULE_SIZE, seed=s) for s in (104, 105)]
    m.train()
    for k in range(3):
        x, noise = xs[k % 2]
        stats = m.training_step(_to(x), noise=_to(noise), lr=LR, fixed=0)
        assert {"G_nll", "boosted_nll", "boosted_bpd"} <= set(stats)
        out += [(f"step {k} {key}", _bits(v.reshape(1)) if hasattr(v, "reshape") else v) for key, v in sorted(stats.items())]
    m.update_rho([(_to(x), None) for x, _ in xs], noise_generator=torch.Generator(device=_dev()).manual_seed(7))
    out.append(("rho", _bits(m.rho)))
    for k, (x, noise) in enumerate(xs):
        for name, t in zip(("new_ll", "fixed_ll", "full_ll"), m._rho_gradients(_to(x), _to(noise))):
            out.append((f"rho gradients {k} {name}", _bits(t)))
    return out


def test_two_identical_boosted_runs_are_bit_equal():
    """8. Two freshly constructed identical models with image_deterministic and image_eval_deterministic on: the statistics of
    every boosted step (the fixed-mixture terms included), the final rho and every _rho_gradients triple agree bit for bit."""
    runs = [_boosted_run(_module(image_deterministic=True, image_eval_deterministic=True)) for _ in range(2)]
    assert [k for k, _ in runs[0]] == [k for k, _ in runs[1]] and len(runs[0]) == 3 * 8 + 1 + 6
    for (key, a), (_, b) in zip(*runs):
        assert np.array_equal(a, b), f"{key}: {a} vs {b}"
    rho = dict(runs[0])["rho"].view(np.float32)
    assert np.isfinite(rho).all() and rho[1] != np.float32(0.5), "update_rho did not move rho[1]"


def test_the_flag_reaches_a_cached_handle():
    """A handle cached before the module's flag was set is switched by the next call that asks for it, and switched back."""
    m = _module()
    m.eval()
    from gbnf_amd import synth
    x, noise = synth.synth_image_batch(5, MODULE_SIZE, seed=104)
    xd, nd = _to(x), _to(noise)
    m.log_prob(xd, noise=nd)
    held = [m.native_flow(c) for c in range(2)]
    assert [h.deterministic for h in held] == [False, False]
    m.image_eval_deterministic = True
    want = _bits(m.log_prob(xd, noise=nd))
    assert all(m.native_flow(c) is held[c] for c in range(2)) and [h.deterministic for h in held] == [True, True]
    for _ in range(11):
        assert np.array_equal(_bits(m.log_prob(xd, noise=nd)), want)
    m.image_eval_deterministic = False
    m.log_prob(xd, noise=nd)
    assert [h.deterministic for h in held] == [False, False]
