"""GPU: deterministic mode of the image trainer (gbnf_image_trainer_set_deterministic, native.NativeImageTrainer(deterministic=True),
BoostedImageFlow.image_deterministic): the ordered weight-gradient and log-det sums give the right answer (the float64 yardstick of
tests/image_grad_oracle.py, the bars of tests/test_hip_image_train.py), and forward / backward / nll_step / boosted_nll_step are
bit-identical from call to call and from trainer to trainer.

"Geometry B with 9 images" (tests/test_image_deterministic_host.py: kink-free for seed 6): every weight-gradient launch of it has 3 to
18 slices, so the order of the partial sums matters in every layer."""
import ctypes as C
import functools

import numpy as np
import pytest

import image_grad_oracle as igo
import image_step_oracle as iso
from conftest import rel_err
from test_image_deterministic_host import b9_case

pytestmark = pytest.mark.gpu
G_RTOL = 2e-4
Z_RTOL = 2e-5
LL_RTOL = 1e-5


def _dev():
    import torch
    return torch.device("cuda:0")


def _to(a, dev):
    import torch
    return torch.from_numpy(np.ascontiguousarray(a)).to(dev)


def _case(key):
    """key: ("B9", seed) = geometry B with 9 images, else a listed (name, seed) of image_grad_oracle.CASES."""
    return b9_case(key[1]) if key[0] == "B9" else igo.make_case(*key)


@functools.lru_cache(maxsize=None)
def _yardstick(key, with_gz=True):
    """(spec, x, noise, g_z, g_ldj, out, ref) of a case: float64, computed once, shared, left unchanged."""
    sp, x, noise = _case(key)
    n = x.shape[0]
    rng = np.random.RandomState(1000 + key[1])
    C_, H, W = sp["input_size"]
    L = len(sp["levels"])
    zshape = (n, C_ * 4 ** L // 2 ** (L - 1), H >> L, W >> L)
    g_z = rng.standard_normal(zshape).astype(np.float32)
    g_ldj = rng.standard_normal(n).astype(np.float32)
    out, ref = igo.grads(sp, x, noise, g_z if with_gz else None, g_ldj)
    assert tuple(out["z"].shape) == zshape
    return sp, x, noise, g_z, g_ldj, out, ref


def _check_forward(z, ldj, out, what):
    zr, lr = out["z"].numpy(), out["ldj_noperm"].numpy()
    ez = float(np.abs(z.cpu().numpy() - zr).max()) / float(np.abs(zr).max())
    el = rel_err(ldj.cpu().numpy(), lr)
    print(f"{what}: forward z {ez:.3e} of {Z_RTOL}, ldj {el:.3e} of {LL_RTOL}")
    assert ez <= Z_RTOL, what
    assert el < LL_RTOL, what


def _check_grads(views, ref, what, scale_by=1.0):
    assert set(views) == set(ref)
    worst, where = 0.0, None
    for path, b in ref.items():
        a = views[path].cpu().numpy().astype(np.float64) / scale_by
        assert a.shape == b.shape, path
        scale = max(float(np.abs(b).max()), 1e-3)
        if float(np.abs(a - b).max()) / scale >= worst:
            worst, where = float(np.abs(a - b).max()) / scale, path
    print(f"{what}: worst gradient error {worst:.3e} of {G_RTOL} ({where})")
    for path, b in ref.items():
        a = views[path].cpu().numpy().astype(np.float64) / scale_by
        scale = max(float(np.abs(b).max()), 1e-3)
        assert np.abs(a - b).max() <= G_RTOL * scale, f"{what}: gradient {path} shape {b.shape}: {np.abs(a - b).max()} vs scale {scale}"


def _right_answer(key, deterministic):
    import torch
    from gbnf_amd import native
    sp, x, noise, g_z, g_ldj, out, ref = _yardstick(key)
    dev = _dev()
    tr = native.NativeImageTrainer(igo.dev_spec(sp, dev), deterministic=deterministic)
    assert tr.deterministic is deterministic
    z, ldj, trace = tr.forward(_to(x, dev), _to(noise, dev))
    _check_forward(z, ldj, out, f"{key}")
    _, views = tr.backward(trace, _to(g_z, dev), _to(g_ldj, dev))
    _check_grads(views, ref, f"{key}")
    if key[0] == "B9":                                   # g_z = None: the log-det path alone
        _, ref0 = _yardstick(key, False)[5:]
        _, views0 = tr.backward(trace, None, _to(g_ldj, dev))
        _check_grads(views0, ref0, f"{key} g_z=None")
    tr.close()


# ---- 1. the right answer in the ordered mode
@pytest.mark.parametrize("key", [("B", 1), ("D", 1), ("C", 5), ("E", 5), ("B9", 6)], ids=lambda k: f"{k[0]}-{k[1]}")
def test_ordered_trainer_matches_yardstick(key):
    _right_answer(key, True)


# ---- 2. bit-equal repeats
def _rounds(tr, xd, nd, gz, gl, rounds):
    """[(z, ldj, trace, grads)] of `rounds` forward + backward rounds, each into freshly zeroed grads."""
    out = []
    for _ in range(rounds):
        z, ldj, trace = tr.forward(xd, nd)
        flat, _ = tr.backward(trace, gz, gl)
        out.append((z, ldj, trace, flat))
    return out


@pytest.mark.parametrize("key", [("B9", 6), ("E", 5)], ids=lambda k: f"{k[0]}-{k[1]}")
def test_repeats_are_bit_equal(key):
    import torch
    from gbnf_amd import native
    sp, x, noise, g_z, g_ldj, _, _ = _yardstick(key)
    dev = _dev()
    xd, nd, gz, gl = (_to(a, dev) for a in (x, noise, g_z, g_ldj))
    ds = igo.dev_spec(sp, dev)
    tr = native.NativeImageTrainer(ds, deterministic=True)
    got = _rounds(tr, xd, nd, gz, gl, 5)
    tr2 = native.NativeImageTrainer(ds, deterministic=True)          # a second trainer on the same tensors
    got += _rounds(tr2, xd, nd, gz, gl, 1)
    torch.cuda.synchronize()
    assert float(got[0][3].abs().max()) > 0.0
    for r, row in enumerate(got[1:], 1):
        for name, a, b in zip(("z", "ldj", "trace", "grads"), got[0], row):
            assert torch.equal(a, b), f"{key}: {name} of round {r} differs from round 0 in {int((a != b).sum())} entries"


# ---- 3. accumulation
def test_two_ordered_backward_calls_accumulate():
    import torch
    from gbnf_amd import native
    key = ("B9", 6)
    sp, x, noise, g_z, g_ldj, _, ref = _yardstick(key)
    dev = _dev()
    xd, nd, gz, gl = (_to(a, dev) for a in (x, noise, g_z, g_ldj))
    tr = native.NativeImageTrainer(igo.dev_spec(sp, dev), deterministic=True)
    _, _, trace = tr.forward(xd, nd)
    pairs = []
    for _ in range(2):
        flat, _ = tr.backward(trace, gz, gl)
        flat, views = tr.backward(trace, gz, gl, out=flat)
        _check_grads(views, ref, "accumulated", scale_by=2.0)
        pairs.append(flat)
    assert torch.equal(pairs[0], pairs[1])


# ---- 4. workspace
def _largest_region(sp):
    """Floats of the largest per-convolution (dW', db') region of a spec: its convolutions and the C x C mixes of its steps."""
    worst = 0
    for lv in sp["levels"]:
        for st in lv["steps"]:
            c = st["an_bias"].size
            worst = max(worst, c * c + c)
            for cv in st["convs"]:
                worst = max(worst, cv["w"].size + cv["w"].shape[0])
        if lv["split"] is not None:
            worst = max(worst, lv["split"]["w"].size + lv["split"]["w"].shape[0])
    return worst


def _last_error():
    from gbnf_amd import native
    L = native.lib()
    L.gbnf_last_error.restype = C.c_char_p
    return (L.gbnf_last_error() or b"").decode()


def test_workspace_grows_and_a_small_one_is_refused():
    import torch
    from gbnf_amd import native
    sp, x, noise, g_z, g_ldj, _, _ = _yardstick(("B9", 6))
    n = x.shape[0]
    dev = _dev()
    xd, nd, gz, gl = (_to(a, dev) for a in (x, noise, g_z, g_ldj))
    tr = native.NativeImageTrainer(igo.dev_spec(sp, dev))
    off, off_step = tr.workspace_bytes(n), tr.step_workspace_bytes(n)
    _, _, trace = tr.forward(xd, nd)
    tr.deterministic = True
    assert tr.deterministic is True
    on, on_step = tr.workspace_bytes(n), tr.step_workspace_bytes(n)
    print(f"workspace {off} -> {on}, step {off_step} -> {on_step}, largest region {_largest_region(sp)} floats")
    assert on > off and on_step > off_step
    assert on - off >= 2 * 4 * _largest_region(sp)
    L = native.lib()
    ptr = lambda t: C.c_void_p(t.data_ptr())
    ws = torch.empty(off // 4 + 1, dtype=torch.float32, device=dev)
    grads = torch.full((tr.step_grad_floats,), 123.0, device=dev)
    rc = L.gbnf_image_trainer_backward(tr.handle, ptr(trace), n, ptr(gz), ptr(gl), ptr(grads), ptr(ws), off, None)
    torch.cuda.synchronize()
    assert rc == -1 and "workspace too small" in _last_error()
    assert bool((grads == 123.0).all()), "the refused backward wrote to grads"
    ws = torch.empty(off_step // 4 + 1, dtype=torch.float32, device=dev)
    stats = torch.full((4,), 7.0, device=dev)
    state = native.OptState(tr, "adamw")
    h = native._OptHyper(kind=native.OPT_KIND["adamw"], step=1, lr=1e-3, beta1=0.9, beta2=0.999, eps=1e-8)
    rc = L.gbnf_image_trainer_nll_step(tr.handle, ptr(xd), ptr(nd), n, 1.0, ptr(grads), ptr(state.exp_avg), ptr(state.exp_avg_sq), C.byref(h),
                                       ptr(stats), ptr(ws), off_step, None)
    torch.cuda.synchronize()
    assert rc == -1 and "workspace too small" in _last_error()
    assert bool((grads == 123.0).all()) and bool((stats == 7.0).all()), "the refused step wrote to grads / stats"
    tr.deterministic = False
    assert tr.deterministic is False
    assert (tr.workspace_bytes(n), tr.step_workspace_bytes(n)) == (off, off_step)


# ---- 5. the one-call step
def _step_trainer(sp, dev):
    """test_hip_image_fused_step._trainer with the mode on: (trainer, {path: tensor}) on fresh device copies of the spec's arrays."""
    from gbnf_amd import native
    ds, top = iso.dev_spec_top(sp, dev)
    tr = native.NativeImageTrainer(ds, deterministic=True)
    if top is not None:
        tr.bind_top(top["w"], top["b"], top["logs"])
    return tr, {path: t for (path, _, _), t in zip(tr._step_regions, tr.params) if t is not None}


@pytest.mark.parametrize("boosted", [False, True], ids=["nll_step", "boosted_nll_step"])
def test_steps_from_equal_states_stay_bit_equal(boosted):
    import torch
    from gbnf_amd import native, synth
    sp, x, noise = _case(("B9", 6))
    dev = _dev()
    xd, nd = _to(x, dev), _to(noise, dev)
    fixed = native.NativeImageFlow(synth.synth_image_glow_spec((1, 16, 16), seed=2, h=32, K=2, L=2), math="f32") if boosted else None
    runs = []
    for _ in range(2):
        tr, tensors = _step_trainer(sp, dev)
        state = native.OptState(tr, "adamw")
        hist = []
        for _ in range(3):
            if boosted:
                stats, flat = tr.boosted_nll_step(fixed, xd, nd, state, lr=1e-3, max_grad_norm=5.0)
            else:
                stats, flat = tr.nll_step(xd, nd, state, lr=1e-3, max_grad_norm=5.0)
            snap = {"stats": stats[:4].clone(), "exp_avg": state.exp_avg.clone(), "exp_avg_sq": state.exp_avg_sq.clone()}
            if not boosted:
                snap["grads"] = flat.clone()
            snap.update({str(p): t.clone() for p, t in tensors.items()})
            hist.append(snap)
        runs.append(hist)
    torch.cuda.synchronize()
    assert not torch.equal(runs[0][0]["exp_avg"], runs[0][2]["exp_avg"]), "the steps did not move the state"
    assert bool(torch.isfinite(runs[0][2]["stats"]).all())
    for step, (a, b) in enumerate(zip(*runs)):
        assert set(a) == set(b)
        for name in a:
            assert torch.equal(a[name], b[name]), f"step {step}: {name} differs in {int((a[name] != b[name]).sum())} entries"


# ---- 6. the default mode is what it was
def _default_workspace_bytes(sp, n):
    """gbnf_image_trainer_workspace_bytes of the default mode, by hand (the layout at the head of the host side of
    csrc/gbnf_image_train.hip): 6 hidden-wide tensors, one of 64 channels, two states, g_ldj, the (dW', db') scratch."""
    up = lambda v: (v + 63) // 64 * 64
    hid = (sp["hidden"] + 15) // 16 * 16 * 256 * n
    C_, H, W = sp["input_size"]
    state, scr = C_ * 32 * 32, 0
    c, hs, wsz = C_, 32, 32
    for lv in sp["levels"]:
        c, hs, wsz = c * 4, max(hs // 2, 8), max(wsz // 2, 8)
        state = max(state, c * hs * wsz)
        for st in lv["steps"]:
            scr += c * c + c + sum(cv["w"].size + cv["w"].shape[0] for cv in st["convs"])
        if lv["split"] is not None:
            scr += lv["split"]["w"].size + lv["split"]["w"].shape[0]
            c //= 2
    return 4 * (6 * hid + 64 * 256 * n + 2 * state * n + up(n) + up(scr)) + 256


# gbnf_image_trainer_step_workspace_bytes of case B at its 3 images, as a library built from the commit before this mode existed
# reports it: z (3 x 128 floats), ldj, the trace (3 x 7680 floats), g_z, g_ldj, the workspace above and 4 x 256 doubles of partial
# sums, each 256-byte aligned: 1536 + 256 + 92160 + 1536 + 256 + 871680 + 8192
PARENT_STEP_WORKSPACE_BYTES = 975616


def test_default_mode_is_unchanged():
    from gbnf_amd import native
    sp, x, _ = _case(("B", 1))
    n = x.shape[0]
    tr = native.NativeImageTrainer(igo.dev_spec(sp, _dev()))
    assert tr.deterministic is False
    print(f"B/1: gbnf_image_trainer_workspace_bytes = {tr.workspace_bytes(n)}, step {tr.step_workspace_bytes(n)}")
    assert tr.workspace_bytes(n) == _default_workspace_bytes(sp, n) == 871680
    assert tr.step_workspace_bytes(n) == PARENT_STEP_WORKSPACE_BYTES
    tr.close()
    _right_answer(("B", 1), False)


# ---- 7. the module
def _g21(dev, **flags):
    import torch
    cfg, data = igo.g21_load(igo.G21[0])
    torch.manual_seed(21)                   # (the module draws base_dist_mean at construction: two modules are to be identical)
    m = igo.g21_module(cfg, data, dev)
    for k, v in flags.items():
        setattr(m, k, v)
    x, noise = (_to(np.asarray(data[k], dtype=np.float32), dev) for k in ("x", "noise"))
    return m, x, noise


def test_module_trains_bit_reproducibly(monkeypatch):
    import torch
    monkeypatch.setenv("GBNF_IMAGE_DETERMINISTIC", "1")
    dev = _dev()
    states = []
    for _ in range(2):
        m, x, noise = _g21(dev)
        assert m.image_deterministic is True and m.deterministic is False
        m.train()
        for _ in range(3):
            out = m.training_step(x, noise=noise, lr=1e-3)
        assert torch.isfinite(out["nll"]).item()
        assert m.native_trainer(0)[0].deterministic is True
        states.append({k: v.detach().clone() for k, v in m.state_dict().items()})
    assert set(states[0]) == set(states[1])
    for k in states[0]:
        assert torch.equal(states[0][k], states[1][k]), f"{k} differs"


def test_module_flag_reaches_cached_trainers():
    import torch
    dev = _dev()
    m, x, noise = _g21(dev)
    assert m.image_deterministic is False
    m.train()
    m.training_step(x, noise=noise, lr=0.0)
    tr = m.native_trainer(0)[0]
    assert tr.deterministic is False
    m.image_deterministic = True
    assert m.native_trainer(0)[0] is tr and tr.deterministic is True          # the cached trainer, switched
    assert torch.isfinite(m.training_step(x, noise=noise, lr=0.0)["nll"]).item()
    m.image_deterministic = False
    assert m.native_trainer(0)[0] is tr and tr.deterministic is False


def test_deterministic_alone_is_still_refused():
    from gbnf_amd import native
    m, x, noise = _g21(_dev(), deterministic=True)
    assert m.image_deterministic is False
    m.train()
    with pytest.raises(native.GbnfError, match="deterministic") as e:
        m.training_step(x, noise=noise, lr=0.0)
    assert "image_deterministic" in str(e.value)
    m.image_deterministic = True                                              # both set: the ordered path serves the call
    m.training_step(x, noise=noise, lr=0.0)
    assert m.native_trainer(0)[0].deterministic is True
