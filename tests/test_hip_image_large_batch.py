"""GPU: the image trainer at multi-image launch shapes (tests/image_large_batch_cases.py: capped and uneven weight-gradient slices,
slices that lie outside the map entirely, the NLL seed on several workgroups per channel, the > 256-channel path with more than one
image, capped ActNorm2d chunks) against the float64 yardsticks of tests/image_grad_oracle.py, tests/image_step_oracle.py and
oracle.image_actnorm_init.

The bars are the existing ones, unchanged: forward z within Z_RTOL = 2e-5 of its largest entry, ldj and the nll within LL_RTOL = 1e-5
relative, every gradient within G_RTOL = 2e-4 of its tensor's largest entry (floor 1e-3), parameters and moments after an update
within PARAM_TOL = 1e-6 x max|tensor| of torch.optim fed the same gradient, ActNorm2d bias / logs within BAR = 1e-5 x max(1, max|ref|).
tests/test_image_large_batch_host.py shows on the host that float32 arithmetic itself stays a factor 20 inside G_RTOL on these cases."""
import numpy as np
import pytest

import image_actnorm_init_cases as aic
import image_grad_oracle as igo
import image_large_batch_cases as T
from test_hip_fused_step import LR, OPT_CASES, STEP_SCALES, _assert_close, _regions, _torch_optimizer, _torch_step
from test_hip_image_fused_step import _trainer as _step_trainer
from test_hip_image_score import _check_gx
from test_hip_image_train import G_RTOL, LL_RTOL, _check_forward, _check_grads

pytestmark = pytest.mark.gpu
assert G_RTOL == T.G_RTOL


def _device():
    import torch
    return torch.device("cuda:0")


def _to(a, dev):
    import torch
    return torch.from_numpy(np.ascontiguousarray(a)).to(dev)


def _inputs(name, dev):
    sp, x, noise, g_z, g_ldj = T.make_case(name)
    return sp, tuple(_to(a, dev) for a in (x, noise, g_z, g_ldj))


# ---- 1. gradients, default mode ---------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("name", sorted(T.CASES))
def test_trainer_matches_yardstick(name):
    """forward z, ldj and every gradient tensor of backward; on W3 and W4 also g_z = None: the log-det path alone."""
    from gbnf_amd import native
    dev = _device()
    sp, (xd, nd, gz, gl) = _inputs(name, dev)
    tr = native.NativeImageTrainer(igo.dev_spec(sp, dev))
    z, ldj, trace = tr.forward(xd, nd)
    out, ref = T.grads(name)
    _check_forward(z, ldj, out, name)
    _, views = tr.backward(trace, gz, gl)
    _check_grads(views, ref, name)
    if name in ("W3", "W4"):
        _, ref0 = T.grads(name, False)
        _, views0 = tr.backward(trace, None, gl)
        _check_grads(views0, ref0, f"{name} g_z=None")
    tr.close()


# ---- 2. gradients, deterministic mode ---------------------------------------------------------------------------------------------
@pytest.mark.parametrize("name", ["W1", "W3", "W5"])
def test_ordered_trainer_matches_yardstick_and_repeats(name):
    """Capped slices (W1, W5), slices without an item inside the map, whose zeros the reduce adds (W3, W5), the reduce loop over
    whole eights and with a tail: the right answer, bit-equal from round to round -- the second round on a workspace filled with NaN,
    so that a partial nobody stored is seen -- and the slice counts of the restatement are the library's."""
    import torch
    from gbnf_amd import native
    dev = _device()
    sp, (xd, nd, gz, gl) = _inputs(name, dev)
    n = xd.shape[0]
    tr = native.NativeImageTrainer(igo.dev_spec(sp, dev), deterministic=True)
    on = tr.workspace_bytes(n)
    tr.deterministic = False
    off = tr.workspace_bytes(n)
    tr.deterministic = True
    print(f"{name}: workspace {off} -> {on} bytes; restated partials {T.det_extra_bytes(name)}")
    assert on - off == T.det_extra_bytes(name)
    out, ref = T.grads(name)
    z, ldj, trace = tr.forward(xd, nd)
    _check_forward(z, ldj, out, f"{name} ordered")
    flat, views = tr.backward(trace, gz, gl)
    _check_grads(views, ref, f"{name} ordered")
    z2, ldj2, trace2 = tr.forward(xd, nd)
    tr._ws.fill_(float("nan"))
    flat2, _ = tr.backward(trace2, gz, gl)
    torch.cuda.synchronize()
    assert torch.equal(z, z2) and torch.equal(ldj, ldj2) and torch.equal(trace, trace2)
    assert torch.equal(flat, flat2), f"{name}: {int((flat != flat2).sum())} gradient entries differ between two rounds"
    tr.close()


# ---- 3. the fused step ------------------------------------------------------------------------------------------------------------
def _by_name(views, ref, paths, what):
    for path in paths:
        a, b = views[path].cpu().numpy().astype(np.float64), ref[path]
        scale = max(float(np.abs(b).max()), 1e-3)
        err = float(np.abs(a - b).max()) / scale
        print(f"{what}: {path} error {err:.3e} of {G_RTOL} (largest entry {scale:.3e})")
        assert scale > 0.1, f"{what}: {path} is too small to test"
        assert err <= G_RTOL, f"{what}: {path}"


@pytest.mark.parametrize("name", ["W1", "W2", "W4"])
def test_nll_step_with_zero_lr_matches_the_yardstick(name):
    """The seed on bpc = 10, 4 (capped) and 2 workgroups per channel: the reported nll (nll_part, all bpc x Cz partials), the learned
    top prior's bias and logs gradients (mu_part / lv_part read back as [Cz][bpc]) and the 1x1 matrices' gradients by name, every
    gradient by the common rule; parameters bit-identical at lr = 0."""
    import torch
    from gbnf_amd import native
    dev = _device()
    sp, (xd, nd, _, _) = _inputs(name, dev)
    nll, ref = T.step_yardstick(name)
    tr, tensors = _step_trainer(sp, dev)
    before = {p: t.clone() for p, t in tensors.items()}
    stats, flat = tr.nll_step(xd, nd, native.OptState(tr, "adamw"), lr=0.0, weight_decay=1e-5, max_grad_norm=50.0)
    stats = stats.cpu()
    print(f"{name}: nll {float(stats[0])} vs {nll}: {abs(float(stats[0]) - nll) / abs(nll):.3e} of {LL_RTOL}")
    assert abs(float(stats[0]) - nll) <= LL_RTOL * abs(nll)
    views = tr.step_views(flat)
    _by_name(views, ref, [("learn_top", "b"), ("learn_top", "logs")] + [p for p in ref if p[-1] == "perm_w"], name)
    _check_grads(views, ref, f"{name} step")
    for p, t in tensors.items():
        assert torch.equal(t, before[p]), p
    norm = float(flat.double().norm())
    assert abs(float(stats[1]) - norm) <= 1e-5 * norm
    tr.close()


def test_a_step_is_its_parts():
    """W4, AdamW with weight decay and clipping at a non-zero learning rate: five nll_step calls against a CPU torch.optim twin fed
    the gradients the calls returned (the protocol of test_hip_image_fused_step.test_a_step_is_its_parts), and the first call's
    gradient against the yardstick."""
    import torch
    from gbnf_amd import native
    cfg = OPT_CASES["adamw_wd_clip"]
    dev = _device()
    sp, (xd, nd, _, _) = _inputs("W4", dev)
    _, ref = T.step_yardstick("W4")
    tr, _ = _step_trainer(sp, dev)
    probe, _ = tr.nll_step(xd, nd, native.OptState(tr, "sgd"), lr=0.0)
    max_norm = 0.5 * float(probe[1])
    regions = _regions(tr)
    live = [r for r in regions if r[2] is not None]
    assert len(live) == len(regions)
    clones = [t.detach().cpu().clone().requires_grad_(True) for _, _, t in live]
    opt = _torch_optimizer(clones, cfg["kind"], LR, cfg["weight_decay"])
    state = native.OptState(tr, cfg["kind"])
    coefs = []
    for it, k in enumerate(STEP_SCALES):
        stats, flat = tr.nll_step(xd, nd, state, loss_scale=k, lr=LR, weight_decay=cfg["weight_decay"], max_grad_norm=max_norm)
        if it == 0:
            _check_grads(tr.step_views(flat), ref, "W4 first step")
        stats = stats.cpu()
        norm, coef = _torch_step(opt, clones, regions, flat.cpu(), max_norm)
        assert abs(float(stats[1]) - norm) <= 1e-5 * norm, f"step {it}: norm {float(stats[1])} vs {norm}"
        assert abs(float(stats[2]) - coef) <= 1e-5, f"step {it}: coefficient {float(stats[2])} vs {coef}"
        coefs.append(coef)
    assert state.step == 5 and min(coefs) < 1.0 and max(coefs) == 1.0
    m_views, v_views = state.views()
    for idx, ((off, size, t), clone) in enumerate(zip(regions, clones)):
        _assert_close(t, clone, f"parameter {idx}")
        _assert_close(m_views[idx], opt.state[clone]["exp_avg"], f"exp_avg {idx}")
        _assert_close(v_views[idx], opt.state[clone]["exp_avg_sq"], f"exp_avg_sq {idx}")
    tr.close()


# ---- 4. input gradients -----------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("name", ["W4", "W5"])
def test_backward_x_matches_yardstick(name):
    from gbnf_amd import native
    dev = _device()
    sp, (xd, nd, gz, gl) = _inputs(name, dev)
    tr = native.NativeImageTrainer(igo.dev_spec(sp, dev))
    _, _, trace = tr.forward(xd, nd)
    _check_gx(tr.backward_x(trace, xd, nd, gz, gl), T.input_grad(name), name)
    tr.close()


# ---- 5. the one-pass ActNorm2d init -----------------------------------------------------------------------------------------------
def _init(name):
    import torch
    from gbnf_amd import native
    sp, x, noise = T.make_init(name)
    dev = _device()
    ds = igo.dev_spec(sp, dev)
    tr = native.NativeImageTrainer(ds)
    tr.actnorm_init(_to(x, dev), _to(noise, dev))
    torch.cuda.synchronize()
    tr.close()
    return [(b.detach().cpu().numpy().reshape(-1), l.detach().cpu().numpy().reshape(-1)) for b, l in aic.spec_actnorms(ds)]


@pytest.mark.parametrize("name", sorted(T.INIT_CASES))
def test_fused_init_matches_float64_oracle(name):
    """A1: 33 chunks at the 64-chunk cap, the last of 3 images; A2: two chunks of 16 and 7 images on the 8 x 8 level.  A1 twice:
    the chunk order is fixed, the two results are bit-equal."""
    got = _init(name)
    w = aic.worst(got, T.init_oracle(name))
    print(f"{name}: worst bias / logs error against float64 {w:.3e} of {aic.BAR}")
    assert w <= aic.BAR
    if name == "A1":
        again = _init(name)
        assert all(np.array_equal(b, b2) and np.array_equal(l, l2) for (b, l), (b2, l2) in zip(got, again))
