"""GPU: the input gradients of the image path and the mixture's score (gbnf_image_trainer_backward_x, gbnf_image_score_seed,
gbnf_mixture_responsibilities, gbnf_image_mixture_score; BoostedImageFlow.component_score / score / responsibilities) against the
float64 yardstick tests/image_grad_oracle.py::forward with x a leaf.  The bars are the project's own (tests/test_hip_image_train.py):
gradients within G_RTOL = 2e-4 of the tensor's largest entry (floor 1e-3), log-densities within LL_RTOL = 1e-5 relative."""
import functools

import numpy as np
import pytest

import image_grad_oracle as igo
import image_score_cases as isc
from conftest import rel_err

pytestmark = pytest.mark.gpu
G_RTOL = 2e-4
LL_RTOL = 1e-5


def _dev(a, dev):
    import torch
    return None if a is None else torch.from_numpy(np.ascontiguousarray(np.asarray(a, dtype=np.float32))).to(dev)


def _check_gx(got, ref, what):
    a = got.detach().cpu().numpy().astype(np.float64)
    assert a.shape == ref.shape, what
    scale = max(float(np.abs(ref).max()), 1e-3)
    err = float(np.abs(a - ref).max()) / scale
    print(f"{what}: g_x error {err:.3e} of {G_RTOL} (largest entry {scale:.3e})")
    assert err <= G_RTOL, what


def _yard_gx(sp, x, noise, g_z, g_ldj):
    """float64: d (sum g_z z + sum g_ldj ldj_noperm) / dx (g_z / g_ldj None = zero; noise None = zero)."""
    import torch
    xl = torch.tensor(np.asarray(x), dtype=torch.float64, requires_grad=True)
    out = igo.forward(sp, igo.leaf_params(sp), xl, np.zeros_like(x) if noise is None else noise)
    loss = torch.zeros((), dtype=torch.float64)
    if g_z is not None:
        loss = loss + (torch.as_tensor(g_z, dtype=torch.float64) * out["z"]).sum()
    if g_ldj is not None:
        loss = loss + (torch.as_tensor(g_ldj, dtype=torch.float64) * out["ldj_noperm"]).sum()
    loss.backward()
    return xl.grad.numpy()


# ---------------------------------------------------------------------------------------------------------------------
# the trainer: gbnf_image_trainer_backward_x
# ---------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("name,seed", igo.CASE_SEEDS)
def test_backward_x_matches_yardstick(name, seed):
    """The same random g_z and g_ldj as test_trainer_matches_yardstick; at the first seed of every case also g_z=None, g_ldj=None,
    the accumulate flag (two calls equal the sum) and the data-gradient-only form (bit-equal g_x)."""
    import torch
    from gbnf_amd import native
    sp, x, noise = igo.make_case(name, seed)
    dev = torch.device("cuda:0")
    tr = native.NativeImageTrainer(igo.dev_spec(sp, dev))
    xd, nd = _dev(x, dev), _dev(noise, dev)
    z, ldj, trace = tr.forward(xd, nd)
    rng = np.random.RandomState(1000 + seed)
    g_z = rng.standard_normal(tuple(z.shape)).astype(np.float32)
    g_ldj = rng.standard_normal(x.shape[0]).astype(np.float32)
    gzd, gld = _dev(g_z, dev), _dev(g_ldj, dev)
    g_x = tr.backward_x(trace, xd, nd, gzd, gld)
    _check_gx(g_x, _yard_gx(sp, x, noise, g_z, g_ldj), f"{name}/{seed}")
    if seed != igo.CASES[name][3][0]:
        tr.close()
        return
    g_x2, flat, views = tr.backward_x(trace, xd, nd, gzd, gld, want_grads=True)
    assert torch.equal(g_x2, g_x), "g_x with and without the weight gradients"
    _, ref = igo.grads(sp, x, noise, g_z, g_ldj)
    for path, b in ref.items():
        a = views[path].cpu().numpy().astype(np.float64)
        assert np.abs(a - b).max() <= G_RTOL * max(float(np.abs(b).max()), 1e-3), f"{name}/{seed}: weight gradient {path}"
    _check_gx(tr.backward_x(trace, xd, nd, None, gld), _yard_gx(sp, x, noise, None, g_ldj), f"{name}/{seed} g_z=None")
    _check_gx(tr.backward_x(trace, xd, nd, gzd, None), _yard_gx(sp, x, noise, g_z, None), f"{name}/{seed} g_ldj=None")
    acc = tr.backward_x(trace, xd, nd, gzd, None)
    tr.backward_x(trace, xd, nd, None, gld, g_x=acc)                  # accumulates: the two halves add up to the whole
    _check_gx(acc, _yard_gx(sp, x, noise, g_z, g_ldj), f"{name}/{seed} accumulated")
    twice = g_x.clone()
    tr.backward_x(trace, xd, nd, gzd, gld, g_x=twice)
    assert torch.equal(twice, g_x + g_x)
    tr.close()


@pytest.mark.parametrize("name", ["A", "F"])
def test_backward_x_without_noise(name):
    import torch
    from gbnf_amd import native
    seed = igo.CASES[name][3][0]
    sp, x, _ = igo.make_case(name, seed)
    rows = igo.kink_report(sp, x, np.zeros_like(x))
    assert rows and all(inside == 0 for inside, _ in rows)
    dev = torch.device("cuda:0")
    tr = native.NativeImageTrainer(igo.dev_spec(sp, dev))
    xd = _dev(x, dev)
    z, ldj, trace = tr.forward(xd, None)
    rng = np.random.RandomState(1000 + seed)
    g_z = rng.standard_normal(tuple(z.shape)).astype(np.float32)
    g_ldj = rng.standard_normal(x.shape[0]).astype(np.float32)
    _check_gx(tr.backward_x(trace, xd, None, _dev(g_z, dev), _dev(g_ldj, dev)), _yard_gx(sp, x, None, g_z, g_ldj), f"{name}/{seed} noise=None")
    tr.close()


@pytest.mark.parametrize("name", ["B", "D"])
def test_deterministic_weight_gradients_equal_backward(name):
    """In deterministic mode the weight gradients of backward_x are those of backward to the bit, and g_x repeats."""
    import torch
    from gbnf_amd import native
    seed = igo.CASES[name][3][0]
    sp, x, noise = igo.make_case(name, seed)
    dev = torch.device("cuda:0")
    tr = native.NativeImageTrainer(igo.dev_spec(sp, dev), deterministic=True)
    xd, nd = _dev(x, dev), _dev(noise, dev)
    z, ldj, trace = tr.forward(xd, nd)
    rng = np.random.RandomState(3)
    gzd, gld = _dev(rng.standard_normal(tuple(z.shape)), dev), _dev(rng.standard_normal(x.shape[0]), dev)
    flat, _ = tr.backward(trace, gzd, gld)
    g_x, flat_x, _ = tr.backward_x(trace, xd, nd, gzd, gld, want_grads=True)
    assert torch.equal(flat, flat_x)
    assert torch.equal(g_x, tr.backward_x(trace, xd, nd, gzd, gld))
    tr.close()


# ---------------------------------------------------------------------------------------------------------------------
# the seed kernel and the responsibilities
# ---------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("per_row", [False, True])
@pytest.mark.parametrize("with_r", [False, True])
def test_score_seed_closed_form(per_row, with_r):
    """g_z = -r (z - mu) exp(-logvar), g_ldj = r against float64: f32 arithmetic of four operations, 4 * 2^-24 relative per entry."""
    import torch
    from gbnf_amd import native
    dev = torch.device("cuda:0")
    rng = np.random.RandomState(11)
    n, Cz, H, W = 5, 6, 3, 7
    z = rng.standard_normal((n, Cz, H, W)).astype(np.float32)
    prior = (0.3 * rng.standard_normal((n, 2 * Cz) if per_row else (2 * Cz,))).astype(np.float32)
    r = rng.uniform(0.0, 1.0, size=n).astype(np.float32) if with_r else None
    g_z, g_ldj = native.score_seed(_dev(z, dev), _dev(prior, dev), _dev(r, dev))
    p = np.broadcast_to(prior.astype(np.float64), (n, 2 * Cz))
    rr = np.ones(n) if r is None else r.astype(np.float64)
    ref = -rr[:, None, None, None] * (z.astype(np.float64) - p[:, :Cz, None, None]) * np.exp(-p[:, Cz:, None, None])
    assert np.abs(g_z.cpu().numpy() - ref).max() <= 8 * 2.0 ** -24 * np.abs(ref).max()
    assert np.array_equal(g_ldj.cpu().numpy(), rr.astype(np.float32))
    with pytest.raises(native.GbnfError):
        native.score_seed(_dev(z, dev), _dev(prior.reshape(-1)[: 2 * Cz - 1], dev))


@pytest.mark.parametrize("C", [1, 2, 5])
@pytest.mark.parametrize("N", [1, 63, 65, 257])
def test_responsibilities_against_float64(C, N):
    """softmax and logsumexp over the components in f64, rounded once: half an ulp of the result (+ the f32 rounding of nothing
    else: ll and log_w are the f32 inputs).  Column 0 is all -inf (N > 1), the last column has a single finite entry."""
    import torch
    from gbnf_amd import native
    dev = torch.device("cuda:0")
    rng = np.random.RandomState(100 * C + N)
    ll = (-3000.0 + 4.0 * rng.standard_normal((C, N))).astype(np.float32)
    w = rng.uniform(0.1, 1.0, size=C)
    log_w = np.log(w / w.sum()).astype(np.float32)
    if N > 1:
        ll[:, 0] = -np.inf
    ll[:, N - 1] = -np.inf
    ll[C - 1, N - 1] = -2999.5
    r, G = native.mixture_responsibilities(_dev(ll, dev), _dev(log_w, dev))
    a = torch.from_numpy(ll).double() + torch.from_numpy(log_w).double().view(-1, 1)
    G_ref = torch.logsumexp(a, dim=0).numpy()
    r_ref = torch.softmax(a, dim=0).numpy()
    r_ref[:, ~np.isfinite(G_ref)] = 0.0                              # (torch: NaN out of -inf - -inf; the library: no mass anywhere)
    G, r = G.cpu().numpy(), r.cpu().numpy()
    fin = np.isfinite(G_ref)
    assert np.array_equal(np.isneginf(G), np.isneginf(G_ref)) and not np.isnan(G).any() and not np.isnan(r).any()
    assert np.abs(G[fin] - G_ref[fin]).max() <= 2.0 ** -24 * np.abs(G_ref[fin]).max()
    assert np.abs(r - r_ref).max() <= 2.0 ** -24
    if N > 1:
        assert (r[:, 0] == 0.0).all()
    assert r[C - 1, N - 1] == 1.0 and (r[: C - 1, N - 1] == 0.0).all()


# ---------------------------------------------------------------------------------------------------------------------
# the mixture: gbnf_image_mixture_score on trainers
# ---------------------------------------------------------------------------------------------------------------------
@functools.lru_cache(maxsize=None)
def _mixture_ref(name):
    specs, log_w, x, noise = isc.mixture_case(name)
    return specs, log_w, x, noise, isc.mixture_yardstick(specs, log_w, x, noise)


def _score_trainers(specs, dev, deterministic=False):
    from gbnf_amd import native
    trainers = []
    for sp in specs:
        tr = native.NativeImageTrainer(igo.dev_spec(sp, dev), deterministic=deterministic)
        if sp["learn_top"] is not None:
            tr.bind_top(None, _dev(sp["learn_top"]["b"], dev), _dev(sp["learn_top"]["logs"], dev))
        trainers.append(tr)
    return trainers


def _r_bar(ll):
    """The bar on r that follows from LL_RTOL on ll: r = softmax(a), |dr_c| <= r_c (1 - r_c) (|da_c| + max|da|) <= 0.5 max|da| with
    |da| <= LL_RTOL max|ll|."""
    return 0.5 * LL_RTOL * float(np.abs(ll).max())


@pytest.mark.parametrize("name", sorted(isc.MIX_MODELS))
def test_mixture_score_matches_yardstick(name):
    import torch
    from gbnf_amd import native
    specs, log_w, x, noise, y = _mixture_ref(name)
    assert np.all(y["r"].max(axis=0) <= isc.R_MAX), "every component's gradient must enter: checked on the yardstick first"
    dev = torch.device("cuda:0")
    trainers = _score_trainers(specs, dev)
    g_x, G, r = native.image_mixture_score(trainers, _dev(log_w, dev), _dev(x, dev), _dev(noise, dev), want_r=True)
    err_r = float(np.abs(r.cpu().numpy() - y["r"]).max())
    print(f"{name}: G {rel_err(G.cpu().numpy(), y['G']):.3e} of {LL_RTOL}, r {err_r:.3e} of {_r_bar(y['ll']):.3e}")
    assert rel_err(G.cpu().numpy(), y["G"]) < LL_RTOL
    assert err_r <= _r_bar(y["ll"])
    _check_gx(g_x, y["gx"], f"mixture {name}")
    # a component alone (log_w = 0): its own score and log-density
    for c in (0, len(specs) - 1):
        ll_c, gx_c = isc.component_yardstick(specs[c], x, noise)
        g1, G1, _ = native.image_mixture_score([trainers[c]], torch.zeros(1, device=dev), _dev(x, dev), _dev(noise, dev))
        assert rel_err(G1.cpu().numpy(), ll_c) < LL_RTOL
        _check_gx(g1, gx_c, f"mixture {name} component {c} alone")
    for tr in trainers:
        tr.close()


def test_mixture_score_is_deterministic_in_ordered_mode():
    import torch
    from gbnf_amd import native
    specs, log_w, x, noise, _ = _mixture_ref("D3")
    dev = torch.device("cuda:0")
    trainers = _score_trainers(specs, dev, deterministic=True)
    args = (trainers, _dev(log_w, dev), _dev(x, dev), _dev(noise, dev))
    first = native.image_mixture_score(*args, want_r=True)
    for _ in range(2):
        again = native.image_mixture_score(*args, want_r=True)
        assert all(torch.equal(a, b) for a, b in zip(first, again))
    for tr in trainers:
        tr.close()


def test_library_refusals():
    """Wrong shapes, a trace of another n, a short workspace: refused (before any launch: the outputs keep their contents)."""
    import torch
    from gbnf_amd import native
    specs, log_w, x, noise, _ = _mixture_ref("A3")
    dev = torch.device("cuda:0")
    trainers = _score_trainers(specs, dev)
    tr = trainers[0]
    xd, nd, lw = _dev(x, dev), _dev(noise, dev), _dev(log_w, dev)
    z, ldj, trace = tr.forward(xd, nd)
    with pytest.raises(native.GbnfError):
        tr.backward_x(trace, xd[:, :, :-2], nd)                                   # another image shape
    with pytest.raises(native.GbnfError):
        tr.backward_x(trace, xd[:2].contiguous(), nd[:2].contiguous())            # a trace of another n
    with pytest.raises(native.GbnfError):
        tr.backward_x(trace, xd, nd, g_z=z[:, :-1].contiguous())
    with pytest.raises(native.GbnfError):
        tr.backward_x(trace, xd, nd, g_ldj=ldj[:-1].contiguous())
    keep = torch.full_like(xd, 7.0)
    small = torch.empty(tr.workspace_bytes(x.shape[0]) // 4 - 64, dtype=torch.float32, device=dev)
    with pytest.raises(native.GbnfError, match="workspace too small"):
        tr.backward_x(trace, xd, nd, z, ldj, g_x=keep, workspace=small)
    assert bool((keep == 7.0).all())
    nb = native.image_mixture_score_workspace_bytes(trainers, x.shape[0])
    with pytest.raises(native.GbnfError, match="workspace too small"):
        native.image_mixture_score(trainers, lw, xd, nd, workspace=torch.empty(nb // 4 - 64, dtype=torch.float32, device=dev))
    with pytest.raises(native.GbnfError):
        native.image_mixture_score(trainers, lw[:2].contiguous(), xd, nd)
    with pytest.raises(native.GbnfError):
        native.image_mixture_score(trainers, lw, xd, nd[:2].contiguous())
    with pytest.raises(native.GbnfError):
        native.image_mixture_score([], lw, xd, nd)
    with pytest.raises(native.GbnfError):
        native.mixture_responsibilities(torch.zeros(3, 4, device=dev), torch.zeros(2, device=dev))
    for t in trainers:
        t.close()


# ---------------------------------------------------------------------------------------------------------------------
# the module: BoostedFlow(args).component_score / score / responsibilities, eval or train mode
# ---------------------------------------------------------------------------------------------------------------------
def _g24(name):
    import os
    return np.load(os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden", "image_score",
                                name.replace("g21_image_grads", "g24_image_score") + ".npz"))


@pytest.mark.parametrize("name", igo.G21)
def test_module_component_score_matches_reference_and_yardstick(name):
    """The g21 modules (invconv affine, LU, shuffle additive): component_score and the one-component score against the reference's
    own d sum(ll) / dx (fixtures g24) and the yardstick; the autograd opt-in returns the same g_x."""
    import torch
    from gbnf_amd import image_glow
    cfg, data = igo.g21_load(name)
    g24 = _g24(name)
    dev = torch.device("cuda:0")
    m = igo.g21_module(cfg, data, dev)
    m.eval()
    xd, nd = _dev(data["x"], dev), _dev(data["noise"], dev)
    g_x, ll = m.component_score(xd, 0, nd)
    ll64, gx64 = isc.component_yardstick(image_glow.image_spec_from_glow_module(m.flows[0]), data["x"], data["noise"])
    assert rel_err(ll.cpu().numpy(), ll64) < LL_RTOL and rel_err(ll.cpu().numpy(), g24["ll"]) < LL_RTOL
    _check_gx(g_x, gx64, f"{name} yardstick")
    _check_gx(g_x, g24["gx"].astype(np.float64), f"{name} reference")
    s, lp, r = m.score(xd, noise=nd, return_log_prob=True, return_responsibilities=True)
    # (g_x has no atomics behind it; the log-density has the forward's log-det atomics: fewer than 128 partials per image, as in
    # test_eval_and_no_grad_keep_the_evaluation_path)
    assert torch.equal(s, g_x) and bool(((lp - ll).abs() <= 128 * 2.0 ** -24 * ll.abs()).all())
    assert tuple(r.shape) == (xd.shape[0], 1) and bool((r == 1.0).all())
    # autograd, opt-in: the recorded forward with x a leaf
    m.train()
    xl = xd.clone().requires_grad_(True)
    with pytest.raises(NotImplementedError):
        m.component_forward(xl, 0, nd)
    z, z_mu, z_var, ldj, _ = m.component_forward(xl, 0, nd, input_grad=True)
    ((-0.5 * (z_var + (z - z_mu) ** 2 * (-z_var).exp())).sum(dim=[1, 2, 3]) + ldj).sum().backward()
    _check_gx(xl.grad, gx64, f"{name} autograd")
    # (the same kernels on seeds torch formed: the chain's ~100 f32 roundings, each 2^-24 of the running value)
    assert float((xl.grad - g_x).abs().max()) <= 1e-5 * float(g_x.abs().max())
    assert all(p.grad is not None for p in m.flows[0].parameters() if p.requires_grad)


def _mixture_module(name, dev, **flags):
    import argparse
    from gbnf_amd import BoostedFlow, image_glow
    specs, log_w, x, noise, y = _mixture_ref(name)
    case = isc.MIX_MODELS[name][0]
    size, kw, _, _ = igo.CASES[case]
    args = argparse.Namespace(
        num_flows=kw["K"], z_size=int(np.prod(size)), density_evaluation=True, device=dev, cuda=True, component_type="glow",
        num_components=len(specs), rho_init="decreasing", learn_top=kw.get("learn_top", True), y_classes=0, y_condition=False,
        sample_size=4, input_size=list(size), h_size=kw["h"], num_blocks=kw["L"], actnorm_scale=1.0,
        flow_permutation=kw.get("permutation", "invconv"), flow_coupling=kw.get("coupling", "affine"), LU_decomposed=False,
        num_dequant_blocks=0, coupling_network="tanh", coupling_network_depth=kw.get("depth", 1), batch_norm=False, **flags)
    m = BoostedFlow(args)
    for c, sp in enumerate(specs):
        image_glow.load_image_spec(m.flows[c], sp)
    return m, x, noise, y


def test_module_score_matches_yardstick_and_composes():
    """score of a three-component module against the yardstick, and against sum_c r_c component_score_c composed on the host."""
    import torch
    dev = torch.device("cuda:0")
    m, x, noise, y = _mixture_module("A3", dev)
    m.eval()
    xd, nd = _dev(x, dev), _dev(noise, dev)
    g_x, lp, r = m.score(xd, noise=nd, return_log_prob=True, return_responsibilities=True)
    assert tuple(r.shape) == (x.shape[0], 3)
    assert rel_err(lp.cpu().numpy(), y["G"]) < LL_RTOL
    assert float(np.abs(r.cpu().numpy() - y["r"].T).max()) <= _r_bar(y["ll"])
    _check_gx(g_x, y["gx"], "module A3")
    assert float(np.abs(m.responsibilities(xd, noise=nd).cpu().numpy() - y["r"].T).max()) <= _r_bar(y["ll"])
    host = sum(r[:, c].view(-1, 1, 1, 1) * m.component_score(xd, c, nd)[0] for c in range(3))
    # the backward is linear in its seed: scaling the seed by r instead of the result moves the chain's f32 roundings only
    assert float((host - g_x).abs().max()) <= 2e-5 * float(g_x.abs().max())
    # the first two components alone: the weights renormalise
    g2, lp2 = m.score(xd, n_used=2, noise=nd, return_log_prob=True)
    a = torch.from_numpy(y["ll"][:2]) + torch.log(torch.tensor([2.0 / 3.0, 1.0 / 3.0], dtype=torch.float64)).view(-1, 1)
    assert rel_err(lp2.cpu().numpy(), torch.logsumexp(a, dim=0).numpy()) < LL_RTOL
    # noise None: drawn once per call, shared by the components
    assert m.score(xd).shape == xd.shape
    with pytest.raises(ValueError):
        m.score(xd, n_used=4)
    with pytest.raises(ValueError):
        m.score(xd, n_used=0)
    with pytest.raises(ValueError):
        m.component_score(xd, 3)
    with pytest.raises(ValueError):
        m.score(xd[:, :, :-2], noise=nd[:, :, :-2])
    m.flows[1].flow.layers[1].actnorm.inited = False
    with pytest.raises(ValueError):
        m.score(xd, noise=nd)


def test_module_score_determinism():
    """image_deterministic: two score calls are bit-equal in g_x, G and r; component_score of one image alone equals its row of
    the batch where the trainer's forward has that property (z of the image alone bit-equal to its row)."""
    import torch
    dev = torch.device("cuda:0")
    m, x, noise, _ = _mixture_module("D3", dev, image_deterministic=True)
    m.eval()
    xd, nd = _dev(x, dev), _dev(noise, dev)
    first = m.score(xd, noise=nd, return_log_prob=True, return_responsibilities=True)
    again = m.score(xd, noise=nd, return_log_prob=True, return_responsibilities=True)
    assert all(torch.equal(a, b) for a, b in zip(first, again))
    tr, _ = m._step_trainer(0)
    assert tr.deterministic
    z_all = tr.forward(xd, nd)[0]
    g_all, _ = m.component_score(xd, 0, nd)
    for i in range(x.shape[0]):
        z_one = tr.forward(xd[i:i + 1].contiguous(), nd[i:i + 1].contiguous())[0]
        if torch.equal(z_one[0], z_all[i]):
            g_one, _ = m.component_score(xd[i:i + 1].contiguous(), 0, nd[i:i + 1].contiguous())
            assert torch.equal(g_one[0], g_all[i])


def test_module_class_conditional_component_score():
    """One class-conditional component (fixture g22, invconv affine) against tests/image_ycond_oracle.py with x a leaf."""
    import torch
    import image_ycond_oracle as iyo
    from gbnf_amd import image_glow
    cfg, data = iyo.g22_load("g22_image_ycond_invconv_affine")
    dev = torch.device("cuda:0")
    m = iyo.g22_module(cfg, data, dev)
    m.eval()
    xd, nd, yd = _dev(data["x"], dev), _dev(data["noise"], dev), _dev(data["y"], dev)
    g_x, ll = m.component_score(xd, 0, nd, y_onehot=yd)
    sp = image_glow.image_spec_from_glow_module(m.flows[0])
    xl = torch.tensor(np.asarray(data["x"]), dtype=torch.float64, requires_grad=True)
    out = iyo.forward(sp, iyo.leaf_params(sp), xl, data["noise"], data["y"])
    out["ll"].sum().backward()
    assert rel_err(ll.cpu().numpy(), out["ll"].detach().numpy()) < LL_RTOL
    _check_gx(g_x, xl.grad.numpy(), "g22 class-conditional")
    with pytest.raises(ValueError):
        m.component_score(xd, 0, nd)                                  # y_onehot missing on a conditional model
    with pytest.raises(ValueError):
        m.score(xd, noise=nd)
