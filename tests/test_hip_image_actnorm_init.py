"""GPU: the data-dependent ActNorm2d initialisation of an image Glow component in ONE pass on the live trainer
(gbnf_image_trainer_actnorm_init, native.NativeImageTrainer.actnorm_init, BoostedImageFlow.initialize_actnorms(fused=True)) against
the reference's stored values (fixtures g20), the float64 oracle (oracle.image_actnorm_init) and the layer-by-layer default path.

Bars: every bias / logs within 1e-5 * max(1, max|ref|) of the reference -- the bar of test_image_actnorm_data_init_matches_reference,
which the float32 oracle meets with a 30x margin on the synthetic cases (tests/test_image_actnorm_init_host.py) --, so two paths
that both meet it agree within 2e-5; ldj within LL_RTOL, z within 2e-5 of its largest entry."""
import copy
import ctypes as C

import numpy as np
import pytest

import image_actnorm_init_cases as cases
import image_grad_oracle as igo
from conftest import IMAGE_ACTNORM_INIT_CASES, load_image_actnorm_init_case, rel_err

pytestmark = pytest.mark.gpu
LL_RTOL = 1e-5
BAR = cases.BAR
PAIR_BAR = 2e-5      # two paths that each lie within 1e-5 of the truth


def _np(t):
    return t.detach().cpu().numpy().reshape(-1)


def _module_actnorms(glow):
    return [(_np(a.bias), _np(a.logs)) for a in glow._actnorms()]


def _module(input_size, h, K, L, dev, LU=False, learn_top=True):
    import argparse
    from gbnf_amd import BoostedFlow
    args = argparse.Namespace(
        num_flows=K, z_size=int(np.prod(input_size)), density_evaluation=True, device=dev, cuda=True, component_type="glow",
        num_components=1, rho_init="decreasing", learn_top=learn_top, y_classes=0, y_condition=False, sample_size=4,
        input_size=list(input_size), h_size=h, num_blocks=L, actnorm_scale=1.0, flow_permutation="invconv", flow_coupling="affine",
        LU_decomposed=LU, num_dequant_blocks=0, coupling_network="tanh", coupling_network_depth=1, batch_norm=False)
    return BoostedFlow(args)


def _fresh_module(dev, LU=False, seed=11):
    """3x32x32, L = 2, K = 2, h = 32 with the numbers of a synthetic spec (LU: the module's own random LU factors for the 1x1
    matrices), every ActNorm2d un-initialised and zero.  -> (module, the spec as loaded: ActNorm2d arrays zeroed)."""
    import torch
    from gbnf_amd import image_glow, synth
    torch.manual_seed(seed)
    m = _module((3, 32, 32), 32, 2, 2, dev, LU=LU)
    sp = cases.zeroed(synth.synth_image_glow_spec((3, 32, 32), h=32, K=2, L=2, seed=seed))
    glow = m.flows[0]
    if LU:
        steps = [st for lv in sp["levels"] for st in lv["steps"]]
        splits = [lv["split"] for lv in sp["levels"] if lv["split"] is not None]
        si = pi = 0
        for layer in glow.flow.layers:
            if isinstance(layer, image_glow.FlowStep):
                for cm, c in zip([q for q in layer.block.network if not isinstance(q, torch.nn.ReLU)], steps[si]["convs"]):
                    image_glow._load_conv(cm, c)
                steps[si]["perm_w"] = layer.invconv.composed_weight().astype(np.float32)
                si += 1
            elif isinstance(layer, image_glow.Split2d):
                image_glow._load_conv(layer.conv, splits[pi])
                pi += 1
        image_glow._load_conv(glow.learn_top_fn, sp["learn_top"])
    else:
        image_glow.load_image_spec(glow, sp)
    for a in glow._actnorms():
        a.inited = False
    return m, sp


def _batch(n, size, dev, seed=3):
    import torch
    from gbnf_amd import synth
    x, noise = synth.synth_image_batch(n, size, seed=seed)
    return x, noise, torch.from_numpy(x).to(dev), torch.from_numpy(noise).to(dev)


# ---- 1. the reference's own numbers ---------------------------------------------------------------------------------------------
@pytest.mark.parametrize("name", IMAGE_ACTNORM_INIT_CASES)
def test_fused_init_matches_reference_fixture(name):
    import torch
    cfg, m, x, noise, after, data = load_image_actnorm_init_case(name, device="cuda:0")
    dev = torch.device("cuda:0")
    xd, nd = torch.from_numpy(x).to(dev), torch.from_numpy(noise).to(dev)
    glow = m.flows[0]
    assert not any(a.inited for a in glow._actnorms())
    m.initialize_actnorms(xd, noise=nd, fused=True)
    acts = glow._actnorms()
    assert all(a.inited for a in acts) and len(acts) == len(after)
    w = cases.worst(_module_actnorms(glow), after)
    print(f"{name}: worst bias / logs error {w:.3e} of {BAR}")
    for a, (rb, rl) in zip(acts, after):
        assert np.abs(_np(a.bias) - rb).max() <= BAR * max(1.0, float(np.abs(rb).max()))
        assert np.abs(_np(a.logs) - rl).max() <= BAR * max(1.0, float(np.abs(rl).max()))
    m.eval()
    zz, ldj, ll = m.native_flow(0).forward(xd, nd)
    assert rel_err(ldj.cpu().numpy(), data["ldj"]) < LL_RTOL
    assert np.abs(zz.cpu().numpy() - data["z"]).max() <= 2e-5 * max(1.0, float(np.abs(data["z"]).max()))


# ---- 2. geometries the fixtures lack, against the float64 oracle ------------------------------------------------------------------
def _raw_init(name, n=None, deterministic=False, workspace=None):
    """The raw trainer call on a listed case -> ([(bias, logs)] as numpy in module order, the device tensors)."""
    import torch
    from gbnf_amd import native
    sp, x, noise = cases.make(name, n)
    dev = torch.device("cuda:0")
    ds = igo.dev_spec(sp, dev)
    tr = native.NativeImageTrainer(ds, deterministic=deterministic)
    assert tr.actnorm_count() == len(cases.spec_actnorms(sp))
    tr.actnorm_init(torch.from_numpy(x).to(dev), torch.from_numpy(noise).to(dev), workspace=workspace(tr, x.shape[0]) if workspace else None)
    tensors = cases.spec_actnorms(ds)
    torch.cuda.synchronize()
    tr.close()
    return [(_np(b), _np(l)) for b, l in tensors], tensors


@pytest.mark.parametrize("name", list(cases.CASES))
def test_fused_init_matches_float64_oracle(name):
    got, _ = _raw_init(name)
    _, ref = cases.oracle_init(name)
    w = cases.worst(got, ref)
    print(f"{name}: worst bias / logs error against float64 {w:.3e} of {BAR}")
    assert w <= BAR


# ---- 3. LU-decomposed 1x1 steps ---------------------------------------------------------------------------------------------------
def test_fused_init_lu_agrees_with_default_path():
    import torch
    dev = torch.device("cuda:0")
    m, _ = _fresh_module(dev, LU=True)
    m2, m3 = copy.deepcopy(m), copy.deepcopy(m)
    _, _, xd, nd = _batch(4, (3, 32, 32), dev)
    m.initialize_actnorms(xd, noise=nd, fused=True)
    m2.initialize_actnorms(xd, noise=nd)
    assert all(a.inited for a in m.flows[0]._actnorms())
    w = cases.worst(_module_actnorms(m.flows[0]), _module_actnorms(m2.flows[0]))
    print(f"LU: fused against default {w:.3e} of {PAIR_BAR}")
    assert w <= PAIR_BAR
    # with the LU factors bound to the trainer (as training_step binds them): the library composes the matrices itself
    m3.flows[0].set_actnorm_init()
    bound, _ = m3._step_trainer(0)
    for a in m3.flows[0]._actnorms():
        a.inited = False
    m3.initialize_actnorms(xd, noise=nd, fused=True)
    assert m3._trainers[0][1] is bound
    assert cases.worst(_module_actnorms(m3.flows[0]), _module_actnorms(m2.flows[0])) <= PAIR_BAR


# ---- 4. skip ------------------------------------------------------------------------------------------------------------------------
def test_fused_init_leaves_initialised_layers_alone():
    import torch
    dev = torch.device("cuda:0")
    m, _ = _fresh_module(dev)
    rng = np.random.RandomState(5)
    acts = m.flows[0]._actnorms()
    for i, a in enumerate(acts):
        if i % 2 == 1:                                         # every second layer: initialised, arbitrary non-zero values
            with torch.no_grad():
                a.bias.copy_(torch.from_numpy((0.2 * rng.standard_normal(a.num_features) + 0.05).astype(np.float32)).view_as(a.bias))
                a.logs.copy_(torch.from_numpy((0.2 * rng.standard_normal(a.num_features) + 0.05).astype(np.float32)).view_as(a.logs))
            a.inited = True
    m2 = copy.deepcopy(m)
    held = [(a.bias.detach().clone(), a.logs.detach().clone()) for a in acts]
    _, _, xd, nd = _batch(4, (3, 32, 32), dev)
    m.initialize_actnorms(xd, noise=nd, fused=True)
    m2.initialize_actnorms(xd, noise=nd)
    assert all(a.inited for a in acts)
    for i, (a, (b0, l0)) in enumerate(zip(acts, held)):
        if i % 2 == 1:
            assert torch.equal(a.bias.detach(), b0) and torch.equal(a.logs.detach(), l0), f"layer {i} was written"
        else:
            assert float(a.logs.detach().abs().max()) > 0.0, f"layer {i} was not written"
    w = cases.worst(_module_actnorms(m.flows[0]), _module_actnorms(m2.flows[0]))
    print(f"skip: fused against default {w:.3e} of {PAIR_BAR}")
    assert w <= PAIR_BAR
    # a second call on the initialised model changes nothing
    now = [(a.bias.detach().clone(), a.logs.detach().clone()) for a in acts]
    m.initialize_actnorms(xd * 0.5, noise=nd, fused=True)
    assert all(torch.equal(a.bias.detach(), b) and torch.equal(a.logs.detach(), l) for a, (b, l) in zip(acts, now))
    # ... also through the raw call with every flag set
    tr = m._trainers[0][1]
    tr.actnorm_init(xd * 0.5, nd, skip=[True] * tr.actnorm_count())
    assert all(torch.equal(a.bias.detach(), b) and torch.equal(a.logs.detach(), l) for a, (b, l) in zip(acts, now))


# ---- 5. nothing is assumed about the workspace ------------------------------------------------------------------------------------
def test_fused_init_on_poisoned_workspace():
    import torch

    def poisoned(tr, n):
        return torch.full(((tr.actnorm_init_workspace_bytes(n) + 3) // 4,), float("nan"), dtype=torch.float32, device="cuda:0")

    got, _ = _raw_init("1x28x20", workspace=poisoned)
    _, ref = cases.oracle_init("1x28x20")
    assert cases.worst(got, ref) <= BAR


# ---- 6. bit-identical from run to run, in and out of deterministic mode -----------------------------------------------------------
def test_fused_init_is_repeatable():
    import torch
    a, _ = _raw_init("1x28x20", n=40)                      # 10 chunks of 4 images on the 16-wide level, 3 of 16 on the 8-wide one
    b, _ = _raw_init("1x28x20", n=40)
    d, _ = _raw_init("1x28x20", n=40, deterministic=True)
    for (ab, al), (bb, bl), (db, dl) in zip(a, b, d):
        assert np.array_equal(ab, bb) and np.array_equal(al, bl)
        assert np.array_equal(ab, db) and np.array_equal(al, dl)
    _, ref = cases.oracle_init("1x28x20", n=40)
    assert cases.worst(a, ref) <= BAR
    # the module's flag: image_deterministic on a clone
    dev = torch.device("cuda:0")
    m, _ = _fresh_module(dev)
    m2 = copy.deepcopy(m)
    m2.image_deterministic = True
    _, _, xd, nd = _batch(40, (3, 32, 32), dev)
    m.initialize_actnorms(xd, noise=nd, fused=True)
    m2.initialize_actnorms(xd, noise=nd, fused=True)
    assert m2._trainers[0][1].deterministic
    for p, q in zip(m.flows[0]._actnorms(), m2.flows[0]._actnorms()):
        assert torch.equal(p.bias, q.bias) and torch.equal(p.logs, q.logs)


# ---- 7. training goes on from the initialised model, on the same trainer ------------------------------------------------------------
def test_training_step_after_fused_init_reuses_the_trainer():
    import torch
    from oracle import gbnf_oracle as oracle
    dev = torch.device("cuda:0")
    m, sp = _fresh_module(dev)
    x, noise, xd, nd = _batch(4, (3, 32, 32), dev)
    m.initialize_actnorms(xd, noise=nd, fused=True)
    tr = m._trainers[0][1]
    # the evaluation path on the initialised parameters against the oracle on the oracle-initialised spec
    ref = oracle.image_actnorm_init(sp, x, noise, dtype=torch.float64)
    assert cases.worst(_module_actnorms(m.flows[0]), ref) <= BAR
    zo, _, _, ld_o, ll_o = oracle.image_component_forward(sp, x, noise, dtype=torch.float64)
    m.eval()
    zz, ldj, ll = m.native_flow(0).forward(xd, nd)
    assert rel_err(ldj.cpu().numpy(), ld_o) < LL_RTOL and rel_err(ll.cpu().numpy(), ll_o) < LL_RTOL
    assert np.abs(zz.cpu().numpy() - zo).max() <= 2e-5 * max(1.0, float(np.abs(zo).max()))
    m.train()
    out = m.training_step(xd, lr=1e-3, noise=nd)
    assert m._trainers[0][1] is tr, "the trainer was re-created after the initialisation"
    assert bool(torch.isfinite(out["nll"]))


# ---- 8. the raw ABI's refusals ------------------------------------------------------------------------------------------------------
def test_raw_abi_refusals_launch_nothing():
    import torch
    from gbnf_amd import native
    sp, x, noise = cases.make("1x28x20")
    dev = torch.device("cuda:0")
    rng = np.random.RandomState(9)
    for st in (st for lv in sp["levels"] for st in lv["steps"]):          # entry values a launch would overwrite
        st["an_bias"] = rng.standard_normal(st["an_bias"].shape).astype(np.float32)
        st["an_logs"] = (0.1 * rng.standard_normal(st["an_logs"].shape)).astype(np.float32)
    ds = igo.dev_spec(sp, dev)
    tr = native.NativeImageTrainer(ds)
    tensors = cases.spec_actnorms(ds)
    before = [(b.clone(), l.clone()) for b, l in tensors]
    xd, nd = torch.from_numpy(x).to(dev), torch.from_numpy(noise).to(dev)
    n = x.shape[0]
    L = native.lib()
    count = C.c_int32()
    assert L.gbnf_image_trainer_actnorm_count(tr.handle, C.byref(count)) == 0
    glow_like = sum(1 + sum(c["an_bias"] is not None for c in st["convs"]) for lv in sp["levels"] for st in lv["steps"])
    assert count.value == glow_like == tr.actnorm_count()
    nb = C.c_int64()
    assert L.gbnf_image_trainer_actnorm_init_workspace_bytes(tr.handle, n, C.byref(nb)) == 0 and nb.value > 0
    ws = torch.empty((nb.value + 3) // 4, dtype=torch.float32, device=dev)
    ptr = lambda t: C.c_void_p(t.data_ptr())
    INVALID = -1                                                           # GBNF_ERR_INVALID
    call = L.gbnf_image_trainer_actnorm_init
    assert call(tr.handle, ptr(xd), ptr(nd), n, 1.0, None, ptr(ws), nb.value - 1, None) == INVALID      # a short workspace
    assert call(tr.handle, ptr(xd), ptr(nd), n, 1.0, None, None, nb.value, None) == INVALID             # no workspace
    assert call(tr.handle, ptr(xd), ptr(nd), 0, 1.0, None, ptr(ws), nb.value, None) == INVALID          # n = 0
    assert call(tr.handle, ptr(xd), ptr(nd), n, 0.0, None, ptr(ws), nb.value, None) == INVALID          # scale = 0
    assert call(tr.handle, ptr(xd), ptr(nd), n, float("nan"), None, ptr(ws), nb.value, None) == INVALID
    assert call(tr.handle, None, ptr(nd), n, 1.0, None, ptr(ws), nb.value, None) == INVALID             # no x
    assert call(tr.handle, ptr(xd), ptr(nd), 65536, 1.0, None, ptr(ws), nb.value, None) == -2           # GBNF_ERR_UNSUPPORTED
    assert L.gbnf_image_trainer_actnorm_count(tr.handle, None) == INVALID
    assert L.gbnf_image_trainer_actnorm_init_workspace_bytes(tr.handle, n, None) == INVALID
    torch.cuda.synchronize()
    for (b, l), (b0, l0) in zip(tensors, before):
        assert torch.equal(b, b0) and torch.equal(l, l0)
    tr.close()


def test_actnorm_count_equals_the_modules():
    import torch
    dev = torch.device("cuda:0")
    m, _ = _fresh_module(dev)
    trainer, _ = m._native_trainer(0, allow_uninit=True)
    assert trainer.actnorm_count() == len(m.flows[0]._actnorms())
    with pytest.raises(ValueError):
        m.native_trainer(0)                                 # the public way in still refuses an un-initialised component
