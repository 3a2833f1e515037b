"""GPU: the full-latent direction of the image path (gbnf_image_flow_encode, NativeImageFlow.encode, BoostedImageFlow.encode_latent /
reconstruct / interpolate / round_trip_error) against the float64 yardstick of tests/image_latent_oracle.py, the reference's decode
fixtures (g16) and the other direction (gbnf_image_flow_inverse).  Bars: the project's own -- 2e-4 * max(1, max |ref|) on z and eps,
1e-5 relative on ldj / ll, 5e-5 absolute on x."""
import ctypes as C
import functools

import numpy as np
import pytest

import image_latent_oracle as ilo
from conftest import IMAGE_DECODE_CASES, load_image_decode_case, rel_err

pytestmark = pytest.mark.gpu
LL_RTOL = 1e-5
X_ATOL = 5e-5
SENTINEL = -12345.0


def _bar(ref):
    return 2e-4 * max(1.0, float(np.abs(ref).max()))


@functools.lru_cache(maxsize=None)
def _case(name, n):
    """(spec, size, x, noise, yardstick (z, eps, ldj, u), ll) of a geometry at a batch of n -- computed once, never modified."""
    import torch
    from oracle import gbnf_oracle as oracle
    sp, size, x, noise = ilo.geometry(name, n)
    ref = ilo.encode(sp, x, noise)
    ll = oracle.image_component_forward(sp, x, noise, dtype=torch.float64)[4]
    return sp, size, x, noise, ref, ll


def _dev(a):
    import torch
    return torch.from_numpy(np.ascontiguousarray(a, dtype=np.float32)).to("cuda:0")


def _assert_latent(z, eps, ref_z, ref_eps, what=""):
    ez = ilo.max_abs(z.cpu().numpy(), ref_z)
    ee = [ilo.max_abs(e.cpu().numpy(), r) for e, r in zip(eps, ref_eps)]
    print(f"{what}: z {ez:.2e} of {_bar(ref_z):.2e}; eps " + ", ".join(f"{a:.2e} of {_bar(r):.2e}" for a, r in zip(ee, ref_eps)))
    assert ez <= _bar(ref_z)
    assert len(eps) == len(ref_eps)
    for a, r in zip(ee, ref_eps):
        assert a <= _bar(r)


# ---- 1. agreement with the yardstick ------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("name,math,n", [("3x32x32_L2", "default", 5), ("3x32x32_L3", "default", 5), ("1x28x28_L2", "default", 5),
                                         ("1x28x20_add_shuffle", "default", 5), ("3x32x32_depth2", "default", 5),
                                         ("3x32x32_L3", "f32", 5), ("1x28x28_L2", "f32", 5),
                                         ("3x32x32_L2", "default", 1), ("1x28x20_add_shuffle", "f32", 1)])
def test_encode_matches_the_yardstick(name, math, n):
    import torch
    from gbnf_amd import native
    sp, size, x, noise, (rz, reps, rld, _), rll = _case(name, n)
    flow = native.NativeImageFlow(sp, math=math)
    if name == "3x32x32_L2" and math == "default":
        assert native.MATH_NAME[int(flow.numerics().math_mode)] == "f16x3"          # the fused split-f16 coupling nets
    xd, nd = _dev(x), _dev(noise)
    z, eps, ldj, ll = flow.encode(xd, nd, want_ll=True)
    assert [tuple(e.shape) for e in eps] == [(n,) + tuple(s) for s in flow.split_shapes()]
    assert all(e.is_contiguous() for e in eps)
    if len(eps) > 1:                                                              # views of one allocation, level 0 first
        assert eps[1].data_ptr() == eps[0].data_ptr() + 4 * eps[0].numel()
    _assert_latent(z, eps, rz, reps, f"{name} {math} n={n}")
    assert rel_err(ldj.cpu().numpy(), rld) < LL_RTOL and rel_err(ll.cpu().numpy(), rll) < LL_RTOL
    z_f, ldj_f, ll_f = flow.forward(xd, nd)
    assert torch.equal(z, z_f)
    assert rel_err(ldj.cpu().numpy(), ldj_f.cpu().numpy()) < LL_RTOL
    # without noise and without ll
    z0, eps0, ldj0, ll0 = flow.encode(xd)
    assert ll0 is None and torch.equal(z0, flow.forward(xd, None)[0])


# ---- 2. the round trip on the caller's data ----------------------------------------------------------------------------------------------
@pytest.mark.parametrize("name,math", [(g, "default") for g in ilo.GEOMETRIES] + [("3x32x32_L3", "f32")])
def test_inverse_of_encode_returns_the_dequantised_input(name, math):
    """inverse(encode(x), temperature = 1) == u = (255 x + noise) / 256 within X_ATOL on every pixel: no mask."""
    from gbnf_amd import native
    sp, size, x, noise, (_, _, _, u), _ = _case(name, 5)
    flow = native.NativeImageFlow(sp, math=math)
    z, eps, _, _ = flow.encode(_dev(x), _dev(noise))
    x_hat = flow.inverse(z, eps, 1.0)
    err = ilo.max_abs(x_hat.cpu().numpy(), u)
    print(f"{name} {math}: max |decode(encode(x)) - u| = {err:.2e}")
    assert err <= X_ATOL


# ---- 3. the reference's decode, taken back ------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("name", IMAGE_DECODE_CASES)
def test_encode_takes_the_reference_decode_back(name):
    """g16: encoding the reference's decoded image with noise = x_ref (u = x_ref; x_ref reaches -0.05 and 1.05, the pre-kernel does not
    clamp) gives back the fixture's z and temperature * eps."""
    from gbnf_amd import native
    cfg, spec, z_fix, eps_fix, x_ref = load_image_decode_case(name)
    flow = native.NativeImageFlow(spec)
    xd = _dev(x_ref)
    z, eps, _, _ = flow.encode(xd, xd.clone())
    _assert_latent(z, eps, z_fix, [cfg["temperature"] * e.astype(np.float64) for e in eps_fix], name)


# ---- 4. repair ------------------------------------------------------------------------------------------------------------------------------
def _blow_up_hidden(sp, step=0, gain_logs=12.0):
    """tests/test_hip_image.py's recipe: the coupling net of one FlowStep leaves the fp16 range (its first convolution's ActNorm2d
    scales every hidden channel by e^gain_logs), the last convolution's weights shrink by the same factor."""
    import copy
    sp = copy.deepcopy(sp)
    net = sp["levels"][0]["steps"][step]["convs"]
    net[0]["an_logs"] = net[0]["an_logs"] + np.float32(gain_logs)
    net[-1]["w"] = (net[-1]["w"] * np.float32(np.exp(-gain_logs))).astype(np.float32)
    return sp


def test_marked_images_get_their_eps_from_the_exact_sequence(monkeypatch):
    """Every image of the batch is out of the fp16 range (probe off, on-data check off): the repair launch of the same call writes
    z, ldj AND eps of each from the exact-f32 sequence."""
    import torch
    from gbnf_amd import native, synth
    monkeypatch.setenv("GBNF_IMAGE_NO_PROBE", "1")
    native.tuning_set("check_every", -1)
    try:
        sp = _blow_up_hidden(synth.synth_image_glow_spec((3, 32, 32), h=64, K=2, L=2, seed=11))
        x, noise = synth.synth_image_batch(5, seed=3)
        rz, reps, rld, u = ilo.encode(sp, x, noise)
        flow = native.NativeImageFlow(sp)
        assert native.MATH_NAME[int(flow.numerics().math_mode)] == "f16x3"
        z, eps, ldj, ll = flow.encode(_dev(x), _dev(noise), want_ll=True)
        torch.cuda.synchronize()
        assert flow.repair_counts()["repaired_images"] == 5
        _assert_latent(z, eps, rz, reps, "repaired")
        assert rel_err(ldj.cpu().numpy(), rld) < LL_RTOL and torch.isfinite(ll).all()
    finally:
        native.tuning_set("check_every", 256)


def test_a_failed_on_data_check_re_evaluates_every_eps():
    """The on-data check with a tolerance no result can meet (negative: at zero a small model's split-f16 ldj can agree with the exact
    one to the last bit): the repair launch of THAT call re-evaluates all images -- z and eps are the exact-f32 handle's, bit for bit."""
    import torch
    from gbnf_amd import native
    sp, size, x, noise, _, _ = _case("3x32x32_L2", 5)
    xd, nd = _dev(x), _dev(noise)
    z3, eps3, _, _ = native.NativeImageFlow(sp, math="f32").encode(xd, nd)
    flow = native.NativeImageFlow(sp)
    assert native.MATH_NAME[int(flow.numerics().math_mode)] == "f16x3"
    native.tuning_set("check_tolerance_e9", -1)
    try:
        z, eps, _, _ = flow.encode(xd, nd)
        torch.cuda.synchronize()
    finally:
        native.tuning_set("check_tolerance_e9", 2500)
    assert flow.repair_counts()["failed_checks"] >= 1
    assert torch.equal(z, z3) and all(torch.equal(a, b) for a, b in zip(eps, eps3))


# ---- 5. determinism ------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("name", ["3x32x32_L3", "1x28x28_L2"])
def test_encode_is_reproducible_and_row_independent(name):
    import torch
    from gbnf_amd import native
    sp, size, x, noise, _, _ = _case(name, 5)
    xd, nd = _dev(x), _dev(noise)
    flow = native.NativeImageFlow(sp)
    got = {}
    for det in (False, True):
        flow.deterministic = det
        a, b = flow.encode(xd, nd, want_ll=True), flow.encode(xd, nd, want_ll=True)
        assert torch.equal(a[0], b[0]) and all(torch.equal(p, q) for p, q in zip(a[1], b[1]))
        one = flow.encode(xd[2:3], nd[2:3], want_ll=True)                      # a row does not depend on n
        assert torch.equal(one[0], a[0][2:3]) and all(torch.equal(p, q[2:3]) for p, q in zip(one[1], a[1]))
        if det:
            assert torch.equal(a[2], b[2]) and torch.equal(a[3], b[3])
            z_f, ldj_f, ll_f = flow.forward(xd, nd)
            assert torch.equal(a[0], z_f) and torch.equal(a[2], ldj_f) and torch.equal(a[3], ll_f)
            assert torch.equal(one[2], a[2][2:3]) and torch.equal(one[3], a[3][2:3])
        got[det] = a
    assert torch.equal(got[False][0], got[True][0])                              # z and eps are identical in both modes
    assert all(torch.equal(p, q) for p, q in zip(got[False][1], got[True][1]))


# ---- 6. a class-conditional handle ---------------------------------------------------------------------------------------------------------
def test_encode_on_a_class_conditional_handle():
    import torch
    from gbnf_amd import native, synth
    sp = synth.synth_image_glow_spec((3, 32, 32), h=32, K=2, L=2, seed=31, y_classes=4)
    x, noise = synth.synth_image_batch(5, seed=32)
    flow = native.NativeImageFlow(sp)
    assert flow.y_classes == 4
    flow.deterministic = True                                                    # (ordered log-det sums: ldj compares bit for bit)
    xd, nd = _dev(x), _dev(noise)
    y = torch.eye(4, device="cuda:0")[torch.tensor([0, 3, 1, 2, 3])].contiguous()
    z_f, ldj_f = flow.forward(xd, nd, y=y)[:2]
    z, eps, ldj, ll = flow.encode(xd, nd)
    assert ll is None and torch.equal(z, z_f) and torch.equal(ldj, ldj_f)
    plain = native.NativeImageFlow({k: v for k, v in sp.items() if k != "ycond"})
    assert all(torch.equal(a, b) for a, b in zip(eps, plain.encode(xd, nd)[1]))   # x -> eps does not depend on the conditioning
    with pytest.raises(native.GbnfError, match="needs y"):
        flow.encode(xd, nd, want_ll=True)


# ---- 7. the module ----------------------------------------------------------------------------------------------------------------------------
def test_module_reconstruct_interpolate_and_round_trip_error():
    import argparse
    import torch
    from gbnf_amd import BoostedFlow, image_glow, synth
    dev = torch.device("cuda:0")
    args = argparse.Namespace(
        num_flows=2, z_size=3072, density_evaluation=True, device=dev, cuda=True, component_type="glow",
        num_components=2, rho_init="decreasing", learn_top=True, y_classes=0, y_condition=False,
        sample_size=4, input_size=[3, 32, 32], h_size=32, num_blocks=2, actnorm_scale=1.0,
        flow_permutation="invconv", flow_coupling="affine", LU_decomposed=False, num_dequant_blocks=0,
        coupling_network="tanh", coupling_network_depth=1, batch_norm=False)
    m = BoostedFlow(args)
    assert isinstance(m, image_glow.BoostedImageFlow)
    for c in range(2):
        image_glow.load_image_spec(m.flows[c], synth.synth_image_glow_spec((3, 32, 32), h=32, K=2, L=2, seed=40 + c))
    m.eval()
    xa, na = synth.synth_image_batch(3, seed=41)
    xb, _ = synth.synth_image_batch(3, seed=42)
    xad, xbd, nd = _dev(xa), _dev(xb), _dev(na)
    u = (255.0 * xa.astype(np.float64) + na) / 256.0
    z, eps = m.encode_latent(xad, 1, noise=nd)
    assert tuple(z.shape) == (3, 24, 8, 8) and [tuple(e.shape) for e in eps] == [(3, 6, 16, 16)]
    assert not z.requires_grad
    ra = m.reconstruct(xad, 1, noise=nd)
    assert ilo.max_abs(ra.cpu().numpy(), u) <= X_ATOL
    assert torch.equal(ra, m.decode(z, None, 1.0, 1, eps=eps))
    rb = m.reconstruct(xbd, 1, noise=nd)
    out = m.interpolate(xad, xbd, [0.0, 0.5, 1.0], 1, noise=nd)
    assert tuple(out.shape) == (3, 3, 3, 32, 32) and torch.isfinite(out).all()
    assert torch.equal(out[0], ra) and torch.equal(out[2], rb)
    assert not torch.equal(out[1], ra) and not torch.equal(out[1], rb)
    err = m.round_trip_error(xad, noise=nd)
    assert err.is_cuda and tuple(err.shape) == (2,)
    print("round_trip_error per component:", err.cpu().numpy())
    assert float(err.max()) <= X_ATOL
    assert tuple(m.round_trip_error(xad, components=0).shape) == (1,)          # (no noise: u = 255 x / 256)
    assert float(m.round_trip_error(xad, components=[1]).max()) <= X_ATOL


# ---- 8. refusals ----------------------------------------------------------------------------------------------------------------------------
def test_refusals_launch_nothing():
    """Each refused with GBNF_ERR_INVALID before any launch: sentinel-filled outputs stay untouched."""
    import torch
    from gbnf_amd import native, synth
    dev = torch.device("cuda:0")
    L = native.lib()
    sp = synth.synth_image_glow_spec((3, 32, 32), h=16, K=1, L=2, seed=51)
    flow = native.NativeImageFlow(sp, math="f32")
    cond = native.NativeImageFlow(synth.synth_image_glow_spec((3, 32, 32), h=16, K=1, L=2, seed=51, y_classes=3), math="f32")
    one = native.NativeImageFlow(synth.synth_image_glow_spec((3, 32, 32), h=16, K=1, L=1, seed=52), math="f32")
    n = 2
    x, noise = synth.synth_image_batch(n, seed=53)
    xd, nd = _dev(x), _dev(noise)
    per = C.c_int64()
    assert L.gbnf_image_flow_eps_floats(flow.handle, C.byref(per)) == 0 and per.value == 3072 - 24 * 8 * 8
    nb = C.c_int64()
    assert L.gbnf_image_flow_workspace_bytes(cond.handle, n, C.byref(nb)) == 0
    ws = torch.empty(nb.value // 4 + 1, dtype=torch.float32, device=dev)
    outs = {"z": torch.full((n,) + flow.z_shape, SENTINEL, device=dev), "eps": torch.full((n * per.value,), SENTINEL, device=dev),
            "ldj": torch.full((n,), SENTINEL, device=dev), "ll": torch.full((n,), SENTINEL, device=dev)}
    ptr = lambda t: C.c_void_p(t.data_ptr()) if t is not None else C.c_void_p(0)

    def enc(h, **kw):
        a = dict(x=xd, noise=nd, n=n, z=outs["z"], eps=outs["eps"], ldj=outs["ldj"], ll=outs["ll"], ws=ws, bytes=nb.value)
        a.update(kw)
        return L.gbnf_image_flow_encode(h, ptr(a["x"]), ptr(a["noise"]), a["n"], ptr(a["z"]), ptr(a["eps"]), ptr(a["ldj"]), ptr(a["ll"]),
                                        ptr(a["ws"]), a["bytes"], None)
    assert enc(None) == -1 and b"flow is null" in L.gbnf_last_error()
    for key in ("x", "z", "ldj", "ws"):
        assert enc(flow.handle, **{key: None}) == -1 and b"null" in L.gbnf_last_error(), key
    assert enc(flow.handle, eps=None) == -1 and b"need eps" in L.gbnf_last_error()          # a multi-level flow
    assert enc(flow.handle, bytes=1024) == -1 and b"workspace" in L.gbnf_last_error()
    assert enc(flow.handle, n=-1) == -1 and b"n < 0" in L.gbnf_last_error()
    assert enc(cond.handle) == -1 and b"needs y" in L.gbnf_last_error()                     # ll of a class-conditional handle
    assert enc(flow.handle, n=0) == 0
    torch.cuda.synchronize()
    for t in outs.values():
        assert bool((t == SENTINEL).all())
    # ... and the same calls with nothing wrong go through (a one-level flow has no eps to give)
    z1 = torch.full((n,) + one.z_shape, SENTINEL, device=dev)
    assert enc(one.handle, z=z1, eps=None) == 0
    assert enc(cond.handle, ll=None) == 0
    assert enc(flow.handle) == 0
    torch.cuda.synchronize()
    assert not any(bool((t == SENTINEL).any()) for t in list(outs.values()) + [z1])
