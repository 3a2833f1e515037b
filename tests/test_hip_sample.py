"""GPU: drawing from the mixture -- the per-row component draw, the stable partition by component and the per-segment inverses
(gbnf_mixture_sample_begin / _finish, native.mixture_sample) and the modules' ``sample``.

The cases and their preconditions are tests/test_sample_host.py's.  Every call is checked the same way (``_check_call``):
  comp   == the numpy restatement of the draw, exactly (the host test keeps every u * T 1e-6 T away from the cdf edges);
  order  a permutation of range(n), ascending inside every segment, comp[order[segment c]] == c;  counts == bincount(comp);
  x, ldj within X_BAR / ILD_BAR (tests/test_hip_inverse.py) of oracle.component_inverse(specs[comp[i]], z[i], backend="numpy64");
  x[rows_c], ldj[rows_c] bit-equal to NativeFlow.inverse(z[rows_c]) of component c: the same rows at the same n are the same launch.
"""
import argparse
import ctypes as C

import numpy as np
import pytest

import test_image_boost_host as image_host
import test_sample_host as host
from test_hip_inverse import ILD_BAR, X_BAR, _deviation

pytestmark = pytest.mark.gpu
ROUND_TRIP_BAR = 2e-5          # test_hip_parity.test_inverse_matches_oracle_and_round_trips: 2e-5 of the data's scale

_FLOWS = {}


def _dev():
    import torch
    assert torch.cuda.is_available(), "GPU tests need the MI355X"
    return torch.device("cuda:0")


def _flows(geometry, math):
    """The geometry's components as NativeFlow handles in one math mode: created once per process."""
    from gbnf_amd import native
    key = (geometry[0], math)
    if key not in _FLOWS:
        _FLOWS[key] = [native.NativeFlow(s, math=math) for s in host.specs_of(geometry)]
    return _FLOWS[key]


def _t(a):
    import torch
    return torch.from_numpy(np.ascontiguousarray(a).copy()).to(_dev())


def _check_partition(tag, comp, order, counts, want_comp, n_components):
    comp, order, counts = comp.cpu().numpy(), order.cpu().numpy(), counts.cpu().numpy()
    n = want_comp.shape[0]
    assert comp.dtype == np.int32 and order.dtype == np.int64 and counts.dtype == np.int64
    assert np.array_equal(comp, want_comp), (tag, int((comp != want_comp).sum()))
    assert np.array_equal(counts, np.bincount(want_comp, minlength=n_components)), (tag, counts)
    assert np.array_equal(np.sort(order), np.arange(n)), tag
    begin = 0
    for c in range(n_components):
        seg = order[begin:begin + counts[c]]
        begin += counts[c]
        assert (comp[seg] == c).all(), (tag, c)
        assert (np.diff(seg) > 0).all(), (tag, c)
    assert begin == n


def _check_call(tag, flows, rho, u, z, want_comp, x64, ild64, n_used=None, alias=False):
    """One begin / finish pair checked as the module docstring says; returns (x, ldj, comp, order)."""
    import torch
    from gbnf_amd import native
    n_used = len(flows) if n_used is None else n_used
    rho_d, u_d, z_d = _t(rho), _t(u), _t(z)
    comp, order, counts, _ = native.mixture_partition(rho_d, u_d, n_used, z_d)
    _check_partition(tag, comp, order, counts, want_comp, n_used)
    z_in = z_d.clone() if alias else z_d
    x, ldj, comp2 = native.mixture_sample(flows, rho_d, u_d, z_in, n_used=n_used, out=z_in if alias else None)
    torch.cuda.synchronize()
    assert torch.equal(comp2, comp), tag
    assert (x.data_ptr() == z_in.data_ptr()) == alias
    assert bool(torch.isfinite(x).all()) and bool(torch.isfinite(ldj).all()), tag
    dx, dl = _deviation(x, ldj, x64, ild64)
    print("SAMPLEDEV", *tag, f"dx {dx:.3e} dild {dl:.3e} counts {counts.cpu().tolist()}")
    assert dx <= X_BAR, (tag, dx)
    assert dl <= ILD_BAR, (tag, dl)
    for c in range(n_used):
        rows = torch.nonzero(comp == c).flatten()
        if rows.numel():
            xs, ls = flows[c].inverse(z_d[rows].contiguous())
            assert torch.equal(x[rows], xs) and torch.equal(ldj[rows], ls), (tag, c)
    x2, none, _ = native.mixture_sample(flows, rho_d, u_d, z_d, n_used=n_used, want_ldj=False)
    assert none is None and torch.equal(x2, x), tag
    return x, ldj, comp, order


# ------------------------------------------------------------------ draw, partition, values
@pytest.mark.parametrize("math", ["default", "f32"])
@pytest.mark.parametrize("case", host.CASES, ids=host.case_id)
def test_draw_partition_and_values(case, math):
    specs, rho, u, comp, z, x64, ild64 = host.case_reference(case)
    _check_call((host.case_id(case), math), _flows(case[0], math), rho, u, z, comp, x64, ild64)


# ------------------------------------------------------------------ edges
def _edge(name, geometry, rho, u, n_used=None, math="default", **kw):
    """A call on `geometry`'s first n_used components with a rho and u of the test's own; the margin rule of the case lists holds."""
    specs = host.specs_of(geometry)[: n_used or len(host.specs_of(geometry))]
    rho, u = np.asarray(rho, dtype=np.float32), np.asarray(u, dtype=np.float32)
    n = u.shape[0]
    assert host.edge_margin(rho, u, len(specs)) >= host.EDGE_MARGIN
    comp, z, x64, ild64 = host.mixture_reference(specs, rho[:len(specs)], u, n, 77 + n, "edge-" + name)
    flows = _flows(geometry, math)
    return _check_call((name, math), flows, rho, u, z, comp, x64, ild64, n_used=len(specs), **kw) + (comp,)


def test_fewer_components_used_than_the_model_holds():
    g = host.GEOMETRIES[1]                                  # C = 4, the first 2 used: rho[2:] must not enter the cdf
    comp = _edge("n_used", g, host.decreasing_rho(4), host.uniforms(100), n_used=2)[-1]
    assert set(comp.tolist()) == {0, 1}


def test_a_component_of_zero_weight_gets_no_row():
    comp = _edge("zero-weight", host.GEOMETRIES[0], [1.0, 0.0, 0.5], host.uniforms(100))[-1]
    assert set(comp.tolist()) == {0, 2}


def test_one_segment_holds_everything():
    comp = _edge("one-segment", host.GEOMETRIES[0], host.decreasing_rho(3), 0.5 * host.uniforms(100))[-1]      # the first edge: 1 / 1.75
    assert set(comp.tolist()) == {0}


def test_a_single_component():
    comp = _edge("single", host.GEOMETRIES[3], host.decreasing_rho(8), host.uniforms(17), n_used=1)[-1]
    assert set(comp.tolist()) == {0}


def test_several_partition_chunks_and_a_ragged_last_one():
    n = 3 * host.CHUNK + 77
    u = host.uniforms(n)
    assert (n + host.CHUNK - 1) // host.CHUNK >= 3 and n % host.CHUNK
    for g in (host.GEOMETRIES[2], host.GEOMETRIES[3]):      # C = 2 at d = 6, C = 8 at d = 21
        comp = _edge("chunks-" + g[0], g, host.decreasing_rho(g[2]), u)[-1]
        chunk_of = np.arange(n) // host.CHUNK
        assert all(len(set(chunk_of[comp == c].tolist())) >= 3 for c in range(2))      # segments gather rows of every chunk


def test_x_may_overwrite_z():
    _edge("alias", host.GEOMETRIES[0], host.decreasing_rho(3), host.uniforms(100), alias=True)


def test_two_identical_calls_are_bit_equal():
    import torch
    from gbnf_amd import native
    case = (host.GEOMETRIES[3], 1000)
    specs, rho, u, comp, z, x64, ild64 = host.case_reference(case)
    flows = _flows(case[0], "default")
    rho_d, u_d, z_d = _t(rho), _t(u), _t(z)
    outs = []
    for _ in range(2):
        part = native.mixture_partition(rho_d, u_d, len(flows), z_d)[:3]
        outs.append(tuple(t.clone() for t in part + native.mixture_sample(flows, rho_d, u_d, z_d)))
    for a, b in zip(*outs):
        assert torch.equal(a, b)


# ------------------------------------------------------------------ refusals
def test_refusals_launch_nothing_and_a_good_call_still_works():
    import torch
    from gbnf_amd import native
    dev = _dev()
    L = native.lib()
    case = (host.GEOMETRIES[0], 100)
    specs, rho, u, comp, z, x64, ild64 = host.case_reference(case)
    flows = _flows(case[0], "default")
    other = _flows(host.GEOMETRIES[1], "default")           # d = 21
    n, d, nc = 100, 43, 3
    rho_d, u_d, z_d = _t(rho), _t(u), _t(z)
    comp_d = torch.full((n,), -5, dtype=torch.int32, device=dev)
    order_d = torch.full((n,), -5, dtype=torch.int64, device=dev)
    counts_d = torch.full((nc,), -5, dtype=torch.int64, device=dev)
    x_d = torch.full((n, d), 7.0, device=dev)
    ldj_d = torch.full((n,), 7.0, device=dev)
    nb = host.workspace_bytes(nc, n, d)
    ws = torch.zeros(nb // 4, dtype=torch.float32, device=dev)
    p = lambda t: C.c_void_p(t.data_ptr())
    handles = (C.c_void_p * nc)(*[f.handle for f in flows])
    mixed = (C.c_void_p * nc)(flows[0].handle, other[1].handle, flows[2].handle)
    holed = (C.c_void_p * nc)(flows[0].handle, None, flows[2].handle)
    counts = lambda *v: (C.c_int64 * nc)(*v)

    def begin(rho=rho_d, n_used=nc, u=u_d, z=z_d, n=n, d=d, comp=comp_d, order=order_d, cnt=counts_d, w=ws, wb=nb):
        q = lambda t: p(t) if t is not None else None
        return L.gbnf_mixture_sample_begin(q(rho), n_used, q(u), q(z), n, d, q(comp), q(order), q(cnt), q(w), wb, None)

    def finish(fl=handles, n_flows=nc, cnt=counts(59, 33, 8), order=order_d, n=n, x=x_d, ldj=ldj_d, w=ws, wb=nb):
        q = lambda t: p(t) if t is not None else None
        return L.gbnf_mixture_sample_finish(fl, n_flows, cnt, q(order), n, q(x), q(ldj), q(w), wb, None)

    refused = [
        ("begin: null rho", lambda: begin(rho=None)), ("begin: null u", lambda: begin(u=None)), ("begin: null comp", lambda: begin(comp=None)),
        ("begin: null order", lambda: begin(order=None)), ("begin: null counts", lambda: begin(cnt=None)),
        ("begin: null workspace", lambda: begin(w=None)), ("begin: n = 0", lambda: begin(n=0)), ("begin: n_used = 0", lambda: begin(n_used=0)),
        ("begin: short workspace", lambda: begin(wb=nb - 1)),
        ("finish: null flows", lambda: finish(fl=None)), ("finish: a null flow", lambda: finish(fl=holed)),
        ("finish: null counts", lambda: finish(cnt=None)), ("finish: null order", lambda: finish(order=None)),
        ("finish: null x", lambda: finish(x=None)), ("finish: null workspace", lambda: finish(w=None)),
        ("finish: n = 0", lambda: finish(n=0)), ("finish: n_flows = 0", lambda: finish(n_flows=0)),
        ("finish: counts sum to n - 1", lambda: finish(cnt=counts(59, 33, 7))), ("finish: counts sum to n + 1", lambda: finish(cnt=counts(59, 33, 9))),
        ("finish: a negative count", lambda: finish(cnt=counts(101, -1, 0))),
        ("finish: flows of another d", lambda: finish(fl=mixed)), ("finish: short workspace", lambda: finish(wb=nb - 1)),
    ]
    for what, call in refused:
        assert call() == -1, f"{what}: accepted"
        assert L.gbnf_last_error(), what
    torch.cuda.synchronize()
    assert bool((comp_d == -5).all()) and bool((order_d == -5).all()) and bool((counts_d == -5).all())
    assert bool((x_d == 7.0).all()) and bool((ldj_d == 7.0).all()) and bool((ws == 0).all())
    # the same buffers, a good pair of calls
    assert begin() == 0
    got = counts_d.cpu().tolist()
    assert got == np.bincount(comp, minlength=nc).tolist()
    assert finish(cnt=counts(*got)) == 0
    torch.cuda.synchronize()
    dx, dl = _deviation(x_d, ldj_d, x64, ild64)
    assert dx <= X_BAR and dl <= ILD_BAR
    assert np.array_equal(comp_d.cpu().numpy(), comp)
    _check_call(("after-refusals", "default"), flows, rho, u, z, comp, x64, ild64)


# ------------------------------------------------------------------ modules
def _tabular_model(geometry, dev):
    import torch
    from gbnf_amd import BoostedFlow
    name, kind, nc, d, h, K, kw = geometry
    args = argparse.Namespace(
        num_flows=K, z_size=d, density_evaluation=True, device=dev, cuda=True, component_type=kind, num_components=nc,
        rho_init="decreasing", learn_top=False, y_classes=0, y_condition=False, sample_size=5, input_size=[d], h_size=h, num_blocks=1,
        actnorm_scale=1.0, flow_permutation=kw.get("permutation", "shuffle"), flow_coupling=kw.get("coupling", "affine"),
        LU_decomposed=False, num_dequant_blocks=0, coupling_network="tanh", coupling_network_depth=1, batch_norm=True)
    m = BoostedFlow(args)
    for c, spec in enumerate(host.specs_of(geometry)):
        m.load_spec(c, spec)
    m.eval()
    m.all_trained = True
    return m


@pytest.mark.parametrize("geometry", [host.GEOMETRIES[0], host.GEOMETRIES[1]], ids=lambda g: g[0])
def test_boosted_flow_sample(geometry):
    import torch
    dev = _dev()
    m = _tabular_model(geometry, dev)
    nc, d = geometry[2], geometry[3]
    assert np.array_equal(m.rho.cpu().numpy(), host.decreasing_rho(nc))
    # explicit z and uniforms: shapes, components, the density the rows were drawn from, and the way back
    n = 100
    u = host.uniforms(n)
    z = _t(np.random.RandomState(5).standard_normal((n, d)).astype(np.float32))
    x, comp, lp = m.sample(z=z, uniforms=_t(u), return_components=True, return_log_prob=True)
    assert x.shape == (n, d) and comp.shape == (n,) and comp.dtype == torch.int32 and lp.shape == (n,)
    assert np.array_equal(comp.cpu().numpy(), host.numpy_draw(host.decreasing_rho(nc), u)[0])
    assert torch.equal(lp, m.log_prob(x)) and bool(torch.isfinite(lp).all())
    assert torch.equal(m.sample(z=z, uniforms=_t(u)), x)
    for c in range(nc):
        rows = torch.nonzero(comp == c).flatten()
        if rows.numel():
            back, _ = m.component_forward(x[rows].contiguous(), c)
            err = float((back - z[rows]).abs().max())
            print(f"ROUNDTRIP {geometry[0]} c{c} rows {rows.numel()} err {err:.3e}")
            assert err <= ROUND_TRIP_BAR * max(1.0, float(z[rows].abs().max()))
            assert torch.equal(x[rows], m.component_inverse(z[rows].contiguous(), c)[0])
    # n_used: only the first components are drawn, and log_prob is that mixture's
    x2, comp2, lp2 = m.sample(z=z, uniforms=_t(u), n_used=2, return_components=True, return_log_prob=True)
    assert np.array_equal(comp2.cpu().numpy(), host.numpy_draw(host.decreasing_rho(nc), u, 2)[0])
    assert torch.equal(lp2, m.log_prob(x2, 2))
    # defaults: sample_size rows, z = randn * temperature then uniforms = rand from the generator
    gen = torch.Generator(device=dev)
    gen.manual_seed(11)
    a = m.sample(generator=gen, temperature=0.7)
    assert a.shape == (5, d) and a.dtype == torch.float32 and bool(torch.isfinite(a).all())
    gen.manual_seed(11)
    b, cb = m.sample(generator=gen, temperature=0.7, return_components=True)
    assert torch.equal(a, b)
    gen.manual_seed(11)
    zz = torch.randn(5, d, device=dev, generator=gen) * 0.7
    uu = torch.rand(5, device=dev, generator=gen)
    c_, cc = m.sample(z=zz, uniforms=uu, return_components=True)
    assert torch.equal(c_, a) and torch.equal(cc, cb)
    assert m.sample(7).shape == (7, d)
    with pytest.raises(ValueError):
        m.sample(z=z, uniforms=_t(u[:50]))
    with pytest.raises(ValueError):
        m.sample(3, n_used=nc + 1)


def test_boosted_image_flow_sample():
    import torch
    from gbnf_amd import BoostedFlow, image_glow, synth
    dev = _dev()
    size, n, nc, T = (1, 16, 16), 7, 3, 0.7
    torch.manual_seed(0)
    m = BoostedFlow(image_host.image_args(size, 32, 2, 2, dev, C_=nc))
    assert isinstance(m, image_glow.BoostedImageFlow)
    for c in range(nc):
        image_glow.load_image_spec(m.flows[c], synth.synth_image_glow_spec(size, h=32, K=2, L=2, seed=410 + c))
    m.eval()
    m.all_trained = True
    rng = np.random.RandomState(3)
    handle = m.native_flow(0)
    e = _t(rng.standard_normal((n,) + tuple(handle.z_shape)).astype(np.float32))
    eps = [_t(rng.standard_normal((n,) + sh).astype(np.float32)) for sh in handle.split_shapes()]
    u = host.uniforms(n)
    rho = m.rho.cpu().numpy()
    assert host.edge_margin(rho, u) >= host.EDGE_MARGIN
    want = host.numpy_draw(rho, u)[0]
    assert len(set(want.tolist())) >= 2
    x, comp = m.sample(temperature=T, e=e, eps=eps, uniforms=_t(u), return_components=True)
    assert x.shape == (n,) + size and np.array_equal(comp.cpu().numpy(), want)
    for c in range(nc):
        rows = torch.nonzero(comp == c).flatten()
        if rows.numel():
            mu, lv = m._prior_on(m.native_flow(c), dev)
            z_c = mu + torch.exp(lv) * T * e[rows]
            assert torch.equal(x[rows], m.decode(z_c, None, T, c, eps=[t[rows].contiguous() for t in eps])), c
    gen = torch.Generator(device=dev)
    gen.manual_seed(3)
    a = m.sample(generator=gen)
    gen.manual_seed(3)
    assert a.shape == (4,) + size and torch.equal(a, m.sample(generator=gen))
