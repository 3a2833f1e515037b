"""CPU: the full-latent direction of an image Glow component (gbnf_image_flow_encode) on the host -- the float64 yardstick
(tests/image_latent_oracle.py) against the oracle's forward and inverse, the reference anchor on the g16 decode fixtures, the ABI
entry and the refusals that need no device."""
import ctypes as C
import types

import numpy as np
import pytest
import torch

import image_latent_oracle as ilo
from conftest import IMAGE_DECODE_CASES, load_image_decode_case
from oracle import gbnf_oracle as oracle

X_ATOL = 5e-5        # the bar for x of tests/test_hip_image.py (a pixel intensity in [0, 1]: absolute)


@pytest.mark.parametrize("name", list(ilo.GEOMETRIES))
def test_yardstick_is_the_oracle_forward_with_the_halves_kept(name):
    sp, size, x, noise = ilo.geometry(name, 3)
    z, eps, ldj, u = ilo.encode(sp, x, noise)
    z_or, _, _, ld_or, _ = oracle.image_component_forward(sp, x, noise, dtype=torch.float64)
    assert np.array_equal(z, z_or) and np.array_equal(ldj, ld_or)
    assert [tuple(e.shape[1:]) for e in eps] == [tuple(s) for s in oracle.image_split_shapes(sp, size)]
    assert u.shape == x.shape and z.dtype == np.float64


@pytest.mark.parametrize("name", list(ilo.GEOMETRIES))
def test_inverse_of_the_yardstick_returns_the_dequantised_input(name):
    """oracle.image_component_inverse(z, eps, 1.0) == u: below 1e-12 in float64; in float32 (torch-CPU, the arithmetic of the
    device's exact-f32 path) below X_ATOL / 2 -- the condition that the inputs themselves leave the device half of the bar."""
    sp, size, x, noise = ilo.geometry(name, 3)
    z, eps, _, u = ilo.encode(sp, x, noise)
    e64 = ilo.max_abs(oracle.image_component_inverse(sp, z, eps, 1.0, dtype=torch.float64), u)
    z32, eps32, _, u32 = ilo.encode(sp, x, noise, dtype=torch.float32)
    e32 = ilo.max_abs(oracle.image_component_inverse(sp, z32, eps32, 1.0, dtype=torch.float32), u32)
    print(f"{name}: round trip float64 {e64:.2e}, float32 {e32:.2e}")
    assert e64 < 1e-12
    assert e32 < X_ATOL / 2


@pytest.mark.parametrize("name", IMAGE_DECODE_CASES)
def test_yardstick_takes_the_reference_decode_back(name):
    """g16: the reference's Glow.decode(z, None, temperature) with Split2d's draws injected.  Encoding its image with noise = x_ref
    (so that u = (255 x + x) / 256 = x_ref) gives back the fixture's z and temperature * eps.  x_ref reaches -0.05 and 1.05 (the
    logit's bounds): nothing clamps, no mask."""
    cfg, spec, z, eps, x_ref = load_image_decode_case(name)
    zy, ey, _, u = ilo.encode(spec, x_ref, x_ref)
    assert ilo.max_abs(u, x_ref) < 1e-7
    ez = ilo.max_abs(zy, z)
    ee = max(ilo.max_abs(a, cfg["temperature"] * b.astype(np.float64)) for a, b in zip(ey, eps))
    print(f"{name}: z {ez:.2e}, eps {ee:.2e}")
    assert ez <= 2e-4 * max(1.0, float(np.abs(z).max()))
    assert ee <= 2e-4 * max(1.0, max(float(np.abs(b).max()) for b in eps) * cfg["temperature"])


def test_abi_entry_and_refusals_without_a_device():
    from gbnf_amd import native
    assert "gbnf_image_flow_encode" in native.ABI_SYMBOLS
    L = native.lib()
    assert L.gbnf_image_flow_encode.argtypes == [C.c_void_p] * 3 + [C.c_int64] + [C.c_void_p] * 5 + [C.c_int64, C.c_void_p]
    buf = (C.c_float * 16)()
    p = C.cast(buf, C.c_void_p)
    for n in (1, 0, -1):                                             # a null flow is refused before anything else
        assert L.gbnf_image_flow_encode(None, p, p, n, p, p, p, p, p, 64, None) == -1
        assert b"gbnf_image_flow_encode" in L.gbnf_last_error() and b"null" in L.gbnf_last_error()
    assert not any(buf)


@pytest.mark.parametrize("name", list(ilo.GEOMETRIES))
def test_eps_list_shapes_are_split_shapes(name):
    """The eps list of the yardstick has the shapes NativeImageFlow.split_shapes() states (the method needs no handle)."""
    from gbnf_amd import native
    sp, size, x, noise = ilo.geometry(name, 2)
    stub = types.SimpleNamespace(input_size=tuple(size), n_levels=len(sp["levels"]))
    shapes = native.NativeImageFlow.split_shapes(stub)
    _, eps, _, _ = ilo.encode(sp, x, noise)
    assert [tuple(e.shape) for e in eps] == [(2,) + tuple(s) for s in shapes]
    assert sum(int(np.prod(s)) for s in shapes) == int(np.prod(size)) - int(np.prod(ilo.encode(sp, x, noise)[0].shape[1:]))
    assert hasattr(native.NativeImageFlow, "encode")
