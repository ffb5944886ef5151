"""Placement (include/tetsim.h: tetsim_place_bodies / _device), as far as a machine without a GPU can see it: declared, exported,
prototyped in the ctypes binding, wrapped by SoftBodyHIP -- and the properties of the numpy statement of its definition
(tests/place_ref.py) that the GPU tests lean on."""
import ctypes as C
import inspect
import os
import re

import numpy as np

import place_ref
from conftest import ROOT
from tetsim_amd import SoftBodyHIP, place_rows
from tetsim_amd import _capi as capi

NEW = ("tetsim_place_bodies_device", "tetsim_place_bodies")


def test_the_symbols_are_declared_and_exported():
    header = open(os.path.join(ROOT, "include", "tetsim.h")).read()
    L = capi.lib()
    for s in NEW:
        assert re.search(r"\bint %s\s*\(tetsim_handle h," % s, header), s
        assert s in capi.SYMBOLS and s in capi.OPTIONAL_SYMBOLS and hasattr(L, s), s
    assert L.tetsim_abi_version() == 5   # additive: the ABI version stays


def test_the_ctypes_prototypes_and_constants_match_the_header():
    L = capi.lib()
    vp, u64, u32 = C.c_void_p, C.c_uint64, C.c_uint32
    assert L.tetsim_place_bodies_device.argtypes == [vp, vp, u64, vp, u32, vp]
    assert L.tetsim_place_bodies.argtypes == [vp, C.POINTER(C.c_float), C.POINTER(C.c_uint8), u32]
    for s in NEW:
        assert getattr(L, s).restype == C.c_int, s
    header = open(os.path.join(ROOT, "include", "tetsim.h")).read()
    for name in ("WIDTH", "Q", "PIVOT", "OFFSET", "LINEAR", "ANGULAR"):
        value = int(re.search(r"TETSIM_PLACE_%s\s*=?\s*(\d+)" % name, header).group(1))
        assert getattr(capi, "PLACE_" + name) == value == getattr(place_ref, name), name
    assert re.search(r"TETSIM_PLACE_KEEP_VELOCITY = 1u << 0", header) and capi.PLACE_KEEP_VELOCITY == 1


def test_a_null_handle_is_refused_without_a_device():
    L = capi.lib()
    assert L.tetsim_place_bodies_device(None, None, 0, None, 0, None) == capi.EINVAL
    assert L.tetsim_place_bodies(None, None, None, 0) == capi.EINVAL


def test_the_python_methods_exist():
    want = {"placeBodiesDevice": ["self", "rows", "bodies", "keep_velocity", "stream"],
            "placeBodies": ["self", "rows", "bodies", "keep_velocity"]}
    for name, args in want.items():
        assert list(inspect.signature(getattr(SoftBodyHIP, name)).parameters) == args, name
    rows = place_rows([[0, 0, 0, 1], [1, 0, 0, 0]], pivot=(1, 2, 3), offset=[[4, 5, 6], [7, 8, 9]], angular=(0, 0, 1))
    assert rows.dtype == np.float32 and rows.shape == (2, 16)
    assert rows[1].tolist() == [1, 0, 0, 0, 1, 2, 3, 7, 8, 9, 0, 0, 0, 0, 0, 1]


# ---- properties of the reference ------------------------------------------------------------------------------------------------------
def state(seed=3, n=97):
    rng = np.random.default_rng(seed)
    pos = rng.uniform(-2.0, 2.0, (n, 3)).astype(np.float32)
    pos[0] = [0.0, -0.0, 1.5]                        # signed zeros compare equal by value
    vel = rng.uniform(-3.0, 3.0, (n, 3)).astype(np.float32)
    q = rng.standard_normal((n, 4)).astype(np.float32)
    q /= np.linalg.norm(q, axis=1, keepdims=True).astype(np.float32)
    corners = rng.uniform(-0.3, 0.3, (n, 4, 3)).astype(np.float32)
    return pos, vel, q, corners


HALVES = place_rows([0.5, 0.5, 0.5, 0.5])[0]         # the rotation by 120 degrees about (1,1,1): e_x -> e_y -> e_z -> e_x


def test_the_half_quaternion_is_exactly_the_cyclic_permutation():
    pos, vel, q, corners = state()
    p1, v1 = place_ref.place_particles(HALVES, pos, vel, keep_velocity=True)
    assert np.array_equal(p1, pos[:, [2, 0, 1]]) and np.array_equal(v1, vel[:, [2, 0, 1]])
    assert np.array_equal(place_ref.place_points(HALVES, pos), pos[:, [2, 0, 1]])
    assert np.array_equal(place_ref.place_shape_centred(HALVES, corners), corners[..., [2, 0, 1]])
    assert np.array_equal(place_ref.place_shape_absolute(HALVES, corners), corners[..., [2, 0, 1]])
    p0, v0 = place_ref.place_particles(HALVES, pos, vel)
    assert np.array_equal(p0, p1) and not v0.any()   # without KEEP_VELOCITY: linear = angular = 0 leaves the body at rest
    # qR (x) identity = qR, exactly
    assert np.array_equal(place_ref.place_quats(HALVES, [[0, 0, 0, 1]]), [[0.5, 0.5, 0.5, 0.5]])


def test_the_identity_row_with_keep_velocity_returns_its_input():
    pos, vel, q, corners = state()
    ident = place_rows([0, 0, 0, 1])[0]
    p1, v1 = place_ref.place_particles(ident, pos, vel, keep_velocity=True)
    assert np.array_equal(p1, pos) and np.array_equal(v1, vel)
    assert np.array_equal(place_ref.place_quats(ident, q), q)
    assert np.array_equal(place_ref.place_shape_centred(ident, corners), corners)
    assert np.array_equal(place_ref.place_shape_absolute(ident, corners), corners)
    # ... and so does a pivot with no offset, where p - pivot + pivot is exact: small integers
    grid = np.array([[1, 2, 3], [-4, 0, 2]], np.float32)
    assert np.array_equal(place_ref.place_points(place_rows([0, 0, 0, 2], pivot=(1, 1, 1))[0], grid), grid)


def test_a_quaternion_followed_by_its_conjugate_returns_the_permuted_input_exactly():
    pos, vel, q, corners = state()
    conj = place_rows([-0.5, -0.5, -0.5, 0.5])[0]
    p1, v1 = place_ref.place_particles(HALVES, pos, vel, keep_velocity=True)
    p2, v2 = place_ref.place_particles(conj, p1, v1, keep_velocity=True)
    assert np.array_equal(p2, pos) and np.array_equal(v2, vel)
    assert np.array_equal(place_ref.place_shape_centred(conj, place_ref.place_shape_centred(HALVES, corners)), corners)
    # the quaternion product with halves is sums of halves of the components: back within an ulp of each component's sum
    back = place_ref.place_quats(conj, place_ref.place_quats(HALVES, q))
    assert np.abs(back - q).max() <= 2.0 ** -23


def test_an_unnormalised_quaternion_gives_what_its_normalised_form_gives():
    pos, vel, q, corners = state()
    # a scale by a power of two commutes with every rounding, so the two rows give the same values; any other scale stays within f32 rounding
    a = np.array([0.3, -0.7, 0.2, 0.6], np.float32)
    row = lambda qq: place_rows(qq, pivot=(0.5, 1.0, -0.25), offset=(1, 2, 3), linear=(0.1, 0.2, 0.3), angular=(1, -2, 0.5))[0]
    for keep in (False, True):
        r1, r4 = place_ref.place_particles(row(a), pos, vel, keep), place_ref.place_particles(row(4 * a), pos, vel, keep)
        assert np.array_equal(r1[0], r4[0]) and np.array_equal(r1[1], r4[1])
    assert np.array_equal(place_ref.place_quats(row(a), q), place_ref.place_quats(row(4 * a), q))
    n64 = a.astype(np.float64) / np.linalg.norm(a.astype(np.float64))
    unit = n64.astype(np.float32)
    p_a, _ = place_ref.place_particles(row(a), pos, vel)
    p_u, _ = place_ref.place_particles(row(unit), pos, vel)
    assert np.abs(p_a - p_u).max() <= 8 * 2.0 ** -23 * 4.0   # f32 rounding of the unit row's components, on coordinates below 4


def test_rows_the_device_leaves_alone():
    good = place_rows([0.3, -0.7, 0.2, 0.6], pivot=(1, 2, 3))[0]
    assert place_ref.row_ok(good)
    for k in range(16):
        bad = good.copy()
        bad[k] = np.nan
        assert not place_ref.row_ok(bad), k
        bad[k] = np.inf
        assert not place_ref.row_ok(bad), k
    assert not place_ref.row_ok(place_rows([0, 0, 0, 0])[0])
    assert place_ref.row_ok(place_rows([1e-30, 0, 0, 0])[0])   # tiny but not 0: the squares are f64
