"""Per-body observations without a GPU: the exact reference (tests/observe_ref.py) on geometry whose answer is known, the binding's
column indices against the header, and the entry points' refusal of a NULL handle."""
import os
import re
from fractions import Fraction

import numpy as np
import pytest

import observe_ref
from tetsim_amd import _capi as capi
from tetsim_amd import make_lattice

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


@pytest.mark.parametrize("n", [2, 4])
def test_reference_on_the_lattice_gives_the_cube(n):
    """tetsim_amd.lattice: n cells of h = 1/n per side from (-1/2, y0, -1/2), every tet of rest volume +h^3/6.  h is a power of two
    here, so the f32 vertices are the documented ones exactly and the cube's volume, mass and centre come out as exact Fractions."""
    y0, density = 0.5, 1000.0
    v, t = make_lattice(n, y0=y0)
    h = Fraction(1, n)
    (o,) = observe_ref.observe(v, t, v, np.zeros_like(v), density)
    assert o["tets"] == 6 * n ** 3
    assert o["rest_volume"] == o["volume"] == (n * h) ** 3 == 1
    assert o["mass"] == Fraction(density) * o["volume"]
    assert o["com"] == [Fraction(0), Fraction(y0) + Fraction(1, 2), Fraction(0)]
    assert o["vcom"] == [0, 0, 0]
    assert o["inverted_tets"] == 0 and o["min_volume_ratio"] == 1 and o["min_abs_ratio"] == 1
    assert o["aabb_min"] == [-0.5, y0, -0.5] and o["aabb_max"] == [0.5, y0 + 1.0, 0.5]
    assert o["max_speed2"] == 0.0 and o["nonfinite"] == 0
    # S is a sum of absolute values: never below the value, and the bound made of it is far below anything f32 input can resolve
    assert all(o["S"][k] >= abs(o[k]) for k in ("mass", "volume", "rest_volume"))
    b = observe_ref.bounds(o)
    assert 0 < b["volume"] < Fraction(1, 10 ** 9) and all(0 < x < Fraction(1, 10 ** 9) for x in b["com"])


def test_reference_on_a_tet_pushed_through_its_face():
    rest = np.array([[0, 0, 0], [1, 0, 0], [0, 1, 0], [0, 0, 1]], np.float32)
    tets = np.array([[0, 1, 2, 3]], np.int32)
    pos = rest.copy()
    pos[3] = [0.0, 0.0, -0.5]                      # the apex, through the face z = 0
    vel = np.array([[1, 0, 0], [1, 0, 0], [1, 0, 0], [1, 2, 2]], np.float32)
    (o,) = observe_ref.observe(rest, tets, pos, vel, 600.0)
    assert o["rest_volume"] == Fraction(1, 6) and o["volume"] == Fraction(-1, 12)
    assert o["min_volume_ratio"] == Fraction(-1, 2) and o["min_volume_ratio"] < 0 and o["inverted_tets"] == 1
    assert o["mass"] == 100 and o["com"] == [Fraction(1, 4), Fraction(1, 4), Fraction(-1, 8)] and o["vcom"] == [1, Fraction(1, 2), Fraction(1, 2)]
    assert o["max_speed2"] == 9.0 and o["aabb_min"] == [0.0, 0.0, -0.5] and o["aabb_max"] == [1.0, 1.0, 0.0]
    flat = pos.copy()
    flat[3] = [0.25, 0.25, 0.0]                    # in the face: V == 0 counts as inverted (V/V0 <= 0)
    (o,) = observe_ref.observe(rest, tets, flat, vel, 600.0)
    assert o["min_volume_ratio"] == 0 and o["inverted_tets"] == 1


def test_reference_leaves_nonfinite_particles_out_of_the_box_only():
    rest = np.array([[0, 0, 0], [1, 0, 0], [0, 1, 0], [0, 0, 1], [5, 5, 5]], np.float32)
    tets = np.array([[0, 1, 2, 3]], np.int32)
    pos = rest.copy()
    pos[3] = np.nan
    pos[4, 1] = np.inf
    (o,) = observe_ref.observe(rest, tets, pos, np.zeros_like(pos), 1.0)
    assert o["nonfinite"] == 2 and o["aabb_max"] == [1.0, 1.0, 0.0]
    assert all(np.isnan(c) for c in o["com"]) and np.isnan(o["volume"]) and o["vcom"] == [0, 0, 0]
    assert o["min_volume_ratio"] == float("inf") and o["inverted_tets"] == 0
    (o,) = observe_ref.observe(rest[:4], np.zeros((0, 4), np.int32), rest[:4], rest[:4], 1.0)   # no tets
    assert o["mass"] == 0 and o["com"] == [0, 0, 0] and o["min_volume_ratio"] == float("inf") and o["max_speed2"] == 1.0


def test_binding_matches_the_header():
    header = open(os.path.join(ROOT, "include", "tetsim.h")).read()
    assert int(re.search(r"#define TETSIM_OBS_WIDTH (\d+)", header).group(1)) == capi.OBS_WIDTH == 20
    names = dict((n, int(v)) for n, v in re.findall(r"TETSIM_(OBS_[A-Z0-9_]+) = (\d+)", header))
    assert len(names) == 12
    for n, v in names.items():
        assert getattr(capi, n) == v, n
    for s in ("tetsim_observe_bodies_device", "tetsim_read_body_observations"):
        assert s in capi.SYMBOLS and s in capi.OPTIONAL_SYMBOLS


def test_entry_points_refuse_a_null_handle():
    L = capi.lib()
    out = np.zeros(capi.OBS_WIDTH)
    assert L.tetsim_observe_bodies_device(None, None, 0, None) == capi.EINVAL
    assert L.tetsim_observe_bodies_device(None, out.ctypes.data, 160, None) == capi.EINVAL
    assert L.tetsim_read_body_observations(None, out.ctypes.data_as(capi.C.POINTER(capi.C.c_double))) == capi.EINVAL
    assert not out.any()
