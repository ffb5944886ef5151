"""Body pins (include/tetsim.h: tetsim_set_body_pins / _device, tetsim_prep_pin_slots), as far as a machine without a GPU can see them: the
normalisation -- a row outside its body or with a non-finite target holds nothing, the lowest row wins a particle -- against a restatement
in numpy, and the symbols declared, exported, prototyped and wrapped."""
import ctypes as C
import inspect
import os
import re

import numpy as np
import pytest

from conftest import ROOT
from tetsim_amd import SoftBodyHIP, prep_pin_slots
from tetsim_amd import _capi as capi

NEW = ("tetsim_set_body_pins", "tetsim_set_body_pins_device", "tetsim_prep_pin_slots")


def _restated(particles, targets, counts):
    """the rule of the header, row by row"""
    particles, targets = np.asarray(particles, np.int64), np.asarray(targets, np.float32)
    k = particles.shape[1]
    out = []
    for b, n in enumerate(counts):
        slot = np.full(n, -1, np.int32)
        for j in range(k):
            p = particles[b, j]
            if 0 <= p < n and np.isfinite(targets[b, j]).all() and slot[p] < 0:
                slot[p] = b * k + j
        out.append(slot)
    return np.concatenate(out) if out else np.zeros(0, np.int32)


def _targets(shape, seed=0):
    return np.random.default_rng(seed).uniform(-1, 1, shape + (3,)).astype(np.float32)


def _check(particles, targets, counts):
    got = prep_pin_slots(particles, targets, counts)
    want = _restated(particles, targets, counts)
    assert got.dtype == np.int32 and np.array_equal(got, want), (got, want)
    return got


def test_indices_outside_the_body_hold_nothing():
    counts = [5, 5, 5]
    p = [[-1, 2], [-7, 3], [5, 4]]   # unused, below the body, one behind its last particle
    got = _check(p, _targets((3, 2)), counts)
    assert got.tolist() == [-1, -1, 1, -1, -1, -1, -1, -1, 3, -1, -1, -1, -1, -1, 5]


@pytest.mark.parametrize("bad", [np.nan, np.inf, -np.inf])
@pytest.mark.parametrize("component", [0, 1, 2])
def test_a_non_finite_target_component_holds_nothing(bad, component):
    t = _targets((2, 3))
    t[1, 1, component] = bad
    got = _check([[0, 1, 2], [0, 1, 2]], t, [4, 4])
    assert got.tolist() == [0, 1, 2, -1, 3, -1, 5, -1]


def test_the_lowest_row_wins_a_particle_named_twice():
    got = _check([[3, 1, 3, 3], [2, 2, 0, 2]], _targets((2, 4)), [4, 3])
    assert got.tolist() == [-1, 1, -1, 0, 6, -1, 4]


def test_a_duplicate_behind_an_invalid_row_wins():
    t = _targets((1, 3))
    t[0, 0, 2] = np.nan   # row 0 names particle 2 but cannot hold it: row 2 does
    got = _check([[2, 0, 2]], t, [3])
    assert got.tolist() == [1, -1, 2]


def test_one_row_per_body_and_a_row_per_particle():
    _check([[1], [-1], [0]], _targets((3, 1)), [2, 2, 2])
    n = 7
    full = _check([list(range(n))[::-1]], _targets((1, n)), [n])
    assert full.tolist() == list(range(n))[::-1]


def test_bodies_of_different_sizes():
    counts = [1, 9, 0, 4]
    rng = np.random.default_rng(3)
    p = rng.integers(-2, 10, size=(4, 6))
    t = _targets((4, 6), 4)
    t[rng.integers(0, 4, 5), rng.integers(0, 6, 5), rng.integers(0, 3, 5)] = np.nan
    got = _check(p, t, counts)
    assert len(got) == sum(counts) and (got >= 0).any() and (got < 0).any()
    # a row is a row of ITS body: body 3's rows never reach into body 1
    first = np.cumsum([0] + counts)
    for b in range(4):
        held = got[first[b]:first[b + 1]]
        assert ((held < 0) | (held // 6 == b)).all()


def test_what_the_host_statement_refuses():
    L = capi.lib()
    ip, fp, up = C.POINTER(C.c_int32), C.POINTER(C.c_float), C.POINTER(C.c_uint32)
    p, t, n, out = (C.c_int32 * 2)(0, 1), (C.c_float * 6)(), (C.c_uint32 * 1)(2), (C.c_int32 * 2)()
    assert L.tetsim_prep_pin_slots(p, t, 1, 2, n, out) == capi.OK
    assert L.tetsim_prep_pin_slots(p, t, 1, 0, n, out) == capi.EINVAL
    for args in ((ip(), t, 1, 2, n, out), (p, fp(), 1, 2, n, out), (p, t, 1, 2, up(), out), (p, t, 1, 2, n, ip())):
        assert L.tetsim_prep_pin_slots(*args) == capi.EINVAL
    assert L.tetsim_prep_pin_slots(p, t, 1 << 16, 1 << 15, n, out) == capi.EINVAL   # 2^31 rows
    with pytest.raises(ValueError):
        prep_pin_slots([[0, 1]], np.zeros((1, 3, 3), np.float32), [2])


def test_the_three_symbols_are_declared_and_exported():
    header = open(os.path.join(ROOT, "include", "tetsim.h")).read()
    L = capi.lib()
    for s in NEW:
        assert re.search(r"\bint %s\s*\(" % s, header), s
        assert s in capi.SYMBOLS and s in capi.OPTIONAL_SYMBOLS and hasattr(L, s), s
        assert getattr(L, s).restype == C.c_int, s
    assert L.tetsim_abi_version() == 5   # additive: the ABI version stays
    vp, u32, u64 = C.c_void_p, C.c_uint32, C.c_uint64
    assert L.tetsim_set_body_pins.argtypes == [vp, C.POINTER(C.c_int32), C.POINTER(C.c_float), u32]
    assert L.tetsim_set_body_pins_device.argtypes == [vp, vp, vp, u64, u32, vp, vp]
    assert L.tetsim_set_body_pins(None, None, None, 1) == capi.EINVAL
    assert L.tetsim_set_body_pins_device(None, None, None, 0, 1, None, None) == capi.EINVAL


def test_the_python_methods_exist():
    want = {"setBodyPins": ["self", "particles", "targets"], "setBodyPinsDevice": ["self", "particles", "targets", "bodies", "stream"]}
    for name, args in want.items():
        assert list(inspect.signature(getattr(SoftBodyHIP, name)).parameters) == args, name
    assert list(inspect.signature(prep_pin_slots).parameters) == ["particles", "targets", "body_particles"]
