"""Body colliders (include/tetsim.h: tetsim_set_body_colliders / _device), as far as a machine without a GPU can see them: declared,
exported, prototyped in the ctypes binding, wrapped by SoftBodyHIP; the row helper against its numpy restatement; the restated validity
rules against the cases tetsim_set_colliders is known to refuse."""
import ctypes as C
import inspect
import os
import re

import numpy as np
import pytest

import body_collider_ref as ref
from conftest import ROOT, load_mesh
from test_gpu_colliders import BAD, scene
from tetsim_amd import SoftBodyHIP, body_collider_rows
from tetsim_amd import _capi as capi

NEW = ("tetsim_set_body_colliders", "tetsim_set_body_colliders_device")


def _header():
    return open(os.path.join(ROOT, "include", "tetsim.h")).read()


def test_the_two_symbols_are_declared_and_exported():
    header = _header()
    L = capi.lib()
    for s in NEW:
        assert re.search(r"\bint %s\s*\(tetsim_handle h," % s, header), s
        assert s in capi.SYMBOLS and s in capi.OPTIONAL_SYMBOLS and hasattr(L, s), s
    assert re.search(r"#define TETSIM_BODY_COLLIDER_FLOATS 24\b", header) and capi.BODY_COLLIDER_FLOATS == 24 == ref.FLOATS
    assert L.tetsim_abi_version() == 5   # additive: the ABI version stays
    assert re.search(r"#define TETSIM_ABI_VERSION 5\b", header)


def test_the_ctypes_prototypes_match_the_header():
    L = capi.lib()
    vp, u64, u32 = C.c_void_p, C.c_uint64, C.c_uint32
    assert L.tetsim_set_body_colliders.argtypes == [vp, C.POINTER(C.c_float), u32]
    assert L.tetsim_set_body_colliders_device.argtypes == [vp, vp, u64, u32, vp, vp]
    for s in NEW:
        assert getattr(L, s).restype == C.c_int, s


def test_a_null_handle_is_refused_without_a_device():
    L = capi.lib()
    assert L.tetsim_set_body_colliders(None, None, 0) == capi.EINVAL
    assert L.tetsim_set_body_colliders_device(None, None, 0, 1, None, None) == capi.EINVAL


def test_the_python_methods_and_the_helper_exist():
    want = {"setBodyColliders": ["self", "lists_or_rows"], "setBodyCollidersDevice": ["self", "rows", "bodies", "stream"]}
    for name, args in want.items():
        assert list(inspect.signature(getattr(SoftBodyHIP, name)).parameters) == args, name
    sig = inspect.signature(body_collider_rows)
    assert list(sig.parameters) == ["lists", "per_body"] and sig.parameters["per_body"].default is None


def test_the_out_of_scope_lists_no_longer_name_what_exists():
    header = _header()
    assert "per-body colliders" not in header and "device-resident collider lists" not in header
    assert "per-body parameters" in header   # ... which stay out of scope


def _lists():
    v, _ = load_mesh("dragon")
    return [scene(v, 0), scene(v, 3)[1:3], [], [dict(kind="plane", a=[0.0, -0.5, 0.0], b=[0.0, 2.0, 0.0], friction=3.0)]]


@pytest.mark.parametrize("per_body", [None, 4, 8])
def test_the_row_helper_agrees_with_its_restatement(per_body):
    lists = _lists()
    got, want = body_collider_rows(lists, per_body), ref.rows(lists, per_body)
    assert got.dtype == np.float32 and got.shape == (4, per_body or 4, 24)
    assert np.array_equal(got.view(np.uint32), want.view(np.uint32))
    assert (got[2, :, 0] == -1.0).all() and (got[1, 2:, 0] == -1.0).all() and not got[:, :, 21:].any()
    for bad in (0, 9, 3):   # too few slots for the longest list, or outside 1 .. 8
        with pytest.raises(ValueError):
            body_collider_rows(lists, bad)
        with pytest.raises(ValueError):
            ref.rows(lists, bad)
    assert body_collider_rows([[], []]).shape == (2, 1, 24)


def test_row_ok_refuses_what_the_host_refuses_and_accepts_the_scene():
    """BAD of test_gpu_colliders.py: the lists tetsim_set_colliders refuses.  Two of them are refused before there is a row -- nine
    colliders do not fit a body's eight slots, and a row has no `reserved` field: rows() raises; every other one has a row row_ok refuses."""
    for what, cols in BAD:
        try:
            r = ref.rows([cols])
        except ValueError:
            assert what in ("too many", "reserved"), what
            with pytest.raises(ValueError):
                body_collider_rows([cols])
            continue
        assert what not in ("too many", "reserved")
        assert not all(ref.row_ok(x) for x in r[0]), what
    v, _ = load_mesh("dragon")
    for frame in (0, 5):
        cols = ref.f32_scene(v, frame)
        assert len(cols) == 4 and [c["kind"] for c in cols] == ["sphere", "capsule", "box", "plane"]
        r = ref.rows([cols], 8)
        assert [ref.row_ok(x) for x in r[0]] == [True] * 4 + [False] * 4
        again = ref.lists_from_rows(r)[0]   # f32 values survive the round trip unchanged
        assert np.array_equal(ref.rows([again], 8).view(np.uint32), r.view(np.uint32))
    assert not ref.row_ok(ref.rows([[]])[0, 0])   # an empty slot is not a collider
