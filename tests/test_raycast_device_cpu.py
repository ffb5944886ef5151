"""Range sensors without a GPU: the entry points exist and refuse a NULL handle, the binding's records have the header's sizes, the
per-body reference (tests/raycast_device_ref.py) equals raycast_ref on each body alone, every kind of invalid ray is named, and every
ray set of tests/test_gpu_raycast_device.py holds the hit-share condition on the rest-state surfaces -- so that no GPU test can pass on
all-miss (or all-hit) output."""
import ctypes as C

import numpy as np
import pytest

import raycast_device_ref as ref
import raycast_ref
from tetsim_amd import _capi as capi
from tetsim_amd import boundary_surface


def bits(a):
    return np.ascontiguousarray(a, dtype=np.float64).view(np.int64)


def test_symbols_are_exported_and_refuse_a_null_handle():
    L = capi.lib()
    assert hasattr(L, "tetsim_raycast_visual_device") and hasattr(L, "tetsim_visual_bounding_spheres_device")
    assert "tetsim_raycast_visual_device" in capi.OPTIONAL_SYMBOLS and "tetsim_visual_bounding_spheres_device" in capi.OPTIONAL_SYMBOLS
    assert L.tetsim_raycast_visual_device(None, None, 0, None, 0, None, 0, None) == capi.EINVAL
    assert L.tetsim_raycast_visual_device(None, None, 0, None, 4, None, 0, None) == capi.EINVAL
    assert L.tetsim_visual_bounding_spheres_device(None, None, 0, None) == capi.EINVAL
    assert capi.RAY_INVALID == -1 == ref.RAY_INVALID


def test_record_sizes():
    assert C.sizeof(capi.TetSimRay) == 64 and C.sizeof(capi.TetSimRayHit) == 48
    assert raycast_ref.HIT_DTYPE.itemsize == 48


def two_tets():
    """two disjoint unit tetrahedra (the second shifted by 3 in x) with their boundary surfaces, as one mesh of two bodies"""
    v1 = np.array([[0, 0, 0], [1, 0, 0], [0, 1, 0], [0, 0, 1]], np.float32)
    t1 = np.array([[0, 1, 2, 3]], np.int32)
    vis1, tri1 = boundary_surface(t1, 4, v1)
    assert len(tri1) == 4 and len(vis1) == 4
    pos1 = v1[t1[0][[int(np.argmax(np.append(r[1:4], 1 - r[1:4].sum()))) for r in vis1]]]
    pos2 = (pos1 + np.float32([3, 0, 0])).astype(np.float32)
    return pos1, pos2, tri1, np.concatenate([pos1, pos2]), np.concatenate([tri1, tri1 + 4]), np.repeat([0, 1], 4)


def test_reference_per_body_equals_each_body_alone():
    pos1, pos2, tri1, pos, tris, row_body = two_tets()
    rng = np.random.default_rng(1)
    o = rng.uniform(-2.0, 5.0, (200, 3))
    target = np.where(rng.random(200)[:, None] < 0.5, [0.25, 0.25, 0.25], [3.25, 0.25, 0.25]) + rng.normal(0, 0.3, (200, 3))
    d = target - o
    b = rng.integers(0, 2, 200).astype(np.int32)
    got = ref.raycast(pos, tris, row_body, 2, o, d, bodies=b)
    for k, solo_pos in enumerate((pos1, pos2)):
        sel = np.flatnonzero(b == k)
        want = raycast_ref.raycast(solo_pos, tri1, o[sel], d[sel])
        hit = want["hit"] == 1
        assert 10 <= int(hit.sum()) < len(sel)
        assert np.array_equal(got["hit"][sel], want["hit"])
        assert np.array_equal(got["triangle"][sel], np.where(hit, want["triangle"] + 4 * k, -1))
        assert np.array_equal(got["body"][sel], np.where(hit, k, -1))
        assert np.array_equal(bits(got["distance"][sel]), bits(want["distance"])) and np.array_equal(bits(got["point"][sel]), bits(want["point"]))
    # a ray through both bodies: the whole mesh names the nearer one, every body answers for itself
    o2, d2 = np.array([[-1.0, 0.2, 0.2]] * 2), np.array([[1.0, 0.0, 0.0]] * 2)
    whole = ref.raycast(pos, tris, row_body, 2, o2, d2)
    own = ref.raycast(pos, tris, row_body, 2, o2, d2, bodies=np.array([0, 1], np.int32))
    assert whole["body"].tolist() == [0, 0] and own["body"].tolist() == [0, 1] and own["distance"][1] == own["distance"][0] + 3.0
    sph = ref.bounding_spheres(pos, row_body, 3)
    assert np.array_equal(bits(sph[0]), bits(np.append(*raycast_ref.bounding_sphere(pos1))))
    assert np.array_equal(bits(sph[1]), bits(np.append(*raycast_ref.bounding_sphere(pos2)))) and not sph[2].any()


INVALID = {   # kind -> (origin, direction, near, far, body)
    "nan origin": ([np.nan, 0, 0], [0, 0, 1], 0.0, np.inf, 0),
    "inf origin": ([0, np.inf, 0], [0, 0, 1], 0.0, np.inf, 0),
    "nan direction": ([0, 0, 0], [0, np.nan, 1], 0.0, np.inf, 0),
    "inf direction": ([0, 0, 0], [0, 0, -np.inf], 0.0, np.inf, 0),
    "zero direction": ([0, 0, 0], [0, 0, 0], 0.0, np.inf, 0),
    "nan near": ([0, 0, 0], [0, 0, 1], np.nan, np.inf, 0),
    "nan far": ([0, 0, 0], [0, 0, 1], 0.0, np.nan, 0),
    "near < 0": ([0, 0, 0], [0, 0, 1], -1.0, np.inf, 0),
    "far < near": ([0, 0, 0], [0, 0, 1], 2.0, 1.0, 0),
    "body too large": ([0, 0, 0], [0, 0, 1], 0.0, np.inf, 2),
    "negative body": ([0, 0, 0], [0, 0, 1], 0.0, np.inf, -1),
}


@pytest.mark.parametrize("kind", list(INVALID))
def test_every_invalid_kind_maps_to_minus_one(kind):
    _, _, _, pos, tris, row_body = two_tets()
    o, d, near, far, body = INVALID[kind]
    good_o, good_d = [0.2, 0.2, 5.0], [0.0, 0.0, -1.0]
    got = ref.raycast(pos, tris, row_body, 2, [good_o, o, good_o], [good_d, d, good_d], [0.0, near, 0.0], [np.inf, far, np.inf],
                      bodies=np.array([0, body, 0], np.int32))
    assert got["hit"].tolist() == [1, -1, 1]
    bad = got[1]
    assert bad["body"] == -1 and bad["triangle"] == -1 and bad["distance"] == 0.0 and not bad["point"].any()
    assert ref.invalid_rays([o], [d], near, far, [body], 2).tolist() == [True]
    if "body" not in kind:                                                       # without bodies the body is not looked at
        assert ref.raycast(pos, tris, row_body, 2, [o], [d], near, far)["hit"].tolist() == [-1]
    assert ref.invalid_rays([good_o], [good_d], 0.0, np.inf, [1], 2).tolist() == [False]
    assert ref.invalid_rays([good_o], [good_d], 0.0, 0.0).tolist() == [False]    # far == near is a (degenerate) window, +inf is a far


# ---- the hit-share conditions of the GPU tests' ray sets ---------------------------------------------------------------------
def test_fixture_sizes():
    assert [len(ref.lattice_surface(n)[3]) for n in ref.LATTICES] == [48, 300, 1728]


def test_batch_ray_sets_hit_and_miss():
    """tests 1, 2, 3 (batch part) and 5: per body and as a whole; with bodies (each alone) and without (the overlapping whole)."""
    bodies = ref.batch_bodies()
    pos = np.concatenate([b[4] for b in bodies])
    row_body = np.concatenate([np.full(len(b[4]), k) for k, b in enumerate(bodies)])
    first = np.cumsum([0] + [len(b[4]) for b in bodies])
    tris = np.concatenate([b[3] + first[k] for k, b in enumerate(bodies)])
    for per_body in (None, {n: (ref.INVALID_RAYS[0] // 3, ref.INVALID_RAYS[1] + n) for n in ref.LATTICES}):
        o, d, b = ref.batch_rays(per_body)
        own = ref.raycast(pos, tris, row_body, 3, o, d, bodies=b)
        for k in range(3):
            assert ref.hit_share_ok(own["hit"][b == k]), (k, own["hit"][b == k].mean())
        assert ref.hit_share_ok(own["hit"])
        whole = ref.raycast(pos, tris, row_body, 3, o, d)
        assert ref.hit_share_ok(whole["hit"])
        assert len(np.unique(whole["body"][whole["hit"] == 1])) == 3             # the whole mesh names every body somewhere
        assert int((whole["body"] != own["body"]).sum()) >= len(o) // 50         # ... and often not the ray's own: the bodies overlap


def test_count_and_stream_ray_sets_hit_and_miss():
    """test 4 (every count from 63 on is a prefix of one set) and test 7"""
    _, _, _, tris, rest = ref.lattice_surface(2)
    o, d, at = ref.count_rays()
    assert len(o) == max(ref.COUNTS) == 70000
    base = np.unique(at, return_index=True)[1]                                   # one of every distinct ray
    hit = np.empty(len(o), np.int32)
    hit_base = raycast_ref.raycast(rest, tris, o[base], d[base])["hit"]
    hit[:] = hit_base[at]
    for count in ref.COUNTS:
        if count >= 63:
            assert ref.hit_share_ok(hit[:count]), count
    _, _, _, tris5, rest5 = ref.lattice_surface(5)
    o, d = ref.seeded_rays(rest5, *ref.STREAM_RAYS)
    assert ref.hit_share_ok(raycast_ref.raycast(rest5, tris5, o, d)["hit"])
