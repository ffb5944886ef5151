"""tetsim_raycast_visual_bvh_device without a GPU: its definition (tests/raycast_bvh_ref.py) against three.js's own answers and against
tests/raycast_ref.py on an adversarial ray set, the monotonicity every conservative tree rests on, the binding, and the topology the
library builds (tetsim_prep_bvh)."""
import ctypes as C
import os

import numpy as np
import pytest

import raycast_bvh_ref as bvh
import raycast_ref
from conftest import GOLDEN, load_f32
from test_raycast_cpu import load_raycast_golden
from tetsim_amd import SoftBodyHIP
from tetsim_amd import _capi as capi


def bits(a):
    return np.ascontiguousarray(a, dtype=np.float64).view(np.int64)


def dragon_surface():
    pos = load_f32("dragon_vispos_10.f32").reshape(-1, 3)
    tris = np.fromfile(os.path.join(GOLDEN, "dragon_vistris.u16"), dtype="<u2").astype(np.int32).reshape(-1, 3)
    return pos, tris


def records_differ(a, b):
    """[count] bool: some field of the two records differs, floats by their bits"""
    return ((a["hit"] != b["hit"]) | (a["body"] != b["body"]) | (a["triangle"] != b["triangle"]) | (bits(a["distance"]) != bits(b["distance"])) |
            (bits(a["point"]) != bits(b["point"])).any(axis=1))


def test_the_definition_equals_the_threejs_fixtures_on_the_dragon():
    pos, tris = dragon_surface()
    rays, h32, h64, _ = load_raycast_golden()
    stats = {}
    got = bvh.raycast(pos, tris, rays[:, 0:3], rays[:, 3:6], rays[:, 6], rays[:, 7], stats=stats)
    assert np.array_equal(got["hit"], h32[:, 0]) and np.array_equal(got["triangle"], h32[:, 1])
    assert np.array_equal(bits(got["distance"]), bits(h64[:, 0])) and np.array_equal(bits(got["point"]), bits(h64[:, 1:4]))
    assert stats["accepted"] >= 512 and stats["removed"] == 0


# what the seeded set produces: (accepted hits, rays with a hit) -- an empty set cannot pass
ADVERSARIAL_HITS = {"dragon": (524, 263), "cube": (304, 236)}


@pytest.mark.parametrize("mesh", ["dragon", "cube"])
def test_the_definition_equals_raycast_ref_on_the_adversarial_set(mesh):
    """Vertices, edge midpoints, centroids, grazing rays at a tilt of 1e-9, origins 1e4 away, axis-aligned directions with exact zeros, an
    origin inside the body, near behind the first surface: the two extra predicates remove no accepted hit and change no record."""
    pos, tris = dragon_surface() if mesh == "dragon" else bvh.cube_surface()
    o, d, near, far = bvh.adversarial_rays(pos, tris)
    assert len(o) == 8 * bvh.ADVERSARIAL_PER_KIND
    assert (d == 0.0).sum() >= 2 * bvh.ADVERSARIAL_PER_KIND and (near > 0.0).sum() >= bvh.ADVERSARIAL_PER_KIND // 4
    stats = {}
    got, want = bvh.raycast(pos, tris, o, d, near, far, stats=stats), raycast_ref.raycast(pos, tris, o, d, near, far)
    print(mesh, stats, int((got["hit"] == 1).sum()))
    assert int(records_differ(got, want).sum()) == 0
    assert stats["removed"] == 0
    assert (stats["accepted"], int((got["hit"] == 1).sum())) == ADVERSARIAL_HITS[mesh]
    if mesh == "dragon":                                                          # ... and the second surface did win where there is one
        last = slice(7 * bvh.ADVERSARIAL_PER_KIND, None)
        first = raycast_ref.raycast(pos, tris, o[last], d[last])
        behind = got["hit"][last] == 1
        assert behind.sum() >= 10 and np.all(got["distance"][last][behind] > first["distance"][behind])


def test_the_slab_interval_is_monotone_in_the_box():
    """A box B that contains a box b: tn_B <= tn_b, tf_B >= tf_b, and B's axis tests pass where b's do -- for f32 boxes, flat ones included,
    and rays whose direction has zero, denormal and tiny components.  This is all a traversal needs to be allowed to skip a node."""
    rng = np.random.default_rng(17)
    n = 4000
    lo_b = rng.uniform(-2.0, 2.0, (n, 3)).astype(np.float32)
    hi_b = (lo_b + (rng.uniform(0.0, 1.0, (n, 3)) * (rng.random((n, 3)) > 0.25)).astype(np.float32)).astype(np.float32)   # a quarter flat
    lo_B = (lo_b - (rng.uniform(0.0, 1.0, (n, 3)) * (rng.random((n, 3)) > 0.25)).astype(np.float32)).astype(np.float32)
    hi_B = (hi_b + (rng.uniform(0.0, 1.0, (n, 3)) * (rng.random((n, 3)) > 0.25)).astype(np.float32)).astype(np.float32)
    assert np.all(lo_B <= lo_b) and np.all(hi_b <= hi_B) and np.all(lo_b <= hi_b)
    lo_b, hi_b, lo_B, hi_B = (x.astype(np.float64) for x in (lo_b, hi_b, lo_B, hi_B))
    special = np.array([0.0, -0.0, 5e-324, -5e-324, 1e-310, 1e-300, -1e-300, 1e-160])
    checked = passed = 0
    for _ in range(200):
        j = rng.integers(n)                                                        # aimed at a point of box j ...
        at = lo_b[j] + rng.random(3) * (hi_b[j] - lo_b[j])
        o = rng.uniform(-4.0, 4.0, 3)
        d = at - o
        for k in range(3):
            if rng.random() < 0.4:                                                 # ... along an axis with no or next to no direction from inside its range
                d[k] = rng.choice(special)
                o[k] = at[k] if rng.random() < 0.7 else lo_b[j, k]                 # (or exactly on its face)
        if not d.any():
            d[0] = 1.0
        e = bvh.PAD * rng.uniform(0.0, 10.0)
        ok_b, tn_b, tf_b = bvh.slab(o, d, lo_b, hi_b, e)
        ok_B, tn_B, tf_B = bvh.slab(o, d, lo_B, hi_B, e)
        assert not np.isnan(tn_b).any() and not np.isnan(tf_b).any() and not np.isnan(tn_B).any() and not np.isnan(tf_B).any()
        assert np.all(tn_B <= tn_b) and np.all(tf_B >= tf_b)
        assert np.all(ok_B[ok_b])
        assert np.all((ok_B & (tn_B <= tf_B))[ok_b & (tn_b <= tf_b)])             # a candidate's node passes
        checked += n
        passed += int((ok_b & (tn_b <= tf_b)).sum())
    assert passed >= 10 * 200                                                      # (ten candidates a ray: the boxes are hit often enough to mean something)


def test_the_symbols_are_declared_exported_and_bound():
    L = capi.lib()
    for s in ("tetsim_raycast_visual_bvh_device", "tetsim_prep_bvh"):
        assert s in capi.SYMBOLS and s in capi.OPTIONAL_SYMBOLS and hasattr(L, s), s
    assert L.tetsim_abi_version() == 5
    assert len(L.tetsim_raycast_visual_bvh_device.argtypes) == len(L.tetsim_raycast_visual_device.argtypes) == 8
    assert L.tetsim_raycast_visual_bvh_device(None, None, 0, None, 0, None, 0, None) == capi.EINVAL
    assert L.tetsim_raycast_visual_bvh_device(None, None, 0, None, 4, None, 0, None) == capi.EINVAL
    assert callable(SoftBodyHIP.raycastVisualBvhDevice)


def prep_bvh(pos, tris, tri_body=None, bodies=1):
    L = capi.lib()
    up, u32 = C.POINTER(C.c_uint32), np.uint32
    pos, tris = np.ascontiguousarray(pos, np.float32), np.ascontiguousarray(tris, np.int32)
    tb = None if tri_body is None else np.ascontiguousarray(tri_body, np.int32)
    tri_first, order, node_first, depth = np.zeros(bodies + 1, u32), np.zeros(max(len(tris), 1), u32), np.zeros(bodies + 1, u32), np.zeros(bodies, u32)

    def call(node_range):
        return L.tetsim_prep_bvh(pos.ctypes.data_as(C.POINTER(C.c_float)), len(pos), tris.ctypes.data_as(C.POINTER(C.c_int32)), len(tris),
                                 None if tb is None else tb.ctypes.data_as(C.POINTER(C.c_int32)), bodies, tri_first.ctypes.data_as(up),
                                 order.ctypes.data_as(up), node_first.ctypes.data_as(up), depth.ctypes.data_as(up),
                                 None if node_range is None else node_range.ctypes.data_as(up))

    assert call(None) == capi.OK
    ranges = np.full((int(node_first[-1]), 2), 0xFFFFFFFF, u32)
    assert call(ranges) == capi.OK
    return tri_first, order[:len(tris)], node_first, depth, ranges


LEAF = 4


def check_topology(ntri, tri_body, bodies, tri_first, order, node_first, depth, ranges):
    body_of = np.zeros(ntri, np.int64) if tri_body is None else np.asarray(tri_body, np.int64)
    assert sorted(order.tolist()) == list(range(ntri))                            # every triangle once ...
    assert tri_first[0] == 0 and tri_first[-1] == ntri and node_first[0] == 0
    for b in range(bodies):
        lo, hi = int(tri_first[b]), int(tri_first[b + 1])
        n = hi - lo
        assert sorted(order[lo:hi].tolist()) == np.flatnonzero(body_of == b).tolist()   # ... in its own body's range
        leaves = (n + LEAF - 1) // LEAF
        d = int(depth[b])
        assert (1 << d) >= max(leaves, 1) and (d == 0 or (1 << (d - 1)) < leaves)
        assert int(node_first[b + 1]) - int(node_first[b]) == 2 << d and int(node_first[b]) % 2 == 0
        r = ranges[int(node_first[b]):int(node_first[b + 1])].astype(np.int64)
        assert tuple(r[0]) == (0, 0) and tuple(r[1]) == (lo, hi)                  # the root holds the body
        seen = []
        for i in range(1, 2 << d):
            assert lo <= r[i, 0] <= r[i, 1] <= hi
            if i < (1 << d):                                                       # an inner node: its children split its range, in order
                assert r[2 * i, 0] == r[i, 0] and r[2 * i, 1] == r[2 * i + 1, 0] and r[2 * i + 1, 1] == r[i, 1]
            else:                                                                  # a leaf: the next LEAF triangles, fewer at the end, none in the padding
                k = i - (1 << d)
                assert (r[i, 0], r[i, 1]) == (min(lo + LEAF * k, hi), min(lo + LEAF * k + LEAF, hi))
                seen += list(range(r[i, 0], r[i, 1]))
        assert seen == list(range(lo, hi))                                         # every triangle of the body in exactly one leaf


@pytest.mark.parametrize("ntri", [0, 1, 3, 4, 5, 16, 17, 48, 1025, 4 * 256 + 1])
def test_the_topology_of_one_body(ntri):
    """counts around the leaf size, around powers of two, and around the 256 leaves a workgroup of the refit folds"""
    rng = np.random.default_rng(ntri)
    pos = rng.standard_normal((3 * max(ntri, 1), 3)).astype(np.float32)
    tris = rng.permutation(3 * ntri).reshape(-1, 3).astype(np.int32)
    out = prep_bvh(pos, tris)
    check_topology(ntri, None, 1, *out)


def test_the_topology_of_a_batch_and_the_morton_order():
    """bodies with 0, 1, 48 and 59,657 triangles behind one list, the triangles of the bodies interleaved; inside a body the order follows
    the Morton curve: leaves are compact -- on the Dragon a leaf's box is a small fraction of the body's"""
    pos, tris = dragon_surface()
    cpos, ctris = bvh.cube_surface()
    one = np.array([[0, 1, 2]], np.int32)
    all_pos = np.concatenate([pos, cpos, cpos[:3]])
    all_tris = np.concatenate([tris, ctris + len(pos), one + len(pos) + len(cpos)])
    tri_body = np.concatenate([np.full(len(tris), 3), np.full(len(ctris), 1), [2]]).astype(np.int32)
    perm = np.random.default_rng(4).permutation(len(all_tris))
    all_tris, tri_body = all_tris[perm], tri_body[perm]
    tri_first, order, node_first, depth, ranges = prep_bvh(all_pos, all_tris, tri_body, 4)
    check_topology(len(all_tris), tri_body, 4, tri_first, order, node_first, depth, ranges)
    assert list(np.diff(tri_first)) == [0, 48, 1, 59657] and list(depth) == [0, 4, 0, 14]
    lo, hi = int(tri_first[3]), int(tri_first[4])
    corners = all_pos[all_tris[order[lo:hi]]].astype(np.float64)                   # [n, 3 corners, xyz] in leaf order
    full = (hi - lo) // LEAF * LEAF
    leaf = corners[:full].reshape(-1, 3 * LEAF, 3)
    diag = np.linalg.norm(leaf.max(axis=1) - leaf.min(axis=1), axis=1)
    body_diag = np.linalg.norm(corners.reshape(-1, 3).max(axis=0) - corners.reshape(-1, 3).min(axis=0))
    assert np.median(diag) < 0.05 * body_diag
    # deterministic: the same input gives the same order
    assert np.array_equal(order, prep_bvh(all_pos, all_tris, tri_body, 4)[1])


def test_prep_refuses_bad_arguments():
    pos, tris = bvh.cube_surface()
    L = capi.lib()
    up = C.POINTER(C.c_uint32)
    a = [np.zeros(64, np.uint32) for _ in range(4)]
    args = [x.ctypes.data_as(up) for x in a]
    fp, ip = C.POINTER(C.c_float), C.POINTER(C.c_int32)
    bad = tris.copy()
    bad[5, 1] = len(pos)
    assert L.tetsim_prep_bvh(pos.ctypes.data_as(fp), len(pos), bad.ctypes.data_as(ip), len(bad), None, 1, *args, None) == capi.EINVAL
    assert L.tetsim_prep_bvh(pos.ctypes.data_as(fp), len(pos), tris.ctypes.data_as(ip), len(tris), None, 0, *args, None) == capi.EINVAL
    assert L.tetsim_prep_bvh(None, len(pos), tris.ctypes.data_as(ip), len(tris), None, 1, *args, None) == capi.EINVAL
    body = np.full(len(tris), 2, np.int32)
    assert L.tetsim_prep_bvh(pos.ctypes.data_as(fp), len(pos), tris.ctypes.data_as(ip), len(tris), body.ctypes.data_as(ip), 2, *args, None) == capi.EINVAL
