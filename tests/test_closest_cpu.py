"""tetsim_closest_visual_device without a GPU: its per-triangle routine (tests/closest_ref.py) against three.js's own answers, a walk of
the library's tree topology (tetsim_prep_bvh) under the header's skip rules against the brute-force definition on an adversarial query set,
how much such a walk prunes, and the binding."""
import ctypes as C
import json
import os

import numpy as np
import pytest

import closest_ref as ref
import raycast_bvh_ref as bvh
from conftest import GOLDEN
from test_raycast_bvh_cpu import dragon_surface, prep_bvh
from tetsim_amd import CLOSEST_DTYPE, SoftBodyHIP, point_queries_tensor
from tetsim_amd import _capi as capi


def bits(a):
    return np.ascontiguousarray(a, dtype=np.float64).view(np.int64)


def same_bits(a, b):
    """bit for bit; a NaN equals a NaN (its sign and payload are no operation's result)"""
    a, b = np.ascontiguousarray(a, np.float64), np.ascontiguousarray(b, np.float64)
    return bool(np.all((bits(a) == bits(b)) | (np.isnan(a) & np.isnan(b))))


def records_differ(a, b):
    """[count] bool: some field of the two records differs, floats by their bits"""
    d = np.zeros(len(a), bool)
    for f in ("found", "body", "triangle", "region"):
        d |= a[f] != b[f]
    for f in ("distance", "v", "w"):
        d |= bits(a[f]) != bits(b[f])
    return d | (bits(a["point"]) != bits(b["point"])).any(axis=1)


def test_the_per_triangle_routine_equals_threejs_bit_for_bit():
    with open(os.path.join(GOLDEN, "closest_three.json")) as f:
        g = json.load(f)
    assert g["three"] == "160" and len(g["cases"]) >= 400
    unhex = lambda rows: np.array([[int(x, 16) for x in r] for r in rows], dtype=np.uint64).view(np.float64)   # noqa: E731
    t, p, q = unhex([c["t"] for c in g["cases"]]), unhex([c["p"] for c in g["cases"]]), unhex([c["q"] for c in g["cases"]])
    region = np.array([c["region"] for c in g["cases"]])
    assert np.array_equal(t, t.astype(np.float32).astype(np.float64))             # the corners are f32 values
    got_q, got_region, v, w = ref.closest_on_triangles(t[:, 0:3], t[:, 3:6], t[:, 6:9], p)
    assert same_bits(got_q, q)
    assert np.array_equal(got_region, region)
    assert np.all(np.bincount(region, minlength=7) >= 20) and set(region) == set(range(7))
    kinds = {c["kind"] for c in g["cases"]}
    assert kinds == {"random", "on_vertex", "on_edge", "in_plane", "degenerate", "near_1e3"}
    assert np.isnan(q).any() and np.abs(t).max() > 999.0                           # a zero-area triangle's 0 / 0 and the far coordinates are in it
    # (v, w) are the record's: q = a + v ab + w ac, to rounding, wherever q is a number
    ok = ~np.isnan(q).any(axis=1)
    a, ab, ac = t[ok, 0:3], t[ok, 3:6] - t[ok, 0:3], t[ok, 6:9] - t[ok, 0:3]
    err = np.abs(a + v[ok, None] * ab + w[ok, None] * ac - q[ok]).max(axis=1)
    assert np.all(err <= 8 * 2.0 ** -52 * (np.abs(t[ok]).max(axis=1) + np.abs(q[ok]).max(axis=1)))
    fixed = {ref.VERTEX_A: (0.0, 0.0), ref.VERTEX_B: (1.0, 0.0), ref.VERTEX_C: (0.0, 1.0)}
    for r, (fv, fw) in fixed.items():
        assert np.all(v[region == r] == fv) and np.all(w[region == r] == fw)
    assert np.all(w[region == ref.EDGE_AB] == 0.0) and np.all(v[region == ref.EDGE_AC] == 0.0)


MESHES = ("dragon", "cube")


@pytest.fixture(scope="module")
def walks():
    """per mesh: the adversarial queries, the brute-force definition and the walk of the library's tree, each computed once"""
    out = {}
    for mesh in MESHES:
        pos, tris = dragon_surface() if mesh == "dragon" else bvh.cube_surface(2)
        points, limit = ref.adversarial_queries(pos, tris)
        tri_first, order, node_first, depth, ranges = prep_bvh(pos, tris)
        brute_stats, walk_stats = {}, {}
        want = ref.closest(pos, tris, points, limit, stats=brute_stats)
        got = ref.traverse(pos, tris, order, ranges, int(depth[0]), points, limit, stats=walk_stats)
        out[mesh] = dict(pos=pos, tris=tris, points=points, limit=limit, want=want, got=got, brute=brute_stats, walk=walk_stats)
    return out


@pytest.mark.parametrize("mesh", MESHES)
def test_a_walk_of_the_tree_equals_the_definition(walks, mesh):
    """Vertices, edge midpoints, centroids, points 1e-9 off the surface and 1e4 away, the body's centre, points equidistant from two
    triangles across an edge, max_distance a hair below and above the truth: the walk equals brute force in every field, the box
    predicate removes nothing, and every query without a limit is found."""
    w = walks[mesh]
    n = ref.ADVERSARIAL_PER_KIND
    assert len(w["points"]) == len(ref.ADVERSARIAL_KINDS) * n
    print(mesh, w["brute"], w["walk"], int((w["want"]["found"] == 1).sum()))
    assert int(records_differ(w["got"], w["want"]).sum()) == 0
    assert w["brute"]["rejected"] == 0 and w["brute"]["within"] > 0
    assert np.all(w["want"]["found"][np.isinf(w["limit"])] == 1)
    kind = {k: slice(i * n, (i + 1) * n) for i, k in enumerate(ref.ADVERSARIAL_KINDS)}
    want = w["want"]
    assert np.all(want["found"][kind["max_below"]] == 0) and np.all(want["found"][kind["max_above"]] == 1)
    assert np.all(want["distance"][kind["vertex"]] == 0.0) and np.all(want["distance"][kind["edge_midpoint"]] <= 1e-7)
    assert np.all(np.abs(want["distance"][kind["off_surface_1e-9"]] - 1e-9) < 1e-10)
    assert np.all(want["distance"][kind["far_1e4"]] > 9e3)
    assert set(want["region"][want["found"] == 1].tolist()) == set(range(7))       # every region wins somewhere
    if mesh == "cube":                                                             # exact ties: the lowest index wins
        P, T, a, b, c = ref.corners(w["pos"], w["tris"])
        ties = 0
        for i in np.flatnonzero(want["found"] == 1):
            q, _, _, _ = ref.closest_on_triangles(a, b, c, w["points"][i])
            d2 = ref.dist2(w["points"][i], q)
            tied = np.flatnonzero(d2 == d2.min())
            ties += len(tied) > 1
            assert want["triangle"][i] == tied[0]
        assert ties >= 3 * n                                                       # vertices, edges and the points across an edge tie exactly


def test_the_walk_prunes(walks):
    """a condition on the reference walk itself, so that a tree that prunes nothing cannot pass: on the Dragon it tests fewer than a
    quarter of the triangles per query on average (observed: see the printed figure; far fewer)"""
    w = walks["dragon"]
    share = w["walk"]["triangles"] / (len(w["points"]) * len(w["tris"]))
    print("triangles tested per query: %.1f of %d (%.4f), boxes %.1f" % (w["walk"]["triangles"] / len(w["points"]), len(w["tris"]), share,
                                                                      w["walk"]["boxes"] / len(w["points"])))
    assert share < 0.25


def test_the_box_bound_is_monotone_in_the_box():
    """A box B that contains a box b has lb_B <= lb_b, for f32 boxes, flat ones included, points inside, outside and on a face: all a
    traversal needs to be allowed to skip a node."""
    rng = np.random.default_rng(23)
    n = 4000
    lo_b = rng.uniform(-2.0, 2.0, (n, 3)).astype(np.float32)
    hi_b = (lo_b + (rng.uniform(0.0, 1.0, (n, 3)) * (rng.random((n, 3)) > 0.25)).astype(np.float32)).astype(np.float32)
    lo_B = (lo_b - (rng.uniform(0.0, 1.0, (n, 3)) * (rng.random((n, 3)) > 0.25)).astype(np.float32)).astype(np.float32)
    hi_B = (hi_b + (rng.uniform(0.0, 1.0, (n, 3)) * (rng.random((n, 3)) > 0.25)).astype(np.float32)).astype(np.float32)
    lo_b, hi_b, lo_B, hi_B = (x.astype(np.float64) for x in (lo_b, hi_b, lo_B, hi_B))
    outside = 0
    for k in range(200):
        j = rng.integers(n)
        p = rng.uniform(-4.0, 4.0, 3) if k % 2 else lo_b[j] + rng.random(3) * (hi_b[j] - lo_b[j])
        if k % 5 == 0:
            p[k % 3] = lo_b[j, k % 3]
        e = ref.PAD * rng.uniform(0.0, 10.0)
        small, big = ref.box_bound(p, lo_b, hi_b, e), ref.box_bound(p, lo_B, hi_B, e)
        assert np.all(big <= small) and np.all(big >= 0.0)
        outside += int((small > 0).sum())
    assert outside > 100 * n


def test_the_symbols_are_declared_exported_and_bound():
    L = capi.lib()
    for s in ("tetsim_closest_visual_device", "tetsim_closest_visual"):
        assert s in capi.SYMBOLS and s in capi.OPTIONAL_SYMBOLS and hasattr(L, s), s
    assert L.tetsim_abi_version() == 5
    assert C.sizeof(capi.TetSimPointQuery) == 32 and C.sizeof(capi.TetSimClosest) == 64
    assert CLOSEST_DTYPE.itemsize == 64 and ref.CLOSEST_DTYPE == CLOSEST_DTYPE and capi.CLOSEST_INVALID == ref.CLOSEST_INVALID == -1
    assert [CLOSEST_DTYPE.fields[f][1] for f in ("found", "body", "triangle", "region", "distance", "point", "v", "w")] == [0, 4, 8, 12, 16, 24, 48, 56]
    assert len(L.tetsim_closest_visual_device.argtypes) == len(L.tetsim_raycast_visual_bvh_device.argtypes) == 8
    assert L.tetsim_closest_visual_device(None, None, 0, None, 0, None, 0, None) == capi.EINVAL
    assert L.tetsim_closest_visual(None, None, None, 0, None) == capi.EINVAL
    assert callable(SoftBodyHIP.closestPointsDevice) and callable(SoftBodyHIP.closestPoints) and callable(point_queries_tensor)
