"""Picking without a GPU: the written definition of the ray cast and the bounding sphere (tests/raycast_ref.py, the text of
include/tetsim.h in numpy) against fixtures recorded from three.js r160 itself (tests/golden/make_golden_raycast.sh), bit for
bit; and tetsim_prep_boundary_surface (host only) on lattices and on irregular meshes."""
import ctypes as C
import hashlib
import json
import os

import numpy as np
import pytest
from scipy.spatial import Delaunay

import raycast_ref
from conftest import GOLDEN, load_f32
from tetsim_amd import _capi as capi
from tetsim_amd import make_lattice


def load_raycast_golden():
    rays = np.fromfile(os.path.join(GOLDEN, "raycast_dragon_rays.f64"), dtype="<f8").reshape(-1, 8)
    h64 = np.fromfile(os.path.join(GOLDEN, "raycast_dragon_hits.f64"), dtype="<f8").reshape(-1, 4)
    h32 = np.fromfile(os.path.join(GOLDEN, "raycast_dragon_hits.i32"), dtype="<i4").reshape(-1, 2)
    sphere = np.fromfile(os.path.join(GOLDEN, "raycast_dragon_sphere.f64"), dtype="<f8")
    return rays, h32, h64, sphere


def dragon_visual():
    pos = load_f32("dragon_vispos_10.f32").reshape(-1, 3)
    tris = np.fromfile(os.path.join(GOLDEN, "dragon_vistris.u16"), dtype="<u2").astype(np.int32).reshape(-1, 3)
    return pos, tris


def bits(a):
    return np.ascontiguousarray(a, dtype=np.float64).view(np.int64)


def assert_hits_equal_golden(hits, h32, h64):
    """Every field of every ray, floating-point values as 64-bit integers."""
    assert np.array_equal(hits["hit"], h32[:, 0])
    assert np.array_equal(hits["triangle"], h32[:, 1])
    assert np.array_equal(bits(hits["distance"]), bits(h64[:, 0]))
    assert np.array_equal(bits(hits["point"]), bits(h64[:, 1:4]))


def test_fixture_files_are_the_recorded_ones():
    with open(os.path.join(GOLDEN, "golden_raycast.json")) as f:
        g = json.load(f)
    assert g["three"] == "160" and g["rays"] == 512
    for name, sha in g["sha256"].items():
        with open(os.path.join(GOLDEN, name), "rb") as f:
            assert hashlib.sha256(f.read()).hexdigest() == sha, name


def test_bounding_sphere_definition_equals_threejs():
    pos, _ = dragon_visual()
    _, _, _, sphere = load_raycast_golden()
    centre, radius = raycast_ref.bounding_sphere(pos)
    assert np.array_equal(bits(np.append(centre, radius)), bits(sphere))
    assert sphere.tolist() == [-0.01030576229095459, 1.2529106736183167, -0.03995586931705475, 1.1317856338816195]


def test_raycast_definition_equals_threejs_on_every_ray():
    pos, tris = dragon_visual()
    rays, h32, h64, _ = load_raycast_golden()
    assert len(pos) == 29800 and len(tris) == 59657 and len(rays) == 512
    hits = raycast_ref.raycast(pos, tris, rays[:, 0:3], rays[:, 3:6], rays[:, 6], rays[:, 7])
    assert_hits_equal_golden(hits, h32, h64)
    # the set must not pass vacuously
    nhit = int(h32[:, 0].sum())
    assert nhit >= len(rays) // 4 and len(rays) - nhit >= len(rays) // 4
    # winners that are ties decided by the triangle index: another triangle at exactly the winning distance
    P = pos.astype(np.float64)
    ties = 0
    for i in np.flatnonzero(h32[:, 0] == 1):
        masked = np.delete(np.arange(len(tris)), h32[i, 1])
        other = raycast_ref.raycast(P, tris[masked], rays[i, 0:3], rays[i, 3:6], rays[i, 6], rays[i, 7], sphere=raycast_ref.bounding_sphere(pos))
        if other["hit"][0] and bits(other["distance"])[0] == bits(h64[i, 0]):
            assert masked[other["triangle"][0]] > h32[i, 1]        # the recorded winner is the lowest index
            ties += 1
    assert ties >= 16, ties
    # windowed rays (the last 32): some hit something other than their unwindowed winner
    w = slice(480, 512)
    assert np.all(np.isfinite(rays[w, 7]) | (rays[w, 6] > 0))
    free = raycast_ref.raycast(pos, tris, rays[w, 0:3], rays[w, 3:6])
    assert int(((h32[w, 0] == 1) & (h32[w, 1] != free["triangle"])).sum()) >= 8
    assert int((h32[w, 0] == 0).sum()) >= 1 and np.all(free["hit"] == 1)


def test_direction_is_normalised_as_threejs_does():
    """Mesh.raycast takes the ray to local space through Vector3.transformDirection, which normalises: a direction of another
    length gives the same hit, and distances stay world lengths."""
    pos, tris = dragon_visual()
    rays, h32, h64, _ = load_raycast_golden()
    i = int(np.flatnonzero(h32[:96, 0] == 1)[0])
    a = raycast_ref.raycast(pos, tris, rays[i, 0:3], rays[i, 3:6] * 4.0)
    assert a["hit"][0] == 1 and a["triangle"][0] == h32[i, 1] and abs(a["distance"][0] - h64[i, 0]) < 1e-12


# ---- tetsim_prep_boundary_surface ---------------------------------------------------------------------------------------
fp = lambda a: a.ctypes.data_as(C.POINTER(C.c_float))  # noqa: E731
ip = lambda a: a.ctypes.data_as(C.POINTER(C.c_int32))  # noqa: E731


def surface(t, nv, v=None):
    L = capi.lib()
    tt = np.ascontiguousarray(t.reshape(-1), dtype=np.int32)
    vv = None if v is None else np.ascontiguousarray(v.reshape(-1), dtype=np.float32)
    nr, ntri = C.c_uint32(), C.c_uint32()
    assert L.tetsim_prep_boundary_surface(fp(vv) if v is not None else None, ip(tt), len(tt) // 4, nv, None, None, C.byref(nr), C.byref(ntri)) == 0
    vis, tri = np.full(4 * nr.value, -7, np.float32), np.full(3 * ntri.value, -7, np.int32)
    nr2, nt2 = C.c_uint32(), C.c_uint32()
    assert L.tetsim_prep_boundary_surface(fp(vv) if v is not None else None, ip(tt), len(tt) // 4, nv, fp(vis), ip(tri), C.byref(nr2), C.byref(nt2)) == 0
    assert (nr2.value, nt2.value) == (nr.value, ntri.value)      # the counts-only query agrees
    return vis.reshape(-1, 4), tri.reshape(-1, 3)


def check_surface(v, t, vis, tri):
    """Closed and consistently oriented, outward, rows well formed."""
    nv = len(v)
    # every row: a tet that contains the particle, one weight equal to 1 (the fourth is 1 - b0 - b1 - b2)
    tn = vis[:, 0].astype(np.int64)
    assert np.array_equal(tn.astype(np.float32), vis[:, 0]) and tn.min() >= 0 and tn.max() < len(t)
    w = np.concatenate([vis[:, 1:4], (np.float32(1) - vis[:, 1] - vis[:, 2] - vis[:, 3])[:, None]], axis=1)
    assert np.all((w == 0) | (w == 1)) and np.all(w.sum(axis=1) == 1)
    particle = t[tn, np.argmax(w, axis=1)]
    assert np.all(np.diff(particle) > 0)                          # rows ascend by particle id
    first_tet = np.full(nv, len(t), np.int64)
    np.minimum.at(first_tet, t.ravel(), np.repeat(np.arange(len(t)), 4))
    assert np.array_equal(tn, first_tet[particle])                # tetNr = the lowest tet containing it
    # every directed edge is met by its reverse exactly as often: closed, and consistently oriented
    P = particle[tri]
    e = np.concatenate([P[:, [0, 1]], P[:, [1, 2]], P[:, [2, 0]]])
    fwd = {}
    for a, b in e.tolist():
        fwd[(a, b)] = fwd.get((a, b), 0) + 1
    assert all(fwd.get((b, a), 0) == n for (a, b), n in fwd.items())
    # divergence theorem on the rest vertices: the surface encloses the tets' volume, and it is positive (outward)
    X = v.astype(np.float64)
    a, b, c = X[P[:, 0]], X[P[:, 1]], X[P[:, 2]]
    vol_surface = np.einsum("ij,ij->i", a, np.cross(b, c)).sum() / 6.0
    d = X[t[:, 1:]] - X[t[:, :1]]
    vol_tets = np.abs(np.linalg.det(d)).sum() / 6.0
    assert vol_surface > 0 and abs(vol_surface - vol_tets) <= 1e-12 * vol_tets
    return P


@pytest.mark.parametrize("n", [1, 4, 12])
def test_boundary_surface_of_a_lattice(n):
    v, t = make_lattice(n)
    vis, tri = surface(t, len(v), v)
    assert len(tri) == 12 * n * n and len(vis) == 6 * n * n + 2
    vis0, tri0 = surface(t, len(v), None)                         # make_lattice orients every tet positively
    assert np.array_equal(vis, vis0) and np.array_equal(tri, tri0)
    P = check_surface(v, t, vis, tri)
    und = np.sort(np.concatenate([P[:, [0, 1]], P[:, [1, 2]], P[:, [2, 0]]]), axis=1)
    _, counts = np.unique(und, axis=0, return_counts=True)
    assert np.all(counts == 2)                                    # every edge is shared by exactly two triangles
    again = surface(t, len(v), v)
    assert np.array_equal(vis, again[0]) and np.array_equal(tri, again[1])


@pytest.mark.parametrize("seed,npts", [(1, 60), (2, 400)])
def test_boundary_surface_of_a_delaunay_body(seed, npts):
    rng = np.random.default_rng(seed)
    pts = (rng.random((npts, 3)) * [0.8, 0.6, 0.7] + [-0.4, 0.15, -0.35]).astype(np.float32)
    tets = Delaunay(pts.astype(np.float64)).simplices.astype(np.int32)
    vol = np.linalg.det(pts[tets[:, 1:]].astype(np.float64) - pts[tets[:, :1]].astype(np.float64))
    tets = np.ascontiguousarray(tets[np.abs(vol) > 1e-9])
    vol = vol[np.abs(vol) > 1e-9]
    assert (vol < 0).any() and (vol > 0).any()                    # either handedness, as Delaunay leaves them: `verts` orients them
    vis, tri = surface(tets, npts, pts)
    check_surface(pts, tets, vis, tri)
    fixed = tets.copy()
    fixed[vol < 0] = fixed[vol < 0][:, [0, 1, 3, 2]]              # all positive: the answer without `verts` is a closed outward surface too
    vis2, tri2 = surface(fixed, npts, None)
    check_surface(pts, fixed, vis2, tri2)


def test_boundary_surface_keeps_the_convention_for_a_zero_volume_tet():
    """A flat tet with `verts` given is taken as positively oriented, like every tet without `verts`; a mirrored one is flipped."""
    v = np.array([[0, 0, 0], [1, 0, 0], [0, 1, 0], [1, 1, 0]], np.float32)           # four coplanar points: det == 0
    t = np.array([[0, 1, 2, 3]], np.int32)
    vis, tri = surface(t, 4, v)
    vis0, tri0 = surface(t, 4, None)
    assert np.array_equal(vis, vis0) and np.array_equal(tri, tri0)
    assert tri.tolist() == [[1, 2, 3], [0, 3, 2], [0, 1, 3], [0, 2, 1]]              # face k opposite corner k, (tet, face) order
    v[3] = [0, 0, -1]                                                                 # negative volume: every face turned over
    _, neg = surface(t, 4, v)
    assert neg.tolist() == [[1, 3, 2], [0, 2, 3], [0, 3, 1], [0, 1, 2]]
    check_surface(v, t[:, [0, 1, 3, 2]], *surface(t[:, [0, 1, 3, 2]], 4, v))


def test_boundary_surface_rejects_bad_input():
    L = capi.lib()
    v, t = make_lattice(2)
    tt = np.ascontiguousarray(t.reshape(-1), dtype=np.int32).copy()
    n = C.c_uint32()
    assert L.tetsim_prep_boundary_surface(None, ip(tt), len(tt) // 4, len(v), None, None, None, C.byref(n)) == capi.EINVAL
    assert L.tetsim_prep_boundary_surface(None, ip(tt), len(tt) // 4, 0, None, None, C.byref(n), C.byref(n)) == capi.EINVAL   # tets without particles
    tt[3] = 10 ** 6
    assert L.tetsim_prep_boundary_surface(None, ip(tt), len(tt) // 4, len(v), None, None, C.byref(n), C.byref(n)) == capi.EINVAL
    assert b"outside" in L.tetsim_last_error(None)
