"""Picking on the device: tetsim_raycast_visual / tetsim_start_grab_ray / tetsim_read_visual_bounding_sphere against three.js
r160's own answers (fixtures of tests/golden/make_golden_raycast.sh) and against the numpy restatement of the definition
(tests/raycast_ref.py, itself pinned to three by tests/test_raycast_cpu.py) -- bit for bit in every field."""
import os

import numpy as np
import pytest

import raycast_ref
from conftest import GOLDEN, load_f32, load_mesh
from test_raycast_cpu import bits, load_raycast_golden
from tetsim_amd import SoftBodyHIP, TetSimError, boundary_surface, make_lattice
from tetsim_amd import _capi as capi

pytestmark = pytest.mark.gpu
PP = dict(gravity=-9.81, friction=1000.0, density=1000.0, devCompliance=1e-5, volCompliance=0.0,
          worldBounds=[-2.5, -1.0, -2.5, 2.5, 10.0, 2.5])
DT = (1.0 / 60.0) / 20


def dragon(solver="neohookean", precision="precise", **kw):
    v, t = load_mesh("dragon")
    vis = load_f32("dragon_vis.f32").reshape(-1, 4)
    tris = np.fromfile(os.path.join(GOLDEN, "dragon_vistris.u16"), dtype="<u2").astype(np.int32).reshape(-1, 3)
    return SoftBodyHIP(v, t, None, dict(PP), vis, tris, solver=solver, precision=precision, **kw), tris


def seeded_rays(pos, n, seed):
    """Both kinds of the fixtures: from a sphere of three radii aimed at a point inside the bounding sphere, and straight at a vertex."""
    rng = np.random.default_rng(seed)
    c, r = raycast_ref.bounding_sphere(pos)
    k = n // 2
    u = rng.standard_normal((k, 3))
    u /= np.linalg.norm(u, axis=1, keepdims=True)
    o = c + 3.0 * r * u
    w = rng.standard_normal((k, 3))
    w *= (rng.random(k) ** (1.0 / 3.0) / np.linalg.norm(w, axis=1))[:, None]
    d = (c + r * w) - o
    d /= np.linalg.norm(d, axis=1, keepdims=True)
    vtx = pos[rng.integers(0, len(pos), n - k)].astype(np.float64)
    o2 = vtx + [0.0, 0.0, 5.0]
    d2 = np.tile([0.0, 0.0, -1.0], (n - k, 1))
    return np.concatenate([o, o2]), np.concatenate([d, d2])


def assert_same_hits(got, ref, body=True):
    assert np.array_equal(got["hit"], ref["hit"])
    assert np.array_equal(got["triangle"], ref["triangle"])
    if body:
        assert np.array_equal(got["body"], ref["body"])
    assert np.array_equal(bits(got["distance"]), bits(ref["distance"]))
    assert np.array_equal(bits(got["point"]), bits(ref["point"]))


def assert_equals_ref(body, tris, origins, directions, near=0.0, far=np.inf):
    pos = body.visualPositions()
    got = body.raycastVisual(origins, directions, near, far)
    ref = raycast_ref.raycast(pos, tris, origins, directions, near, far)
    assert_same_hits(got, ref)
    c, r = body.visualBoundingSphere()
    rc, rr = raycast_ref.bounding_sphere(pos)
    assert np.array_equal(bits(np.append(c, r)), bits(np.append(rc, rr)))
    return got


def test_dragon_equals_the_threejs_fixtures_bit_for_bit():
    """1. Neo-Hookean PRECISE, 10 substeps (the visual positions are then dragon_vispos_10 bit for bit, test_gpu_skinning.py)."""
    body, _ = dragon()
    dt = (1.0 * (1.0 / 60.0)) / 10
    for _ in range(10):
        body.simulate(dt, PP)
    rays, h32, h64, sphere = load_raycast_golden()
    got = body.raycastVisual(rays[:, 0:3], rays[:, 3:6], rays[:, 6], rays[:, 7])
    assert np.array_equal(got["hit"], h32[:, 0])
    assert np.array_equal(got["triangle"], h32[:, 1])
    assert np.array_equal(bits(got["distance"]), bits(h64[:, 0]))
    assert np.array_equal(bits(got["point"]), bits(h64[:, 1:4]))
    assert np.array_equal(got["body"], np.where(h32[:, 0] == 1, 0, -1))
    c, r = body.visualBoundingSphere()
    assert np.array_equal(bits(np.append(c, r)), bits(sphere))


@pytest.mark.parametrize("kw", [dict(precision="fast"), dict(precision="fast", lean_state=True), dict(precision="precise")],
                         ids=["fast", "fast-lean", "precise"])
def test_deformed_polar_dragon_equals_the_restatement(kw):
    """2. 200 substeps with a sphere collider pushed into the body: a state no fixture covers; whichever solver made it."""
    body, tris = dragon("polar", **kw)
    body.setColliders([dict(kind="sphere", a=[0.1, -0.4, 0.0], radius=1.0, friction=100.0)])
    body.simulateSubsteps(200, DT, PP)
    pos = body.visualPositions()
    rest = load_f32("dragon_vispos_10.f32").reshape(-1, 3)
    assert np.isfinite(pos).all() and np.abs(pos - rest).max() > 0.05          # really deformed
    o, d = seeded_rays(pos, 1024, 11)
    got = assert_equals_ref(body, tris, o, d)
    assert 256 <= int(got["hit"].sum()) <= 1000


@pytest.mark.parametrize("n", [12, 55])
def test_lattice_through_boundary_surface(n):
    """3. A body without an artist's mesh: its boundary as the visual mesh; a ray straight down hits the top face."""
    v, t = make_lattice(n)
    vis, tris = boundary_surface(t, len(v), v)
    body = SoftBodyHIP(v, t, None, dict(PP), vis, tris, solver="polar", precision="fast")
    pos = body.visualPositions()
    top = float(v[:, 1].max())
    cx, cz = float(v[:, 0].mean()) + 0.0123, float(v[:, 2].mean()) - 0.0071
    hit = body.raycastVisual([[cx, top + 2.0, cz]], [[0.0, -1.0, 0.0]])[0]
    assert hit["hit"] == 1 and abs(hit["distance"] - 2.0) <= 1e-12 * 2.0
    assert np.all(pos[tris[hit["triangle"]]][:, 1] == np.float32(top))        # a triangle of the top face
    o, d = seeded_rays(pos, 256, n)
    assert_equals_ref(body, tris, o, d)
    body.simulateSubsteps(40, DT, PP)
    assert_equals_ref(body, tris, o, d)


def test_batch_of_three_dragons_names_the_body():
    """4. Every ray's body is right; distance / point / triangle (minus the body's triangle offset) equal the solo answer."""
    v, t = load_mesh("dragon")
    vis = load_f32("dragon_vis.f32").reshape(-1, 4)
    tris = np.fromfile(os.path.join(GOLDEN, "dragon_vistris.u16"), dtype="<u2").astype(np.int32).reshape(-1, 3)
    # translations that f32 positions carry exactly enough for a solo twin at the same place: the solo bodies are translated too
    shifts = [np.array([-3.0, 0.0, 0.0], np.float32), np.array([0.0, 0.0, 0.0], np.float32), np.array([3.0, 0.0, 0.5], np.float32)]
    wide = dict(PP, worldBounds=[-10.0, -1.0, -10.0, 10.0, 10.0, 10.0])
    bodies = [((v + s).astype(np.float32), t) for s in shifts]
    allvis = np.concatenate([vis + np.array([b * len(t), 0, 0, 0], np.float32) for b in range(3)])
    alltris = np.concatenate([tris + b * len(vis) for b in range(3)])
    batch = SoftBodyHIP.batch(bodies, dict(wide), solver="polar", precision="precise", ref_fixed_bounds=False)
    batch.setVisualMesh(allvis)
    batch.setVisualTriangles(alltris)
    batch.simulateSubsteps(5, DT, wide)
    for b in range(3):
        solo = SoftBodyHIP(bodies[b][0], t, None, dict(wide), vis, tris, solver="polar", precision="precise", ref_fixed_bounds=False)
        solo.simulateSubsteps(5, DT, wide)
        pos = solo.visualPositions()
        assert np.array_equal(pos.view(np.uint32), batch.visualPositions()[b * len(vis):(b + 1) * len(vis)].view(np.uint32))
        # rays at vertices of this body, from above (+y): nothing of another body lies on them
        rng = np.random.default_rng(b)
        vtx = pos[rng.integers(0, len(pos), 64)].astype(np.float64)
        o, d = vtx + [0.0, 4.0, 0.0], np.tile([0.0, -1.0, 0.0], (64, 1))
        want = solo.raycastVisual(o, d)
        got = batch.raycastVisual(o, d)
        assert want["hit"].sum() >= 48
        assert np.array_equal(got["hit"], want["hit"])
        assert np.array_equal(got["body"], np.where(want["hit"] == 1, b, -1))
        assert np.array_equal(got["triangle"], np.where(want["hit"] == 1, want["triangle"] + b * len(tris), -1))
        assert np.array_equal(bits(got["distance"]), bits(want["distance"])) and np.array_equal(bits(got["point"]), bits(want["point"]))


def test_seventy_thousand_rays_in_one_call():
    """5. Beyond gridDim.y: one call equals the same rays in calls of 1,000."""
    body, tris = dragon()
    pos = body.visualPositions()
    o, d = seeded_rays(pos, 70000, 5)
    perm = np.random.default_rng(6).permutation(70000)
    o, d = o[perm], d[perm]
    one = body.raycastVisual(o, d)
    parts = np.concatenate([body.raycastVisual(o[i:i + 1000], d[i:i + 1000]) for i in range(0, 70000, 1000)])
    assert_same_hits(one, parts)
    assert 17500 <= int(one["hit"].sum()) <= 65000
    ref = raycast_ref.raycast(pos, tris, o[:128], d[:128])
    assert_same_hits(one[:128], ref)
    single = body.raycastVisual(o[:1], d[:1])                                 # (one ray: many blocks per ray)
    assert_same_hits(single, one[:1])


def test_start_grab_ray():
    """6. The grabbed id equals startGrab(f32(hit point)) on a twin; after a miss the body steps as one that never asked."""
    a, _ = dragon("polar", "fast")
    b, _ = dragon("polar", "fast")
    c, _ = dragon("polar", "fast")
    for x in (a, b, c):
        x.simulateSubsteps(20, DT, PP)
    pos = a.visualPositions()
    o = pos[12345].astype(np.float64) + [0.0, 0.0, 5.0]
    d = np.array([0.0, 0.0, -1.0])
    gid, hit = a.startGrabRay(o, d)
    assert hit["hit"] == 1 and gid >= 0
    want = b.raycastVisual([o], [d])[0]
    assert bits(hit["distance"]) == bits(want["distance"]) and hit["triangle"] == want["triangle"]
    point = (o + d * want["distance"]).astype(np.float32)
    assert b.startGrab(point) == gid
    a.simulateSubsteps(10, DT, PP)
    b.simulateSubsteps(10, DT, PP)
    assert np.array_equal(a.pos.view(np.uint32), b.pos.view(np.uint32))
    gid, hit = c.startGrabRay([0.0, 50.0, 0.0], [0.0, 1.0, 0.0])              # points away: a miss
    assert gid == -1 and hit["hit"] == 0 and c.grabId == -1
    c.simulateSubsteps(10, DT, PP)
    never, _ = dragon("polar", "fast")
    never.simulateSubsteps(20, DT, PP)
    never.simulateSubsteps(10, DT, PP)
    assert np.array_equal(c.pos.view(np.uint32), never.pos.view(np.uint32))
    # a grab in force survives a miss
    a.startGrabRay([0.0, 50.0, 0.0], [0.0, 1.0, 0.0])
    a.simulateSubsteps(5, DT, PP)
    b.simulateSubsteps(5, DT, PP)
    assert np.array_equal(a.pos.view(np.uint32), b.pos.view(np.uint32))


def test_errors():
    """7. Every TETSIM_EINVAL / TETSIM_ESTATE case, with its message; a failed call leaves the next good one correct."""
    body, tris = dragon()
    L = capi.lib()
    o, d = np.array([[0.0, 1.2, 5.0]]), np.array([[0.0, 0.0, -1.0]])
    good = body.raycastVisual(o, d)
    assert good["hit"][0] == 1

    def bad(code, text, *a, **k):
        with pytest.raises(TetSimError) as e:
            body.raycastVisual(*a, **k)
        assert e.value.code == code and text in str(e.value), str(e.value)
        assert_same_hits(body.raycastVisual(o, d), good)

    bad(capi.EINVAL, "non-finite", [[np.nan, 0, 0]], d)
    bad(capi.EINVAL, "non-finite", o, [[0, np.inf, 0]])
    bad(capi.EINVAL, "zero direction", o, [[0.0, 0.0, 0.0]])
    bad(capi.EINVAL, "near < 0", o, d, -1.0)
    bad(capi.EINVAL, "far < near", o, d, 2.0, 1.0)
    bad(capi.EINVAL, "NaN", o, d, np.nan)
    bad(capi.EINVAL, "NaN", o, d, 0.0, np.nan)
    bad(capi.EINVAL, "ray 1:", np.concatenate([o, o]), np.concatenate([d, [[0.0, 0.0, 0.0]]]))
    assert L.tetsim_raycast_visual(body._h, None, 1, None) == capi.EINVAL and b"null" in L.tetsim_last_error(body._h)
    assert L.tetsim_raycast_visual(body._h, None, 0, None) == capi.OK          # count == 0 succeeds
    assert len(body.raycastVisual(np.zeros((0, 3)), np.zeros((0, 3)))) == 0
    assert L.tetsim_start_grab_ray(body._h, None, None, None) == capi.EINVAL
    assert L.tetsim_read_visual_bounding_sphere(body._h, None, None) == capi.EINVAL
    with pytest.raises(TetSimError) as e:
        body.startGrabRay([0.0, 1.2, 5.0], [0.0, 0.0, 0.0])
    assert e.value.code == capi.EINVAL and body.grabId == -1
    assert_same_hits(body.raycastVisual(o, d), good)

    v, t = load_mesh("dragon")
    vis = load_f32("dragon_vis.f32").reshape(-1, 4)
    bare = SoftBodyHIP(v, t, None, dict(PP), solver="neohookean")
    for call in (lambda: bare.raycastVisual(o, d), lambda: bare.visualBoundingSphere(), lambda: bare.startGrabRay(o[0], d[0])):
        with pytest.raises(TetSimError) as e:
            call()
        assert e.value.code == capi.ESTATE and "no visual mesh" in str(e.value)
    notris = SoftBodyHIP(v, t, None, dict(PP), vis, solver="neohookean")
    with pytest.raises(TetSimError) as e:
        notris.raycastVisual(o, d)
    assert e.value.code == capi.ESTATE and "no visual triangles" in str(e.value)
    c, r = notris.visualBoundingSphere()                                        # the sphere needs no triangles
    assert r > 0
    part = SoftBodyHIP(v, t, None, dict(PP), vis, solver="polar", precision="fast", part_count=2, part_index=1)
    part.setVisualTriangles(tris)
    for call in (lambda: part.raycastVisual(o, d), lambda: part.visualBoundingSphere(), lambda: part.startGrabRay(o[0], d[0])):
        with pytest.raises(TetSimError) as e:
            call()
        assert e.value.code == capi.ESTATE and "partition" in str(e.value)


def test_a_ray_cast_between_calls_changes_nothing():
    """8. A read: the trajectory equals a twin's that never asked; device_bytes grows only once a query has run."""
    for solver, precision in (("polar", "fast"), ("neohookean", "precise")):
        a, _ = dragon(solver, precision)
        b, _ = dragon(solver, precision)
        a.simulateSubsteps(20, DT, PP)
        b.simulateSubsteps(20, DT, PP)
        pos = a.visualPositions()
        o, d = seeded_rays(pos, 64, 3)
        a.raycastVisual(o, d)
        a.visualBoundingSphere()
        a.simulateSubsteps(20, DT, PP)
        b.simulateSubsteps(20, DT, PP)
        assert np.array_equal(a.pos.view(np.uint32), b.pos.view(np.uint32))
        assert np.array_equal(a.vel.view(np.uint32), b.vel.view(np.uint32))
        ia, ib = capi.TetSimInfo(), capi.TetSimInfo()
        a._L.tetsim_get_info(a._h, ia)
        b._L.tetsim_get_info(b._h, ib)
        assert ia.device_bytes > ib.device_bytes       # the query's buffers are counted once they exist, and only then
