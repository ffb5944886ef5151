"""Range sensors on the device (include/tetsim.h: tetsim_raycast_visual_device / tetsim_visual_bounding_spheres_device;
SoftBodyHIP.raycastVisualDevice / visualBoundingSpheresDevice): every field of every record bit for bit against the body ALONE (its
host raycastVisual), against the batch's own host call (bodies=None) and against the numpy restatement (tests/raycast_device_ref.py).
The ray sets come from raycast_device_ref, where tests/test_raycast_device_cpu.py holds them to the hit-share condition."""
import ctypes as C
import os

import numpy as np
import pytest
import torch

import raycast_device_ref as ref
from conftest import GOLDEN, load_f32, load_mesh
from test_gpu_snapshot import _hip_runtime, device_bytes
from test_raycast_cpu import load_raycast_golden
from tetsim_amd import RAY_HIT_DTYPE, SoftBodyHIP, TetSimError, rays_tensor
from tetsim_amd import _capi as capi

pytestmark = pytest.mark.gpu
PP = dict(gravity=-9.81, friction=1000.0, density=1000.0, devCompliance=1e-5, volCompliance=0.0,
          worldBounds=[-2.5, -1.0, -2.5, 2.5, 10.0, 2.5])
DT = (1.0 / 60.0) / 20
KW = dict(solver="polar", precision="fast", ref_fixed_bounds=False)
COLLIDER = [dict(kind="sphere", a=[0.05, 0.35, 0.0], radius=0.3, friction=100.0)]   # pushed into the bottoms of all three lattices
SENTINEL = 0xA5


def bits(a):
    return np.ascontiguousarray(a, dtype=np.float64).view(np.int64)


def records(raw):
    """the packed TetSimRayHit records of a [count, 48] uint8 tensor, on the host"""
    return np.frombuffer(raw.contiguous().cpu().numpy().tobytes(), dtype=RAY_HIT_DTYPE)


def dev_i32(a):
    return torch.from_numpy(np.ascontiguousarray(a, dtype=np.int32)).cuda()


def cast(body, o, d, near=0.0, far=np.inf, bodies=None, **kw):
    res = body.raycastVisualDevice(rays_tensor(o, d, near, far), None if bodies is None else dev_i32(bodies), **kw)
    torch.cuda.synchronize()
    return records(res["raw"])


def assert_same(got, want, what=""):
    for f in ("hit", "body", "triangle", "reserved"):
        assert np.array_equal(got[f], want[f]), (what, f, np.flatnonzero(got[f] != want[f])[:8])
    assert np.array_equal(bits(got["distance"]), bits(want["distance"])), what
    assert np.array_equal(bits(got["point"]), bits(want["point"])), what


def make_batch(substeps):
    parts = ref.batch_bodies()
    batch = SoftBodyHIP.batch([(v, t) for v, t, _, _, _ in parts], dict(PP), **KW)
    first_tet = np.cumsum([0] + [len(p[1]) for p in parts])
    first_row = np.cumsum([0] + [len(p[2]) for p in parts])
    batch.setVisualMesh(np.concatenate([p[2] + np.array([first_tet[k], 0, 0, 0], np.float32) for k, p in enumerate(parts)]))
    tris = np.concatenate([p[3] + first_row[k] for k, p in enumerate(parts)])
    batch.setVisualTriangles(tris)
    solos = [SoftBodyHIP(v, t, None, dict(PP), vis, tri, **KW) for v, t, vis, tri, _ in parts]
    for b in [batch] + solos:
        b.setColliders(COLLIDER)
        if substeps:
            b.simulateSubsteps(substeps, DT, PP)
    row_body = np.concatenate([np.full(len(p[2]), k) for k, p in enumerate(parts)])
    first_tri = np.cumsum([0] + [len(p[3]) for p in parts])
    return batch, solos, tris, row_body, first_tri


@pytest.fixture(scope="module")
def world():
    """the three-lattice batch and its bodies alone, 40 substeps against one sphere collider; never stepped again"""
    return make_batch(40)


def solo_answer(solos, first_tri, o, d, b, near=0.0, far=np.inf):
    """every ray's record from ITS body alone (the host call), the triangle shifted into the batch's list"""
    want = np.zeros(len(o), dtype=RAY_HIT_DTYPE)
    near, far = np.broadcast_to(np.asarray(near, np.float64), len(o)), np.broadcast_to(np.asarray(far, np.float64), len(o))
    for k, solo in enumerate(solos):
        sel = np.flatnonzero(b == k)
        h = solo.raycastVisual(o[sel], d[sel], near[sel], far[sel])
        hit = h["hit"] == 1
        h["triangle"][hit] += first_tri[k]
        h["body"][hit] = k
        want[sel] = h
    return want


def test_a_batch_equals_its_bodies_alone(world):
    """1."""
    batch, solos, tris, row_body, first_tri = world
    o, d, b = ref.batch_rays()
    assert len(o) == 1000
    got = cast(batch, o, d, bodies=b)
    assert_same(got, solo_answer(solos, first_tri, o, d, b), "solo")
    pos = batch.exportTensors(("visPos",))["visPos"].cpu().numpy()
    for k, solo in enumerate(solos):                                              # (the bodies really are what they are alone, and deformed)
        mine = pos[row_body == k]
        assert np.array_equal(mine.view(np.uint32), solo.visualPositions().view(np.uint32))
        assert np.abs(mine - ref.batch_bodies()[k][4]).max() > 1e-3
    assert_same(got, ref.raycast(pos, tris, row_body, 3, o, d, bodies=b), "reference")
    assert ref.hit_share_ok(got["hit"]) and all(ref.hit_share_ok(got["hit"][b == k]) for k in range(3))


def test_order_independence(world):
    """2. sorted by body (uniform workgroups) and shuffled (mixed workgroups): the same record for the same ray"""
    batch = world[0]
    o, d, b = ref.batch_rays()
    order = np.argsort(b, kind="stable")
    shuffled = cast(batch, o, d, bodies=b)
    grouped = cast(batch, o[order], d[order], bodies=b[order])
    assert_same(grouped, shuffled[order])
    assert ref.hit_share_ok(grouped["hit"])
    again = np.random.default_rng(3).permutation(len(o))
    assert_same(cast(batch, o[again], d[again], bodies=b[again]), shuffled[again])


def test_without_bodies_the_batch_answers_as_its_host_call(world):
    """3a. every field, `body` included -- and it is often not the body the ray was made for"""
    batch, _, tris, row_body, _ = world
    o, d, b = ref.batch_rays()
    got = cast(batch, o, d)
    assert_same(got, batch.raycastVisual(o, d), "host")
    assert ref.hit_share_ok(got["hit"]) and int((got["body"] != np.where(got["hit"] == 1, b, -1)).sum()) >= 20
    single = world[1][1]                                                          # a single body: with zeros as bodies, and without
    o5, d5 = ref.seeded_rays(ref.batch_bodies()[1][4], *ref.STREAM_RAYS)
    want = single.raycastVisual(o5, d5)
    assert_same(cast(single, o5, d5), want)
    assert_same(cast(single, o5, d5, bodies=np.zeros(len(o5), np.int32)), want)


def test_many_rays_with_mixed_bodies_take_the_unsplit_launch(world):
    """More rays than the candidate buffer serves (131,072): one part, the record written by the cast itself -- on bodies of several
    tiles, in workgroups of mixed bodies.  The 1,000 rays of the batch test 140 times over, shuffled; against the bodies alone."""
    batch, solos, _, _, first_tri = world
    o, d, b = ref.batch_rays()
    want = solo_answer(solos, first_tri, o, d, b)
    at = np.random.default_rng(9).permutation(140 * len(o)) % len(o)
    assert len(at) == 140000 > 131072
    got = cast(batch, o[at], d[at], bodies=b[at])
    assert_same(got, want[at])
    assert ref.hit_share_ok(got["hit"])
    order = np.argsort(b[at], kind="stable")                                       # ... and grouped by body: uniform workgroups
    assert_same(cast(batch, o[at][order], d[at][order], bodies=b[at][order]), want[at][order])


def dragon(solver, precision):
    v, t = load_mesh("dragon")
    vis = load_f32("dragon_vis.f32").reshape(-1, 4)
    tris = np.fromfile(os.path.join(GOLDEN, "dragon_vistris.u16"), dtype="<u2").astype(np.int32).reshape(-1, 3)
    return SoftBodyHIP(v, t, None, dict(PP), vis, tris, solver=solver, precision=precision)


def test_without_bodies_a_deformed_dragon_answers_as_its_host_call():
    """3b. polar FAST, 200 substeps against the collider of test_gpu_raycast.py's second test, 1,024 rays"""
    body = dragon("polar", "fast")
    body.setColliders([dict(kind="sphere", a=[0.1, -0.4, 0.0], radius=1.0, friction=100.0)])
    body.simulateSubsteps(200, DT, PP)
    o, d = ref.seeded_rays(body.visualPositions(), 1024, 11)
    got = cast(body, o, d)
    assert_same(got, body.raycastVisual(o, d))
    assert 256 <= int(got["hit"].sum()) <= 1000
    assert_same(cast(body, o[:40], d[:40]), got[:40])                             # few rays: the triangle range split over many workgroups


def test_without_bodies_the_dragon_equals_the_threejs_fixtures():
    """3c. Neo-Hookean PRECISE after 10 substeps: three.js r160's own answers"""
    body = dragon("neohookean", "precise")
    dt = (1.0 * (1.0 / 60.0)) / 10
    for _ in range(10):
        body.simulate(dt, PP)
    rays, h32, h64, sphere = load_raycast_golden()
    got = cast(body, rays[:, 0:3], rays[:, 3:6], rays[:, 6], rays[:, 7])
    assert np.array_equal(got["hit"], h32[:, 0]) and np.array_equal(got["triangle"], h32[:, 1])
    assert np.array_equal(bits(got["distance"]), bits(h64[:, 0])) and np.array_equal(bits(got["point"]), bits(h64[:, 1:4]))
    assert np.array_equal(got["body"], np.where(h32[:, 0] == 1, 0, -1))
    s = body.visualBoundingSpheresDevice()
    torch.cuda.synchronize()
    assert np.array_equal(bits(s.cpu().numpy()[0]), bits(sphere))


@pytest.mark.parametrize("count", ref.COUNTS)
def test_counts(world, count):
    """4. on the lattice-2 body alone; 70,000 is more than a grid has rows"""
    solo = world[1][0]
    o, d, _ = ref.count_rays()
    o, d = o[:count], d[:count]
    got = cast(solo, o, d, bodies=np.zeros(count, np.int32))
    assert len(got) == count
    assert_same(got, solo.raycastVisual(o, d))
    assert_same(cast(solo, o, d), got)
    if count >= 63:
        assert ref.hit_share_ok(got["hit"])


def test_invalid_rays_disturb_nobody(world):
    """5. one of every kind among valid rays: -1 for it, the others bit-equal to a cast without it"""
    batch = world[0]
    n = ref.INVALID_RAYS[0] // 3
    o, d, b = ref.batch_rays({k: (n, ref.INVALID_RAYS[1] + k) for k in ref.LATTICES})
    near, far = np.zeros(len(o)), np.full(len(o), np.inf)
    clean = cast(batch, o, d, near, far, bodies=b)
    assert ref.hit_share_ok(clean["hit"])
    nan, inf = np.nan, np.inf
    kinds = [("o", [nan, 0, 0]), ("o", [0, -inf, 0]), ("d", [0, nan, 1]), ("d", [inf, 0, 0]), ("d", [0, 0, 0]), ("near", nan), ("far", nan),
             ("near", -1.0), ("far<near", None), ("b", 3), ("b", -1), ("b", 2 ** 31 - 1)]
    at = np.arange(len(kinds)) * 7 + 3
    for i, (what, value) in zip(at, kinds):
        if what == "o":
            o[i] = value
        elif what == "d":
            d[i] = value
        elif what == "near":
            near[i] = value
        elif what == "far":
            far[i] = value
        elif what == "far<near":
            near[i], far[i] = 2.0, 1.0
        else:
            b[i] = value
    got = cast(batch, o, d, near, far, bodies=b)
    bad = np.zeros(len(o), bool)
    bad[at] = True
    assert np.all(got["hit"][bad] == capi.RAY_INVALID) and np.all(got["body"][bad] == -1) and np.all(got["triangle"][bad] == -1)
    assert not got["distance"][bad].any() and not got["point"][bad].any() and not got["reserved"].any()
    assert_same(got[~bad], clean[~bad])
    pos = batch.visualPositions()
    assert_same(got, ref.raycast(pos, world[2], world[3], 3, o, d, near, far, bodies=b))
    nobody = cast(batch, o, d, near, far)                                         # without bodies a body is not looked at
    assert np.array_equal(nobody["hit"] == capi.RAY_INVALID, bad & (np.arange(len(o)) < at[9]))


def test_strides(world):
    """6. ray_stride 96, hit_stride 64 over sentinel-filled buffers, a guard row in front of each and one behind"""
    batch = world[0]
    o, d, b = ref.batch_rays()
    n = len(o)
    packed = rays_tensor(o, d)
    wide = torch.full((n + 2, 12), float("nan"), dtype=torch.float64, device="cuda")
    wide[1:-1, :8] = packed
    rays = wide[1:-1, :8]
    buf = torch.full((n + 2, 64), SENTINEL, dtype=torch.uint8, device="cuda")
    out = buf[1:-1, :48]
    assert rays.stride(0) * 8 == 96 and out.stride(0) == 64
    res = batch.raycastVisualDevice(rays, dev_i32(b), out=out)
    torch.cuda.synchronize()
    assert res["raw"] is out
    want = cast(batch, o, d, bodies=b)
    assert_same(records(out), want)
    host = buf.cpu().numpy()
    assert (host[0] == SENTINEL).all() and (host[-1] == SENTINEL).all() and (host[1:-1, 48:] == SENTINEL).all()
    for f in ("hit", "body", "triangle"):                                          # the views name the fields of the strided buffer
        assert res[f].dtype == torch.int32 and np.array_equal(res[f].cpu().numpy(), want[f]), f
    for f in ("distance", "point"):
        assert res[f].dtype == torch.float64 and np.array_equal(bits(res[f].cpu().numpy()), bits(want[f])), f
    assert torch.isnan(wide[:, 8:]).all() and torch.isnan(wide[0]).all() and torch.isnan(wide[-1]).all()


def test_stream_order():
    """7. rays written by torch work on a side stream right before the call, hits read by it right after; no synchronisation between"""
    v, t, vis, tris, rest = ref.lattice_surface(5)
    body = SoftBodyHIP(v, t, None, dict(PP), vis, tris, **KW)
    o, d = ref.seeded_rays(rest, *ref.STREAM_RAYS)
    src = rays_tensor(o, d)
    side = torch.cuda.Stream()
    rays = torch.zeros_like(src)
    torch.cuda.synchronize()
    with torch.cuda.stream(side):
        body.simulateSubsteps(20, DT, PP)
        big = torch.randn(4096, 4096, device="cuda")
        for _ in range(4):                                                         # work in front of the rays: a call that did not wait would read zeros
            big = big @ big * 1e-3
        rays.copy_(src + big[0, 0].double() * 0.0)
        res = body.raycastVisualDevice(rays)
        kept = res["raw"].clone()                                                  # torch work on the caller's stream, right behind the call
        rays.zero_()                                                               # ... which may reuse the rays at once
    torch.cuda.synchronize()
    want = body.raycastVisual(o, d)
    assert_same(records(kept), want)
    assert ref.hit_share_ok(want["hit"])
    rays.copy_(src)                                                                # the stream named explicitly, from another current stream
    torch.cuda.synchronize()
    res = body.raycastVisualDevice(rays, stream=side)
    side.synchronize()
    assert_same(records(res["raw"]), want)


@pytest.mark.parametrize("substeps", [40, 0])
def test_spheres(world, substeps):
    """8. every row equals the body's own sphere; padded rows keep their padding"""
    batch, solos = world[:2] if substeps else make_batch(0)[:2]
    buf = torch.full((5, 6), float("nan"), dtype=torch.float64, device="cuda")
    out = buf[1:4, :4]
    got = batch.visualBoundingSpheresDevice(out=out)
    packed = batch.visualBoundingSpheresDevice()
    torch.cuda.synchronize()
    assert got is out and tuple(packed.shape) == (3, 4) and packed.is_contiguous()
    for k, solo in enumerate(solos):
        c, r = solo.visualBoundingSphere()
        assert r > 0.1
        assert np.array_equal(bits(out[k].cpu().numpy()), bits(np.append(c, r))), k
    assert np.array_equal(bits(packed.cpu().numpy()), bits(out.cpu().numpy()))
    pos = batch.visualPositions()
    assert np.array_equal(bits(packed.cpu().numpy()), bits(ref.bounding_spheres(pos, world[3], 3)))
    assert torch.isnan(buf[0]).all() and torch.isnan(buf[4]).all() and torch.isnan(buf[:, 4:]).all()
    assert batch.visualBoundingSpheresDevice() is packed


def test_a_body_without_rows_or_triangles():
    """a miss for its rays, zeros as its sphere; the other body as ever"""
    parts = ref.batch_bodies()[:2]
    batch = SoftBodyHIP.batch([(v, t) for v, t, _, _, _ in parts], dict(PP), **KW)
    batch.setVisualMesh(parts[1][2] + np.array([len(parts[0][1]), 0, 0, 0], np.float32))   # rows on the second body only
    batch.setVisualTriangles(parts[1][3])
    solo = SoftBodyHIP(parts[1][0], parts[1][1], None, dict(PP), parts[1][2], parts[1][3], **KW)
    o, d = ref.seeded_rays(parts[1][4], 128, 5)
    got = cast(batch, o, d, bodies=np.tile([0, 1], 64))
    want = solo.raycastVisual(o, d)
    want["body"][want["hit"] == 1] = 1
    assert_same(got[1::2], want[1::2])
    assert not got["hit"][0::2].any() and np.all(got["body"][0::2] == -1) and want["hit"][1::2].sum() >= 16
    s = batch.visualBoundingSpheresDevice().cpu().numpy()
    c, r = solo.visualBoundingSphere()
    assert not s[0].any() and np.array_equal(bits(s[1]), bits(np.append(c, r)))


def test_errors(world):
    """9. every TETSIM_EINVAL / TETSIM_ESTATE case; the sentinel-filled hits are as they were"""
    L, hip = capi.lib(), _hip_runtime()
    batch = world[0]
    h, n = batch._h, 64
    o, d, b = ref.batch_rays()
    rays, bodies = rays_tensor(o[:n], d[:n]), dev_i32(b[:n])
    hits = torch.full((n, 48), SENTINEL, dtype=torch.uint8, device="cuda")
    dst = torch.full((3, 4), float("nan"), dtype=torch.float64, device="cuda")
    r, bp, hp, dp = rays.data_ptr(), bodies.data_ptr(), hits.data_ptr(), dst.data_ptr()
    host = np.zeros(n * 64, np.uint8)
    short = C.c_void_p()
    assert hip.hipMalloc(C.byref(short), C.c_size_t(n * 48 - 8)) == 0            # allocations of their own, one word too short
    assert hip.hipMemset(short, SENTINEL, C.c_size_t(n * 48 - 8)) == 0
    d0 = device_bytes(batch)

    def ray_call(*a):
        return L.tetsim_raycast_visual_device(h, *a)

    cases = [((None, 0, bp, n, hp, 0), "null"), ((r, 0, bp, n, None, 0), "null"),
             ((r, 60, bp, n, hp, 0), "ray_stride"), ((r, 68, bp, n, hp, 0), "ray_stride"), ((r, 8, bp, n, hp, 0), "ray_stride"),
             ((r, 0, bp, n, hp, 40), "hit_stride"), ((r, 0, bp, n, hp, 52), "hit_stride"),
             ((r + 4, 0, bp, n - 1, hp, 0), "rays is not 8-byte aligned"), ((r, 0, bp, n - 1, hp + 4, 0), "hits is not 8-byte aligned"),
             ((r, 0, bp + 2, n - 1, hp, 0), "ray_body is not 4-byte aligned"),
             ((host.ctypes.data, 0, bp, n, hp, 0), "rays is not device memory"), ((r, 0, bp, n, host.ctypes.data, 0), "hits is not device memory"),
             ((r, 0, host.ctypes.data, n, hp, 0), "ray_body is not device memory"),
             ((r, 0, bp, n, short.value, 0), "do not fit"), ((r, 0, None, n, short.value, 0), "do not fit")]
    for args, text in cases:
        rc = ray_call(*args, None)
        assert rc == capi.EINVAL, (args, rc, L.tetsim_last_error(h))
        assert text.encode() in L.tetsim_last_error(h), (args, L.tetsim_last_error(h))
    assert L.tetsim_raycast_visual_device(None, r, 0, bp, n, hp, 0, None) == capi.EINVAL
    if torch.cuda.device_count() > 1:                                             # memory of another device
        far_rays, far_bodies = rays.to("cuda:1"), bodies.to("cuda:1")
        far_hits, far_dst = torch.full((n, 48), SENTINEL, dtype=torch.uint8, device="cuda:1"), torch.zeros((3, 4), dtype=torch.float64, device="cuda:1")
        torch.cuda.synchronize("cuda:1")
        for args in ((far_rays.data_ptr(), 0, bp, n, hp, 0), (r, 0, far_bodies.data_ptr(), n, hp, 0), (r, 0, bp, n, far_hits.data_ptr(), 0)):
            assert ray_call(*args, None) == capi.EINVAL and b"is not device memory of device" in L.tetsim_last_error(h), (args, L.tetsim_last_error(h))
        assert L.tetsim_visual_bounding_spheres_device(h, far_dst.data_ptr(), 0, None) == capi.EINVAL
        assert b"is not device memory of device" in L.tetsim_last_error(h)
        assert (far_hits.cpu().numpy() == SENTINEL).all() and not far_dst.cpu().numpy().any()
    assert ray_call(None, 0, None, 0, None, 0, None) == capi.OK                   # count == 0 succeeds
    for args, text in (((None, 0), "null"), ((dp + 4, 0), "aligned"), ((dp, 24), "row_stride"), ((dp, 36), "row_stride"),
                       ((host.ctypes.data, 0), "not device memory"), ((short.value + n * 48 - 8 - 88, 0), "do not fit")):
        rc = L.tetsim_visual_bounding_spheres_device(h, args[0], args[1], None)
        assert rc == capi.EINVAL and text.encode() in L.tetsim_last_error(h), (args, rc, L.tetsim_last_error(h))
    assert L.tetsim_visual_bounding_spheres_device(None, dp, 0, None) == capi.EINVAL
    torch.cuda.synchronize()
    back = np.zeros(n * 48 - 8, np.uint8)
    assert hip.hipMemcpy(C.c_void_p(back.ctypes.data), short, C.c_size_t(back.size), 2) == 0 and (back == SENTINEL).all()
    assert hip.hipFree(short) == 0
    assert (hits.cpu().numpy() == SENTINEL).all() and torch.isnan(dst).all() and not host.any() and device_bytes(batch) == d0
    for bad in (rays.float(), rays[:, :7], rays.cpu()):
        with pytest.raises(ValueError):
            batch.raycastVisualDevice(bad)
    for bad in (bodies.long(), bodies[:-1], bodies.cpu()):
        with pytest.raises(ValueError):
            batch.raycastVisualDevice(rays, bad)
    with pytest.raises(ValueError):
        batch.raycastVisualDevice(rays, out=hits[:, :47])
    with pytest.raises(ValueError):
        batch.visualBoundingSpheresDevice(out=dst.float())

    # ---- TETSIM_ESTATE
    v, t, vis, tris, rest = ref.lattice_surface(2)

    def refused(body, text, sphere=True, bodies_too=True):
        calls = [lambda: body.raycastVisualDevice(rays, out=hits)]
        if bodies_too:
            calls.append(lambda: body.raycastVisualDevice(rays, torch.zeros(n, dtype=torch.int32, device="cuda"), out=hits))
        if sphere:
            calls.append(lambda: body.visualBoundingSpheresDevice())
        for call in calls:
            with pytest.raises(TetSimError) as e:
                call()
            assert e.value.code == capi.ESTATE and text in str(e.value), str(e.value)

    refused(SoftBodyHIP(v, t, None, dict(PP), **KW), "no visual mesh")
    notris = SoftBodyHIP(v, t, None, dict(PP), vis, **KW)
    refused(notris, "no visual triangles", sphere=False)
    assert notris.visualBoundingSpheresDevice().shape == (1, 4)                   # the spheres need no triangles
    part = SoftBodyHIP(v, t, None, dict(PP), vis, solver="polar", precision="fast", part_count=2, part_index=1)
    part.setVisualTriangles(tris)
    refused(part, "partition")
    # a triangle that spans two bodies: no per-body cast, and the whole mesh as ever
    parts = ref.batch_bodies()[:2]
    mixed = SoftBodyHIP.batch([(pv, pt) for pv, pt, _, _, _ in parts], dict(PP), **KW)
    mixed.setVisualMesh(np.concatenate([parts[0][2], parts[1][2] + np.array([len(parts[0][1]), 0, 0, 0], np.float32)]))
    rows0 = len(parts[0][2])
    mtris = np.concatenate([parts[0][3], parts[1][3] + rows0, [[0, 1, rows0]]]).astype(np.int32)
    mixed.setVisualTriangles(mtris)
    with pytest.raises(TetSimError) as e:
        mixed.raycastVisualDevice(rays, bodies.clamp(max=1), out=hits)
    assert e.value.code == capi.ESTATE and "different bodies" in str(e.value)
    torch.cuda.synchronize()
    assert (hits.cpu().numpy() == SENTINEL).all()
    assert_same(cast(mixed, o[:n], d[:n]), mixed.raycastVisual(o[:n], d[:n]))
    assert mixed.visualBoundingSpheresDevice().shape == (2, 4)
    # ... and the batch that was refused so much answers as before
    assert_same(cast(batch, o[:n], d[:n], bodies=b[:n]), cast(batch, o, d, bodies=b)[:n])


def test_nothing_else_moved():
    """10. a twin that never asked has the same state, byte for byte; device_bytes grows with the first call only"""
    v, t, vis, tris, rest = ref.lattice_surface(5)
    a, twin = (SoftBodyHIP(v, t, None, dict(PP), vis, tris, **KW) for _ in range(2))
    o, d = ref.seeded_rays(rest, *ref.STREAM_RAYS)
    rays, zeros = rays_tensor(o, d), torch.zeros(len(o), dtype=torch.int32, device="cuda")
    for x in (a, twin):
        x.simulateSubsteps(10, DT, PP)
    d0 = device_bytes(a)
    a.raycastVisualDevice(rays, zeros)
    a.visualBoundingSpheresDevice()
    a.raycastVisualDevice(rays)
    a.raycastVisualDevice(rays[:16], zeros[:16])
    d1 = device_bytes(a)
    assert d1 > d0
    for x in (a, twin):
        x.simulateSubsteps(10, DT, PP)
    for _ in range(3):
        a.raycastVisualDevice(rays, zeros)
        a.raycastVisualDevice(rays)
        a.raycastVisualDevice(rays[:16], zeros[:16])
        a.visualBoundingSpheresDevice()
    torch.cuda.synchronize()
    assert device_bytes(a) == d1
    assert a.saveState() == twin.saveState()
    for x in (a, twin):
        x.simulateSubsteps(5, DT, PP)
    assert np.array_equal(a.pos.view(np.uint32), twin.pos.view(np.uint32)) and np.array_equal(a.vel.view(np.uint32), twin.vel.view(np.uint32))
