"""Range sensors through the refitted tree (include/tetsim.h: tetsim_raycast_visual_bvh_device; SoftBodyHIP.raycastVisualBvhDevice): every
field of every record bit for bit against the definition in numpy (tests/raycast_bvh_ref.py: brute force, no tree) on the positions read
back from the device, and where stated against raycastVisualDevice in the same state.  Stale boxes, the edges of the tree's shape and the
brute-force parity are what catches a wrong tree; the rest is the contract of the brute-force call, asked of its twin."""
import ctypes as C
import os

import numpy as np
import pytest
import torch

import raycast_bvh_ref as bvh
import raycast_device_ref as ref
import raycast_ref
from conftest import GOLDEN
from test_gpu_raycast_device import DT, KW, PP, SENTINEL, assert_same, bits, dev_i32, dragon, make_batch, records
from test_gpu_snapshot import _hip_runtime, device_bytes
from test_raycast_bvh_cpu import records_differ
from test_raycast_cpu import load_raycast_golden
from tetsim_amd import SoftBodyHIP, TetSimError, place_rows, rays_tensor
from tetsim_amd import _capi as capi

pytestmark = pytest.mark.gpu


def cast(body, o, d, near=0.0, far=np.inf, bodies=None, brute=False, **kw):
    call = body.raycastVisualDevice if brute else body.raycastVisualBvhDevice
    res = call(rays_tensor(o, d, near, far), None if bodies is None else dev_i32(bodies), **kw)
    torch.cuda.synchronize()
    return records(res["raw"]).copy()


@pytest.fixture(scope="module")
def world():
    """the three-lattice batch (48, 300 and 1,728 triangles: one leaf level, a folded subtree, tops) and its bodies alone, 40 substeps against
    one sphere collider; never stepped again.  With it the batch's rays and the definition's answer for them."""
    batch, solos, tris, row_body, first_tri = make_batch(40)
    o, d, b = ref.batch_rays()
    pos = batch.visualPositions()
    want = bvh.raycast_device(pos, tris, row_body, 3, o, d, bodies=b)
    return dict(batch=batch, solos=solos, tris=tris, row_body=row_body, first_tri=first_tri, o=o, d=d, b=b, pos=pos, want=want)


def test_a_batch_equals_its_bodies_alone_in_any_ray_order(world):
    batch, o, d, b, want = world["batch"], world["o"], world["d"], world["b"], world["want"]
    got = cast(batch, o, d, bodies=b)
    assert_same(got, want, "definition")
    assert ref.hit_share_ok(got["hit"]) and all(ref.hit_share_ok(got["hit"][b == k]) for k in range(3))
    for k, solo in enumerate(world["solos"]):                                     # the body alone: its own handle, its own tree
        sel = np.flatnonzero(b == k)
        alone = cast(solo, o[sel], d[sel])
        hit = alone["hit"] == 1
        alone["triangle"][hit] += world["first_tri"][k]
        alone["body"][hit] = k
        assert_same(got[sel], alone, "solo %d" % k)
        assert_same(cast(solo, o[sel], d[sel], bodies=np.zeros(len(sel), np.int32)), cast(solo, o[sel], d[sel]), "zeros as bodies")
    grouped = np.argsort(b, kind="stable")
    for name, order in (("grouped", grouped), ("reversed", np.arange(len(o))[::-1]), ("shuffled", np.random.default_rng(3).permutation(len(o)))):
        assert_same(cast(batch, o[order], d[order], bodies=b[order]), got[order], name)
    assert_same(got, cast(batch, o, d, bodies=b, brute=True), "brute force")       # on these rays the two calls agree


def test_brute_force_parity_on_a_deformed_dragon():
    """40 substeps against a sphere, then the adversarial set built on the positions read back: the records equal the definition, the
    definition equals three.js's on every ray, and so the records equal raycastVisualDevice's.  (Should the agreement ever fail on a device
    state, that is a finding for DESIGN.md 9, not a tolerance to add.)"""
    body = dragon("polar", "fast")
    body.setColliders([dict(kind="sphere", a=[0.1, -0.4, 0.0], radius=1.0, friction=100.0)])
    body.simulateSubsteps(40, DT, PP)
    pos = body.visualPositions()
    tris = np.fromfile(os.path.join(GOLDEN, "dragon_vistris.u16"), dtype="<u2").astype(np.int32).reshape(-1, 3)
    o, d, near, far = bvh.adversarial_rays(pos, tris)
    stats = {}
    want = bvh.raycast(pos, tris, o, d, near, far, stats=stats)
    three = raycast_ref.raycast(pos, tris, o, d, near, far)
    print("accepted", stats, "hits", int((want["hit"] == 1).sum()), "differ", int(records_differ(want, three).sum()))
    assert int(records_differ(want, three).sum()) == 0 and stats["removed"] == 0
    assert stats["accepted"] > 0 and int((want["hit"] == 1).sum()) >= len(o) // 2
    got = cast(body, o, d, near, far)
    assert_same(got, want, "definition")
    assert_same(got, cast(body, o, d, near, far, brute=True), "brute force")
    assert_same(cast(body, o, d, near, far, bodies=np.zeros(len(o), np.int32)), got, "zeros as bodies")


def rays_at(pos, row_body, counts, seed):
    """every body's rays aimed at ITS current surface, shuffled"""
    o, d, b = [], [], []
    for k, n in enumerate(counts):
        ok, dk = ref.seeded_rays(pos[row_body == k], n, seed + k)
        o.append(ok), d.append(dk), b.append(np.full(n, k, np.int32))
    o, d, b = np.concatenate(o), np.concatenate(d), np.concatenate(b)
    perm = np.random.default_rng(seed).permutation(len(o))
    return o[perm], d[perm], b[perm]


def test_stale_boxes():
    """cast (which builds the tree), move every body several diameters away with a quarter turn, cast, step 20 substeps, cast: the answers are
    the definition's on the NEW positions each time.  A refit that is skipped, or that runs in front of the skinning, fails here."""
    batch, _, tris, row_body, _ = make_batch(10)
    shares = []

    def check(seed):
        pos = batch.visualPositions()
        o, d, b = rays_at(pos, row_body, (100, 100, 200), seed)
        got = cast(batch, o, d, bodies=b)
        assert_same(got, bvh.raycast_device(pos, tris, row_body, 3, o, d, bodies=b), "seed %d" % seed)
        assert_same(cast(batch, o, d), bvh.raycast_device(pos, tris, row_body, 3, o, d), "whole mesh, seed %d" % seed)
        assert ref.hit_share_ok(got["hit"])
        shares.append(int((got["hit"] == 1).sum()))
        return pos

    before = check(60)
    s = np.float32(np.sqrt(0.5))
    quarter = [[s, 0, 0, s], [0, s, 0, s], [0, 0, s, s]]                           # 90 degrees about x, y, z
    offsets = [[4.0, 1.0, 0.0], [0.0, 5.0, 3.0], [-6.0, 2.0, 4.0]]                 # the lattices are 1 wide
    pivots = [before[row_body == k].mean(axis=0) for k in range(3)]
    batch.placeBodies(place_rows(quarter, pivots, offsets))
    moved = check(61)
    for k in range(3):
        assert np.linalg.norm(moved[row_body == k].mean(axis=0) - before[row_body == k].mean(axis=0)) > 3.0
    wide = dict(PP, worldBounds=[-20.0, -20.0, -20.0, 20.0, 20.0, 20.0])
    batch.simulateSubsteps(20, DT, wide)
    stepped = check(62)
    assert np.abs(stepped - moved).max() > 1e-4                                    # (a sixtieth of a second of free fall: 1.4e-3)
    print("hits", shares)


TREE_EDGE_TRIANGLES = (None, 0, 1, 3, 4, 5, 33)   # None: a body without visual rows; then 0, 1, leaf - 1, leaf, leaf + 1, 8 * leaf + 1


def test_tree_edges():
    """seven lattice-2 bodies in a row whose own surfaces are the first k of the lattice's 48 boundary triangles"""
    v, t, vis, tri, rest = ref.lattice_surface(2)
    shift = [np.array([1.5 * k, 0.0, 0.0], np.float32) for k in range(len(TREE_EDGE_TRIANGLES))]
    wide = dict(PP, worldBounds=[-20.0, -1.0, -20.0, 20.0, 10.0, 20.0])
    batch = SoftBodyHIP.batch([((v + s).astype(np.float32), t) for s in shift], dict(wide), **KW)
    rows, tris, row_body, first_row = [], [], [], 0
    for k, n in enumerate(TREE_EDGE_TRIANGLES):
        if n is None:
            continue
        rows.append(vis + np.array([k * len(t), 0, 0, 0], np.float32))
        tris.append(tri[:n] + first_row)
        row_body.append(np.full(len(vis), k))
        first_row += len(vis)
    tris, row_body = np.concatenate(tris).astype(np.int32), np.concatenate(row_body)
    batch.setVisualMesh(np.concatenate(rows))
    batch.setVisualTriangles(tris)
    batch.simulateSubsteps(5, DT, wide)
    pos = batch.visualPositions()
    nb = len(TREE_EDGE_TRIANGLES)
    o, d, b = [], [], []
    for k in range(nb):                                                            # at every body's place, whatever it has there
        here = (rest + shift[k]).astype(np.float64)
        ok, dk = ref.seeded_rays(here.astype(np.float32), 96, 70 + k)
        o.append(ok), d.append(dk), b.append(np.full(96, k, np.int32))
        for a in tri[:TREE_EDGE_TRIANGLES[k] or 0]:                                # ... and straight at each of its triangles, from the front
            nrm = np.cross(here[a[1]] - here[a[0]], here[a[2]] - here[a[0]])
            nrm /= np.linalg.norm(nrm)
            o.append(here[a].mean(axis=0)[None, :] + 2.0 * nrm), d.append(-nrm[None, :]), b.append(np.full(1, k, np.int32))
    o, d, b = np.concatenate(o), np.concatenate(d), np.concatenate(b)
    perm = np.random.default_rng(8).permutation(len(o))
    o, d, b = o[perm], d[perm], b[perm]
    got = cast(batch, o, d, bodies=b)
    assert_same(got, bvh.raycast_device(pos, tris, row_body, nb, o, d, bodies=b), "bodies")
    assert_same(got, cast(batch, o, d, bodies=b, brute=True), "brute force")
    for k, n in enumerate(TREE_EDGE_TRIANGLES):
        hits = int((got["hit"][b == k] == 1).sum())
        assert (hits == 0) if not n else (hits >= 1), (k, n, hits)
    whole = cast(batch, o, d)
    assert_same(whole, bvh.raycast_device(pos, tris, row_body, nb, o, d), "whole mesh")
    assert int((whole["hit"] == 1).sum()) >= 20


def test_without_bodies(world):
    """the batch: the definition over the whole mesh, `body` that of the triangle; the Dragon: three.js r160's own answers"""
    batch, o, d, b = world["batch"], world["o"], world["d"], world["b"]
    got = cast(batch, o, d)
    assert_same(got, bvh.raycast_device(world["pos"], world["tris"], world["row_body"], 3, o, d), "definition")
    assert_same(got, cast(batch, o, d, brute=True), "brute force")
    assert ref.hit_share_ok(got["hit"]) and int((got["body"] != np.where(got["hit"] == 1, b, -1)).sum()) >= 20
    body = dragon("neohookean", "precise")
    dt = (1.0 * (1.0 / 60.0)) / 10
    for _ in range(10):
        body.simulate(dt, PP)
    rays, h32, h64, _ = load_raycast_golden()
    got = cast(body, rays[:, 0:3], rays[:, 3:6], rays[:, 6], rays[:, 7])
    assert np.array_equal(got["hit"], h32[:, 0]) and np.array_equal(got["triangle"], h32[:, 1])
    assert np.array_equal(bits(got["distance"]), bits(h64[:, 0])) and np.array_equal(bits(got["point"]), bits(h64[:, 1:4]))
    assert np.array_equal(got["body"], np.where(h32[:, 0] == 1, 0, -1))


@pytest.mark.parametrize("count", [0, 1, 63, 64, 65, 255, 256, 257, 1000])
def test_counts(world, count):
    """prefixes of the batch's shuffled rays: mixed bodies in every wave"""
    o, d, b = world["o"][:count], world["d"][:count], world["b"][:count]
    got = cast(world["batch"], o, d, bodies=b)
    assert len(got) == count
    assert_same(got, world["want"][:count])
    if count >= 63:
        assert ref.hit_share_ok(got["hit"])


def test_invalid_rays_disturb_nobody(world):
    batch = world["batch"]
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
    assert_same(got, bvh.raycast_device(world["pos"], world["tris"], world["row_body"], 3, o, d, near, far, bodies=b))
    nobody = cast(batch, o, d, near, far)                                          # without bodies a body is not looked at
    assert np.array_equal(nobody["hit"] == capi.RAY_INVALID, bad & (np.arange(len(o)) < at[9]))


def test_strides(world):
    """ray_stride 96, hit_stride 64 over sentinel-filled buffers, a guard row in front of each and one behind"""
    batch, o, d, b = world["batch"], world["o"], world["d"], world["b"]
    n = len(o)
    wide = torch.full((n + 2, 12), float("nan"), dtype=torch.float64, device="cuda")
    wide[1:-1, :8] = rays_tensor(o, d)
    rays = wide[1:-1, :8]
    buf = torch.full((n + 2, 64), SENTINEL, dtype=torch.uint8, device="cuda")
    out = buf[1:-1, :48]
    assert rays.stride(0) * 8 == 96 and out.stride(0) == 64
    res = batch.raycastVisualBvhDevice(rays, dev_i32(b), out=out)
    torch.cuda.synchronize()
    assert res["raw"] is out
    assert_same(records(out), world["want"])
    host = buf.cpu().numpy()
    assert (host[0] == SENTINEL).all() and (host[-1] == SENTINEL).all() and (host[1:-1, 48:] == SENTINEL).all()
    for f in ("hit", "body", "triangle"):
        assert res[f].dtype == torch.int32 and np.array_equal(res[f].cpu().numpy(), world["want"][f]), f
    assert torch.isnan(wide[:, 8:]).all() and torch.isnan(wide[0]).all() and torch.isnan(wide[-1]).all()


def test_stream_order():
    """rays written by torch work on a side stream right before the call, hits read by it right after; no synchronisation between.  The
    body is stepped on that stream first, so the refit has new positions to follow as well."""
    v, t, vis, tris, rest = ref.lattice_surface(5)
    body, twin = (SoftBodyHIP(v, t, None, dict(PP), vis, tris, **KW) for _ in range(2))
    o, d = ref.seeded_rays(rest, *ref.STREAM_RAYS)
    src = rays_tensor(o, d)
    body.raycastVisualBvhDevice(src)                                               # the tree exists, its boxes are those of the rest pose
    side = torch.cuda.Stream()
    rays = torch.zeros_like(src)
    torch.cuda.synchronize()
    with torch.cuda.stream(side):
        body.simulateSubsteps(20, DT, PP)
        big = torch.randn(4096, 4096, device="cuda")
        for _ in range(4):                                                         # work in front of the rays: a call that did not wait would read zeros
            big = big @ big * 1e-3
        rays.copy_(src + big[0, 0].double() * 0.0)
        res = body.raycastVisualBvhDevice(rays)
        kept = res["raw"].clone()                                                  # torch work on the caller's stream, right behind the call
        rays.zero_()                                                               # ... which may reuse the rays at once
    torch.cuda.synchronize()
    twin.simulateSubsteps(20, DT, PP)
    pos = twin.visualPositions()
    assert np.array_equal(pos.view(np.uint32), body.visualPositions().view(np.uint32))
    want = bvh.raycast_device(pos, tris, np.zeros(len(pos), np.int64), 1, o, d)
    assert_same(records(kept), want)
    assert ref.hit_share_ok(want["hit"])
    rays.copy_(src)                                                                # the stream named explicitly, from another current stream
    torch.cuda.synchronize()
    res = body.raycastVisualBvhDevice(rays, stream=side)
    side.synchronize()
    assert_same(records(res["raw"]), want)


def test_errors(world):
    """the error list of tetsim_raycast_visual_device; the sentinel-filled hits are as they were"""
    L, hip = capi.lib(), _hip_runtime()
    batch, o, d, b = world["batch"], world["o"], world["d"], world["b"]
    h, n = batch._h, 64
    rays, bodies = rays_tensor(o[:n], d[:n]), dev_i32(b[:n])
    hits = torch.full((n, 48), SENTINEL, dtype=torch.uint8, device="cuda")
    r, bp, hp = rays.data_ptr(), bodies.data_ptr(), hits.data_ptr()
    host = np.zeros(n * 64, np.uint8)
    short = C.c_void_p()
    assert hip.hipMalloc(C.byref(short), C.c_size_t(n * 48 - 8)) == 0            # an allocation of its own, one word too short
    assert hip.hipMemset(short, SENTINEL, C.c_size_t(n * 48 - 8)) == 0
    d0 = device_bytes(batch)
    cases = [((None, 0, bp, n, hp, 0), "null"), ((r, 0, bp, n, None, 0), "null"),
             ((r, 60, bp, n, hp, 0), "ray_stride"), ((r, 68, bp, n, hp, 0), "ray_stride"), ((r, 8, bp, n, hp, 0), "ray_stride"),
             ((r, 0, bp, n, hp, 40), "hit_stride"), ((r, 0, bp, n, hp, 52), "hit_stride"),
             ((r + 4, 0, bp, n - 1, hp, 0), "rays is not 8-byte aligned"), ((r, 0, bp, n - 1, hp + 4, 0), "hits is not 8-byte aligned"),
             ((r, 0, bp + 2, n - 1, hp, 0), "ray_body is not 4-byte aligned"),
             ((host.ctypes.data, 0, bp, n, hp, 0), "rays is not device memory"), ((r, 0, bp, n, host.ctypes.data, 0), "hits is not device memory"),
             ((r, 0, host.ctypes.data, n, hp, 0), "ray_body is not device memory"),
             ((r, 0, bp, n, short.value, 0), "do not fit"), ((r, 0, None, n, short.value, 0), "do not fit")]
    for args, text in cases:
        rc = L.tetsim_raycast_visual_bvh_device(h, *args, None)
        assert rc == capi.EINVAL, (args, rc, L.tetsim_last_error(h))
        assert text.encode() in L.tetsim_last_error(h), (args, L.tetsim_last_error(h))
    assert L.tetsim_raycast_visual_bvh_device(None, r, 0, bp, n, hp, 0, None) == capi.EINVAL
    assert L.tetsim_raycast_visual_bvh_device(h, None, 0, None, 0, None, 0, None) == capi.OK   # count == 0 succeeds
    torch.cuda.synchronize()
    back = np.zeros(n * 48 - 8, np.uint8)
    assert hip.hipMemcpy(C.c_void_p(back.ctypes.data), short, C.c_size_t(back.size), 2) == 0 and (back == SENTINEL).all()
    assert hip.hipFree(short) == 0
    assert (hits.cpu().numpy() == SENTINEL).all() and not host.any() and device_bytes(batch) == d0
    for bad in (rays.float(), rays[:, :7], rays.cpu()):
        with pytest.raises(ValueError):
            batch.raycastVisualBvhDevice(bad)
    for bad in (bodies.long(), bodies[:-1], bodies.cpu()):
        with pytest.raises(ValueError):
            batch.raycastVisualBvhDevice(rays, bad)
    with pytest.raises(ValueError):
        batch.raycastVisualBvhDevice(rays, out=hits[:, :47])

    # ---- TETSIM_ESTATE
    v, t, vis, tris, rest = ref.lattice_surface(2)

    def refused(body, text, bodies_too=True):
        calls = [lambda: body.raycastVisualBvhDevice(rays, out=hits)]
        if bodies_too:
            calls.append(lambda: body.raycastVisualBvhDevice(rays, torch.zeros(n, dtype=torch.int32, device="cuda"), out=hits))
        for call in calls:
            with pytest.raises(TetSimError) as e:
                call()
            assert e.value.code == capi.ESTATE and text in str(e.value), str(e.value)

    refused(SoftBodyHIP(v, t, None, dict(PP), **KW), "no visual mesh")
    refused(SoftBodyHIP(v, t, None, dict(PP), vis, **KW), "no visual triangles")
    part = SoftBodyHIP(v, t, None, dict(PP), vis, solver="polar", precision="fast", part_count=2, part_index=1)
    part.setVisualTriangles(tris)
    refused(part, "partition")
    # a triangle that spans two bodies: no per-body cast; without bodies it belongs to the body of its first row
    parts = ref.batch_bodies()[:2]
    mixed = SoftBodyHIP.batch([(pv, pt) for pv, pt, _, _, _ in parts], dict(PP), **KW)
    mixed.setVisualMesh(np.concatenate([parts[0][2], parts[1][2] + np.array([len(parts[0][1]), 0, 0, 0], np.float32)]))
    rows0 = len(parts[0][2])
    mtris = np.concatenate([parts[0][3], parts[1][3] + rows0, [[0, 1, rows0]]]).astype(np.int32)
    mixed.setVisualTriangles(mtris)
    with pytest.raises(TetSimError) as e:
        mixed.raycastVisualBvhDevice(rays, bodies.clamp(max=1), out=hits)
    assert e.value.code == capi.ESTATE and "different bodies" in str(e.value)
    torch.cuda.synchronize()
    assert (hits.cpu().numpy() == SENTINEL).all()
    mrow_body = np.concatenate([np.zeros(rows0, np.int64), np.ones(len(parts[1][2]), np.int64)])
    assert_same(cast(mixed, o[:n], d[:n]), bvh.raycast_device(mixed.visualPositions(), mtris, mrow_body, 2, o[:n], d[:n]))
    # ... and the batch that was refused so much answers as before
    assert_same(cast(batch, o[:n], d[:n], bodies=b[:n]), world["want"][:n])


def test_nothing_else_moved():
    """a twin that never asked has the same state, byte for byte; raycastVisualDevice answers the same before and after the tree exists;
    device_bytes rises once, at the first call, and not with count"""
    v, t, vis, tris, rest = ref.lattice_surface(5)
    a, twin = (SoftBodyHIP(v, t, None, dict(PP), vis, tris, **KW) for _ in range(2))
    o, d = ref.seeded_rays(rest, *ref.STREAM_RAYS)
    rays, zeros = rays_tensor(o, d), torch.zeros(len(o), dtype=torch.int32, device="cuda")
    many = rays.repeat(40, 1)
    for x in (a, twin):
        x.simulateSubsteps(10, DT, PP)
    before = cast(a, o, d, bodies=np.zeros(len(o), np.int32), brute=True)           # (the brute-force call's own tables exist from here on)
    state = a.saveState()
    d0 = device_bytes(a)
    a.raycastVisualBvhDevice(rays[:16], zeros[:16])
    d1 = device_bytes(a)
    assert d1 > d0
    a.raycastVisualBvhDevice(rays, zeros)
    a.raycastVisualBvhDevice(rays)
    a.raycastVisualBvhDevice(many)
    torch.cuda.synchronize()
    assert device_bytes(a) == d1
    assert a.saveState() == state == twin.saveState()
    assert_same(cast(a, o, d, bodies=np.zeros(len(o), np.int32), brute=True), before)
    for x in (a, twin):
        x.simulateSubsteps(10, DT, PP)
    a.raycastVisualBvhDevice(rays, zeros)
    torch.cuda.synchronize()
    assert device_bytes(a) == d1 and a.saveState() == twin.saveState()
    for x in (a, twin):
        x.simulateSubsteps(5, DT, PP)
    assert np.array_equal(a.pos.view(np.uint32), twin.pos.view(np.uint32)) and np.array_equal(a.vel.view(np.uint32), twin.vel.view(np.uint32))
