"""Closest-point queries through the refitted tree (include/tetsim.h: tetsim_closest_visual_device / tetsim_closest_visual;
SoftBodyHIP.closestPointsDevice / closestPoints): every field of every record bit for bit against the definition in numpy
(tests/closest_ref.py: brute force, no tree) on the positions read back from the device.  The fixtures are those of
tests/test_gpu_raycast_device.py and tests/test_gpu_raycast_bvh.py: the three-lattice batch and the row of bodies at the tree's edges."""
import ctypes as C
import os

import numpy as np
import pytest
import torch

import closest_ref as cref
import raycast_device_ref as ref
from conftest import GOLDEN
from test_closest_cpu import bits
from test_gpu_raycast_bvh import TREE_EDGE_TRIANGLES
from test_gpu_raycast_bvh import cast as cast_rays
from test_gpu_raycast_device import DT, KW, PP, SENTINEL, dev_i32, dragon, make_batch
from test_gpu_raycast_device import assert_same as assert_same_hits
from test_gpu_snapshot import _hip_runtime, device_bytes
from tetsim_amd import CLOSEST_DTYPE, SoftBodyHIP, TetSimError, place_rows, point_queries_tensor
from tetsim_amd import _capi as capi

pytestmark = pytest.mark.gpu


def records(raw):
    """the packed TetSimClosest records of a [count, 64] uint8 tensor, on the host"""
    return np.frombuffer(raw.contiguous().cpu().numpy().tobytes(), dtype=CLOSEST_DTYPE)


def ask(body, points, limit=np.inf, bodies=None, **kw):
    res = body.closestPointsDevice(point_queries_tensor(points, limit), None if bodies is None else dev_i32(bodies), **kw)
    torch.cuda.synchronize()
    return records(res["raw"]).copy()


def assert_same(got, want, what=""):
    assert len(got) == len(want), what
    for f in ("found", "body", "triangle", "region"):
        assert np.array_equal(got[f], want[f]), (what, f, np.flatnonzero(got[f] != want[f])[:8])
    for f in ("distance", "point", "v", "w"):
        assert np.array_equal(bits(got[f]), bits(want[f])), (what, f)


@pytest.fixture(scope="module")
def world():
    """the three-lattice batch (48, 300 and 1,728 triangles: one leaf level, a folded subtree, tops) and its bodies alone, 40 substeps against
    one sphere collider; never stepped again.  With it the batch's queries and the definition's answer for them."""
    batch, solos, tris, row_body, first_tri = make_batch(40)
    p, m, b = cref.batch_queries()
    pos = batch.visualPositions()
    want = cref.closest_device(pos, tris, row_body, 3, p, m, bodies=b)
    return dict(batch=batch, solos=solos, tris=tris, row_body=row_body, first_tri=first_tri, p=p, m=m, b=b, pos=pos, want=want)


def test_a_batch_equals_its_bodies_alone_in_any_query_order(world):
    batch, p, m, b, want = world["batch"], world["p"], world["m"], world["b"], world["want"]
    assert len(p) == 1000
    got = ask(batch, p, m, bodies=b)
    assert_same(got, want, "definition")
    assert cref.found_share_ok(got["found"]) and all(cref.found_share_ok(got["found"][b == k]) for k in range(3))
    assert set(got["region"][got["found"] == 1].tolist()) == set(range(7))
    for k, solo in enumerate(world["solos"]):                                     # the body alone: its own handle, its own tree
        sel = np.flatnonzero(b == k)
        alone = ask(solo, p[sel], m[sel])
        found = alone["found"] == 1
        alone["triangle"][found] += world["first_tri"][k]
        alone["body"][found] = k
        assert_same(got[sel], alone, "solo %d" % k)
        assert_same(ask(solo, p[sel], m[sel], bodies=np.zeros(len(sel), np.int32)), ask(solo, p[sel], m[sel]), "zeros as bodies")
    grouped = np.argsort(b, kind="stable")
    for name, order in (("grouped", grouped), ("reversed", np.arange(len(p))[::-1]), ("shuffled", np.random.default_rng(3).permutation(len(p)))):
        assert_same(ask(batch, p[order], m[order], bodies=b[order]), got[order], name)


def test_without_query_body(world):
    """the definition over the whole mesh, `body` that of the winner's first row -- often not the body the query was made for"""
    batch, p, m, b = world["batch"], world["p"], world["m"], world["b"]
    got = ask(batch, p, m)
    assert_same(got, cref.closest_device(world["pos"], world["tris"], world["row_body"], 3, p, m), "definition")
    assert cref.found_share_ok(got["found"]) and int((got["body"] != np.where(got["found"] == 1, b, -1)).sum()) >= 20


def test_a_deformed_dragon():
    """40 substeps against a sphere, then the adversarial set built on the positions read back: the records equal the definition, whose box
    predicate removed nothing, and with an infinite max_distance every valid query is found"""
    body = dragon("polar", "fast")
    body.setColliders([dict(kind="sphere", a=[0.1, -0.4, 0.0], radius=1.0, friction=100.0)])
    body.simulateSubsteps(40, DT, PP)
    pos = body.visualPositions()
    tris = np.fromfile(os.path.join(GOLDEN, "dragon_vistris.u16"), dtype="<u2").astype(np.int32).reshape(-1, 3)
    p, m = cref.adversarial_queries(pos, tris)
    stats = {}
    want = cref.closest_device(pos, tris, np.zeros(len(pos), np.int64), 1, p, m, stats=stats)
    print(stats, "found", int((want["found"] == 1).sum()), "of", len(p))
    assert stats["rejected"] == 0 and np.all(want["found"][np.isinf(m)] == 1)
    got = ask(body, p, m)
    assert_same(got, want, "definition")
    assert int((got["found"] == 1).sum()) >= 0.95 * int(np.isinf(m).sum()) and np.all(got["found"][np.isinf(m)] == 1)
    n = cref.ADVERSARIAL_PER_KIND
    assert np.all(got["found"][-2 * n:-n] == 0) and np.all(got["found"][-n:] == 1)   # max_distance a hair below, a hair above
    assert_same(ask(body, p, m, bodies=np.zeros(len(p), np.int32)), got, "zeros as bodies")


def queries_at(pos, row_body, counts, seed):
    """every body's queries around ITS current surface, shuffled"""
    p, m, b = [], [], []
    for k, n in enumerate(counts):
        pk, mk = cref.seeded_points(pos[row_body == k], n, seed + k)
        p.append(pk), m.append(mk), b.append(np.full(n, k, np.int32))
    p, m, b = np.concatenate(p), np.concatenate(m), np.concatenate(b)
    perm = np.random.default_rng(seed).permutation(len(p))
    return p[perm], m[perm], b[perm]


def test_stale_boxes():
    """query (which builds the tree), move every body several diameters away with a quarter turn, query, step 20 substeps, query: the answers
    are the definition's on the NEW positions each time.  A refit that is skipped, or that runs in front of the skinning, fails here."""
    batch, _, tris, row_body, _ = make_batch(10)

    def check(seed):
        pos = batch.visualPositions()
        p, m, b = queries_at(pos, row_body, (100, 100, 200), seed)
        got = ask(batch, p, m, bodies=b)
        assert_same(got, cref.closest_device(pos, tris, row_body, 3, p, m, bodies=b), "seed %d" % seed)
        assert_same(ask(batch, p, m), cref.closest_device(pos, tris, row_body, 3, p, m), "whole mesh, seed %d" % seed)
        assert cref.found_share_ok(got["found"])
        return pos

    before = check(160)
    s = np.float32(np.sqrt(0.5))
    quarter = [[s, 0, 0, s], [0, s, 0, s], [0, 0, s, s]]                           # 90 degrees about x, y, z
    offsets = [[4.0, 1.0, 0.0], [0.0, 5.0, 3.0], [-6.0, 2.0, 4.0]]                 # the lattices are 1 wide
    pivots = [before[row_body == k].mean(axis=0) for k in range(3)]
    batch.placeBodies(place_rows(quarter, pivots, offsets))
    moved = check(161)
    for k in range(3):
        assert np.linalg.norm(moved[row_body == k].mean(axis=0) - before[row_body == k].mean(axis=0)) > 3.0
    wide = dict(PP, worldBounds=[-20.0, -20.0, -20.0, 20.0, 20.0, 20.0])
    batch.simulateSubsteps(20, DT, wide)
    stepped = check(162)
    assert np.abs(stepped - moved).max() > 1e-4


def test_tree_edges():
    """seven lattice-2 bodies in a row whose own surfaces are the first k of the lattice's 48 boundary triangles: a body without rows or
    without triangles finds nothing, every other body finds a point for every query without a limit"""
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
    p, m, b = [], [], []
    for k in range(nb):                                                            # around every body's place, whatever it has there
        pk, mk = cref.seeded_points((rest + shift[k]).astype(np.float32), 96, 170 + k)
        p.append(pk), m.append(mk), b.append(np.full(96, k, np.int32))
    p, m, b = np.concatenate(p), np.concatenate(m), np.concatenate(b)
    perm = np.random.default_rng(8).permutation(len(p))
    p, m, b = p[perm], m[perm], b[perm]
    got = ask(batch, p, m, bodies=b)
    assert_same(got, cref.closest_device(pos, tris, row_body, nb, p, m, bodies=b), "bodies")
    for k, n in enumerate(TREE_EDGE_TRIANGLES):
        mine = b == k
        if not n:
            assert np.all(got["found"][mine] == 0), (k, n)
        else:
            assert np.all(got["found"][mine & np.isinf(m)] == 1), (k, n)
    whole = ask(batch, p, m)
    assert_same(whole, cref.closest_device(pos, tris, row_body, nb, p, m), "whole mesh")
    assert np.all(whole["found"][np.isinf(m)] == 1)


@pytest.mark.parametrize("count", [0, 1, 63, 64, 65, 255, 256, 257, 1000])
def test_counts(world, count):
    """prefixes of the batch's shuffled queries: mixed bodies in every wave"""
    p, m, b = world["p"][:count], world["m"][:count], world["b"][:count]
    got = ask(world["batch"], p, m, bodies=b)
    assert len(got) == count
    assert_same(got, world["want"][:count])
    if count >= 63:
        assert cref.found_share_ok(got["found"]) and len(set(b.tolist())) == 3


def test_invalid_queries_disturb_nobody(world):
    batch = world["batch"]
    p, m, b = cref.batch_queries({k: (32, 140 + k) for k in ref.LATTICES})
    clean = ask(batch, p, m, bodies=b)
    assert cref.found_share_ok(clean["found"])
    nan, inf = np.nan, np.inf
    kinds = [("p", [nan, 0, 0]), ("p", [0, -inf, 0]), ("p", [0, 0, inf]), ("m", nan), ("m", -1.0), ("m", -inf), ("b", 3), ("b", -1), ("b", 2 ** 31 - 1)]
    at = np.arange(len(kinds)) * 7 + 3
    for i, (what, value) in zip(at, kinds):
        if what == "p":
            p[i] = value
        elif what == "m":
            m[i] = value
        else:
            b[i] = value
    good = at[-1] + 2                                                              # ... and what stays valid: no limit, a limit of zero
    m[good], m[good + 1] = inf, 0.0
    got = ask(batch, p, m, bodies=b)
    bad = np.zeros(len(p), bool)
    bad[at] = True
    assert np.all(got["found"][bad] == capi.CLOSEST_INVALID)
    for f in ("body", "triangle", "region"):
        assert np.all(got[f][bad] == -1), f
    for f in ("distance", "point", "v", "w"):
        assert not bits(got[f][bad]).any(), f
    keep = ~bad
    keep[[good, good + 1]] = False
    assert_same(got[keep], clean[keep])
    assert got["found"][good] == 1
    assert_same(got, cref.closest_device(world["pos"], world["tris"], world["row_body"], 3, p, m, bodies=b))
    nobody = ask(batch, p, m)                                                      # without bodies a body is not looked at
    assert np.array_equal(nobody["found"] == capi.CLOSEST_INVALID, bad & (np.arange(len(p)) < at[6]))


def test_strides(world):
    """query stride 48, out stride 96 over sentinel-filled buffers, a guard row in front of each and one behind"""
    batch, p, m, b = world["batch"], world["p"], world["m"], world["b"]
    n = len(p)
    wide = torch.full((n + 2, 6), float("nan"), dtype=torch.float64, device="cuda")
    wide[1:-1, :4] = point_queries_tensor(p, m)
    queries = wide[1:-1, :4]
    buf = torch.full((n + 2, 96), SENTINEL, dtype=torch.uint8, device="cuda")
    out = buf[1:-1, :64]
    assert queries.stride(0) * 8 == 48 and out.stride(0) == 96
    res = batch.closestPointsDevice(queries, dev_i32(b), out=out)
    torch.cuda.synchronize()
    assert res["raw"] is out
    assert_same(records(out), world["want"])
    host = buf.cpu().numpy()
    assert (host[0] == SENTINEL).all() and (host[-1] == SENTINEL).all() and (host[1:-1, 64:] == SENTINEL).all()
    for f in ("found", "body", "triangle", "region"):
        assert res[f].dtype == torch.int32 and np.array_equal(res[f].cpu().numpy(), world["want"][f]), f
    for f in ("distance", "point", "v", "w"):
        assert res[f].dtype == torch.float64 and np.array_equal(bits(res[f].cpu().numpy()), bits(world["want"][f])), f
    assert torch.isnan(wide[:, 4:]).all() and torch.isnan(wide[0]).all() and torch.isnan(wide[-1]).all()


def test_stream_order():
    """queries written by torch work on a side stream right before the call, records read by it right after; no synchronisation between.
    The body is stepped on that stream first, so the refit has new positions to follow as well."""
    v, t, vis, tris, rest = ref.lattice_surface(5)
    body, twin = (SoftBodyHIP(v, t, None, dict(PP), vis, tris, **KW) for _ in range(2))
    p, m = cref.seeded_points(rest, *cref.STREAM_QUERIES)
    src = point_queries_tensor(p, m)
    body.closestPointsDevice(src)                                                  # the tree exists, its boxes are those of the rest pose
    side = torch.cuda.Stream()
    queries = torch.full_like(src, float("nan"))                                   # a call that did not wait would read invalid queries
    torch.cuda.synchronize()
    with torch.cuda.stream(side):
        body.simulateSubsteps(20, DT, PP)
        big = torch.randn(4096, 4096, device="cuda")
        for _ in range(4):                                                         # work in front of the queries
            big = big @ big * 1e-3
        queries.copy_(src + big[0, 0].double() * 0.0)
        res = body.closestPointsDevice(queries)
        kept = res["raw"].clone()                                                  # torch work on the caller's stream, right behind the call
        queries.fill_(float("nan"))                                                # ... which may reuse the queries at once
    torch.cuda.synchronize()
    twin.simulateSubsteps(20, DT, PP)
    pos = twin.visualPositions()
    assert np.array_equal(pos.view(np.uint32), body.visualPositions().view(np.uint32))
    want = cref.closest_device(pos, tris, np.zeros(len(pos), np.int64), 1, p, m)
    assert_same(records(kept), want)
    assert cref.found_share_ok(want["found"])
    queries.copy_(src)                                                             # the stream named explicitly, from another current stream
    torch.cuda.synchronize()
    res = body.closestPointsDevice(queries, stream=side)
    side.synchronize()
    assert_same(records(res["raw"]), want)


def test_errors(world):
    """the error list of tetsim_raycast_visual_bvh_device; the sentinel-filled records are as they were and device_bytes has not moved"""
    L, hip = capi.lib(), _hip_runtime()
    batch, p, m, b = world["batch"], world["p"], world["m"], world["b"]
    h, n = batch._h, 64
    queries, bodies = point_queries_tensor(p[:n], m[:n]), dev_i32(b[:n])
    out = torch.full((n, 64), SENTINEL, dtype=torch.uint8, device="cuda")
    q, bp, op = queries.data_ptr(), bodies.data_ptr(), out.data_ptr()
    host = np.zeros(n * 64, np.uint8)
    short = C.c_void_p()
    assert hip.hipMalloc(C.byref(short), C.c_size_t(n * 64 - 8)) == 0            # an allocation of its own, one word too short
    assert hip.hipMemset(short, SENTINEL, C.c_size_t(n * 64 - 8)) == 0
    d0 = device_bytes(batch)
    cases = [((None, 0, bp, n, op, 0), "null"), ((q, 0, bp, n, None, 0), "null"),
             ((q, 28, bp, n, op, 0), "query_stride"), ((q, 36, bp, n, op, 0), "query_stride"), ((q, 8, bp, n, op, 0), "query_stride"),
             ((q, 0, bp, n, op, 56), "out_stride"), ((q, 0, bp, n, op, 68), "out_stride"),
             ((q + 4, 0, bp, n - 1, op, 0), "queries is not 8-byte aligned"), ((q, 0, bp, n - 1, op + 4, 0), "out is not 8-byte aligned"),
             ((q, 0, bp + 2, n - 1, op, 0), "query_body is not 4-byte aligned"),
             ((host.ctypes.data, 0, bp, n, op, 0), "queries is not device memory"), ((q, 0, bp, n, host.ctypes.data, 0), "out is not device memory"),
             ((q, 0, host.ctypes.data, n, op, 0), "query_body is not device memory"),
             ((q, 0, bp, n, short.value, 0), "do not fit"), ((q, 0, None, n, short.value, 0), "do not fit")]
    for args, text in cases:
        rc = L.tetsim_closest_visual_device(h, *args, None)
        assert rc == capi.EINVAL, (args, rc, L.tetsim_last_error(h))
        assert text.encode() in L.tetsim_last_error(h), (args, L.tetsim_last_error(h))
    assert L.tetsim_closest_visual_device(None, q, 0, bp, n, op, 0, None) == capi.EINVAL
    assert L.tetsim_closest_visual_device(h, None, 0, None, 0, None, 0, None) == capi.OK   # count == 0 succeeds
    torch.cuda.synchronize()
    back = np.zeros(n * 64 - 8, np.uint8)
    assert hip.hipMemcpy(C.c_void_p(back.ctypes.data), short, C.c_size_t(back.size), 2) == 0 and (back == SENTINEL).all()
    assert hip.hipFree(short) == 0
    assert (out.cpu().numpy() == SENTINEL).all() and not host.any() and device_bytes(batch) == d0
    for bad in (queries.float(), queries[:, :3], queries.cpu()):
        with pytest.raises(ValueError):
            batch.closestPointsDevice(bad)
    for bad in (bodies.long(), bodies[:-1], bodies.cpu()):
        with pytest.raises(ValueError):
            batch.closestPointsDevice(queries, bad)
    with pytest.raises(ValueError):
        batch.closestPointsDevice(queries, out=out[:, :63])

    # ---- TETSIM_ESTATE
    v, t, vis, tris, rest = ref.lattice_surface(2)

    def refused(body, text):
        for call in (lambda: body.closestPointsDevice(queries, out=out),
                     lambda: body.closestPointsDevice(queries, torch.zeros(n, dtype=torch.int32, device="cuda"), out=out),
                     lambda: body.closestPoints(p[:n], m[:n])):
            with pytest.raises(TetSimError) as e:
                call()
            assert e.value.code == capi.ESTATE and text in str(e.value), str(e.value)

    refused(SoftBodyHIP(v, t, None, dict(PP), **KW), "no visual mesh")
    refused(SoftBodyHIP(v, t, None, dict(PP), vis, **KW), "no visual triangles")
    part = SoftBodyHIP(v, t, None, dict(PP), vis, solver="polar", precision="fast", part_count=2, part_index=1)
    part.setVisualTriangles(tris)
    refused(part, "partition")
    # a triangle that spans two bodies: no per-body query; without bodies it belongs to the body of its first row
    parts = ref.batch_bodies()[:2]
    mixed = SoftBodyHIP.batch([(pv, pt) for pv, pt, _, _, _ in parts], dict(PP), **KW)
    mixed.setVisualMesh(np.concatenate([parts[0][2], parts[1][2] + np.array([len(parts[0][1]), 0, 0, 0], np.float32)]))
    rows0 = len(parts[0][2])
    mtris = np.concatenate([parts[0][3], parts[1][3] + rows0, [[0, 1, rows0]]]).astype(np.int32)
    mixed.setVisualTriangles(mtris)
    with pytest.raises(TetSimError) as e:
        mixed.closestPointsDevice(queries, bodies.clamp(max=1), out=out)
    assert e.value.code == capi.ESTATE and "different bodies" in str(e.value)
    torch.cuda.synchronize()
    assert (out.cpu().numpy() == SENTINEL).all()
    mrow_body = np.concatenate([np.zeros(rows0, np.int64), np.ones(len(parts[1][2]), np.int64)])
    assert_same(ask(mixed, p[:n], m[:n]), cref.closest_device(mixed.visualPositions(), mtris, mrow_body, 2, p[:n], m[:n]))
    # ... and the batch that was refused so much answers as before
    assert_same(ask(batch, p[:n], m[:n], bodies=b[:n]), world["want"][:n])


def test_nothing_else_moved():
    """a twin that never asked has the same state, byte for byte; raycastVisualBvhDevice answers the same before and after; device_bytes
    rises at most once -- not at all where the ray call has built the tree already -- and not with count"""
    v, t, vis, tris, rest = ref.lattice_surface(5)
    a, twin, c = (SoftBodyHIP(v, t, None, dict(PP), vis, tris, **KW) for _ in range(3))
    p, m = cref.seeded_points(rest, *cref.STREAM_QUERIES)
    o, d = ref.seeded_rays(rest, *ref.STREAM_RAYS)
    queries, zeros = point_queries_tensor(p, m), torch.zeros(len(p), dtype=torch.int32, device="cuda")
    many = queries.repeat(40, 1)
    for x in (a, twin, c):
        x.simulateSubsteps(10, DT, PP)
    state = a.saveState()
    d0 = device_bytes(a)
    a.closestPointsDevice(queries[:16], zeros[:16])                                # this handle's first tree call is this one
    d1 = device_bytes(a)
    assert d1 > d0
    a.closestPointsDevice(queries, zeros)
    a.closestPointsDevice(queries)
    a.closestPointsDevice(many)
    torch.cuda.synchronize()
    assert device_bytes(a) == d1
    assert a.saveState() == state == twin.saveState()
    before = cast_rays(c, o, d, bodies=np.zeros(len(o), np.int32))                 # on c the ray call builds the tree ...
    d2 = device_bytes(c)
    got = ask(c, p, m, bodies=np.zeros(len(p), np.int32))                          # ... and the closest-point call reuses it
    assert device_bytes(c) == d2 == d1
    assert_same(got, ask(a, p, m), "the tree of either call")
    assert_same_hits(cast_rays(c, o, d, bodies=np.zeros(len(o), np.int32)), before)
    assert_same_hits(cast_rays(a, o, d, bodies=np.zeros(len(o), np.int32)), before)   # ... and the reverse
    assert device_bytes(a) == d1
    for x in (a, twin):
        x.simulateSubsteps(10, DT, PP)
    a.closestPointsDevice(queries, zeros)
    torch.cuda.synchronize()
    assert device_bytes(a) == d1 and a.saveState() == twin.saveState()
    for x in (a, twin):
        x.simulateSubsteps(5, DT, PP)
    assert np.array_equal(a.pos.view(np.uint32), twin.pos.view(np.uint32)) and np.array_equal(a.vel.view(np.uint32), twin.vel.view(np.uint32))


def test_the_host_variant_equals_the_device_call(world):
    batch, p, m, b = world["batch"], world["p"], world["m"], world["b"]
    assert_same(batch.closestPoints(p, m, b), world["want"], "bodies")
    assert_same(batch.closestPoints(p, m), ask(batch, p, m), "whole mesh")
    assert_same(batch.closestPoints(p[:5], np.inf, b[:5]), ask(batch, p[:5], np.inf, bodies=b[:5]), "a scalar limit")
    assert len(batch.closestPoints(np.zeros((0, 3)))) == 0
    bad_p, bad_m, bad_b = p[:8].copy(), m[:8].copy(), b[:8].copy()
    bad_p[3, 1] = np.nan
    bad_m[5] = -0.5
    bad_b[6] = 3
    for args, text in (((bad_p, m[:8], b[:8]), "query 3: non-finite point"), ((p[:8], bad_m, b[:8]), "query 5: max_distance < 0"),
                       ((p[:8], m[:8], bad_b), "query 6: query_body")):
        with pytest.raises(TetSimError) as e:
            batch.closestPoints(*args)
        assert e.value.code == capi.EINVAL and text in str(e.value), str(e.value)
    assert_same(batch.closestPoints(p, m, b), world["want"], "after the refusals")
