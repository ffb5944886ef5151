"""Device-side export and import (include/tetsim.h: tetsim_export_device / tetsim_import_device; SoftBodyHIP.exportTensors /
importTensors): what a torch tensor receives equals the host read of the same name bit for bit -- without a synchronisation between
the step call and the export --, padded rows and guard rows keep their bytes, a tensor reused on one stream is ordered against its
earlier readers, an import leaves the state tetsim_write_state leaves, and every refused call leaves dst and the state alone.

Bodies: the two polar arithmetic modes, the lean tet record (its quaternions are recovered on the device before they leave), and the
Neo-Hookean solver as PRECISE coloured levels and as the FAST clustered schedule (the one-launch call, whose stamps live in prev.w).
Meshes, all from tests/golden: the Dragon (irregular; internal particle order; a visual mesh with triangles), lat4 (the smallest
lattice: one partial block of rows in every field; its boundary as the visual mesh) and a batch of three Dragons."""
import ctypes as C
import os

import numpy as np
import pytest
import torch

from conftest import GOLDEN, load_f32, load_mesh
from tetsim_amd import SoftBodyHIP, TetSimError, boundary_surface
from tetsim_amd import _capi as capi

pytestmark = pytest.mark.gpu
PP = dict(gravity=-9.81, friction=1000.0, density=1000.0, devCompliance=1e-5, volCompliance=0.0,
          worldBounds=[-2.5, -1.0, -2.5, 2.5, 10.0, 2.5])
WIDE = dict(PP, worldBounds=[-10.0, -1.0, -10.0, 10.0, 10.0, 10.0])
DT = (1.0 / 60.0) / 20
SENTINEL = 0x7FC0DEAD   # a NaN payload no kernel produces

KINDS = {
    "polar-precise": dict(solver="polar", precision="precise"),
    "polar-fast": dict(solver="polar", precision="fast"),
    "polar-fast-lean": dict(solver="polar", precision="fast", lean_state=True),
    "nh-precise-coloured": dict(solver="neohookean", precision="precise", order="coloured"),
    "nh-fast": dict(solver="neohookean", precision="fast", order="clustered"),
}
MESHES = ["dragon", "lat4", "dragon3"]


def make_body(mesh, kind, visual=True):
    """(body, physicsParams).  Polar bodies get seeded rest normals, so that visNormals exists."""
    kw = KINDS[kind]
    pp = PP
    if mesh == "dragon3":
        v, t = load_mesh("dragon")
        vis1 = load_f32("dragon_vis.f32").reshape(-1, 4)
        tris1 = np.fromfile(os.path.join(GOLDEN, "dragon_vistris.u16"), dtype="<u2").astype(np.int32).reshape(-1, 3)
        shifts = [np.array([-3.0, 0.0, 0.0], np.float32), np.array([0.0, 0.0, 0.0], np.float32), np.array([3.0, 0.0, 0.5], np.float32)]
        pp = WIDE
        body = SoftBodyHIP.batch([((v + s).astype(np.float32), t) for s in shifts], dict(pp), ref_fixed_bounds=False, **kw)
        vis = np.concatenate([vis1 + np.array([b * len(t), 0, 0, 0], np.float32) for b in range(3)])
        tris = np.concatenate([tris1 + b * len(vis1) for b in range(3)])
    else:
        v, t = load_mesh(mesh)
        body = SoftBodyHIP(v, t, None, dict(pp), **kw)
        if mesh == "dragon":
            vis = load_f32("dragon_vis.f32").reshape(-1, 4)
            tris = np.fromfile(os.path.join(GOLDEN, "dragon_vistris.u16"), dtype="<u2").astype(np.int32).reshape(-1, 3)
        else:
            vis, tris = boundary_surface(t, len(v), v)
    if visual:
        n0 = None
        if kw["solver"] == "polar":
            n0 = np.random.default_rng(7).standard_normal((len(vis), 3)).astype(np.float32)
            n0 /= np.linalg.norm(n0, axis=1, keepdims=True)
        body.setVisualMesh(vis, n0)
        body.setVisualTriangles(tris)
    return body, pp


def fields_of(body):
    if body.solver == "polar":
        return ("pos", "vel", "quats", "visPos", "visNormals", "visVertexNormals")
    return ("pos", "vel", "prevPos", "visPos", "visVertexNormals")


def host_read(body, name):
    if name in ("visPos", "visNormals"):
        if body.solver != "polar":
            return body.visualPositions()
        return body.visualPositions(with_normals=True)[0 if name == "visPos" else 1]
    return {"pos": lambda: body.pos, "vel": lambda: body.vel, "prevPos": lambda: body.prevPos, "quats": lambda: body.quats,
            "visVertexNormals": body.visualVertexNormals}[name]()


def bits(a):
    if isinstance(a, torch.Tensor):
        a = a.cpu().numpy()
    return np.ascontiguousarray(a, dtype=np.float32).view(np.uint32)


def sentinel_rows(rows, width):
    """[rows, width] floats that all hold the sentinel's bits."""
    return torch.full((rows, width), SENTINEL, dtype=torch.int32, device="cuda").view(torch.float32)


def is_sentinel(t):
    return bool((t.contiguous().view(torch.int32) == SENTINEL).all())


@pytest.mark.parametrize("kind", list(KINDS))
@pytest.mark.parametrize("mesh", MESHES)
def test_export_equals_the_host_reads(mesh, kind):
    """20 substeps, then -- with no synchronisation in between -- every field the body has in ONE call; and one per call."""
    body, pp = make_body(mesh, kind)
    names = fields_of(body)
    body.simulateSubsteps(20, DT, pp)
    out = body.exportTensors(names)
    torch.cuda.synchronize()
    assert list(out) == list(names)
    want = {n: host_read(body, n) for n in names}
    for n in names:
        t = out[n]
        assert t.dtype == torch.float32 and t.is_cuda and tuple(t.shape) == want[n].shape, n
        assert want[n].shape[0] > 0 and np.isfinite(want[n]).all(), n
        assert np.array_equal(bits(t), bits(want[n])), n
    assert body.exportTensors(names)["pos"] is out["pos"]                       # allocated once, reused
    for n in names:
        fresh = sentinel_rows(*want[n].shape)
        got = body.exportTensors((n,), out={n: fresh})
        torch.cuda.synchronize()
        assert got[n] is fresh and np.array_equal(bits(fresh), bits(out[n])), n


@pytest.mark.parametrize("stride", [16, 32])
@pytest.mark.parametrize("mesh,kind", [("dragon", "polar-fast"), ("lat4", "polar-precise"), ("dragon", "nh-fast"), ("lat4", "nh-precise-coloured")])
def test_strided_rows_leave_padding_and_guard_rows_alone(mesh, kind, stride):
    body, pp = make_body(mesh, kind, visual=False)
    body.simulateSubsteps(20, DT, pp)
    n, w = body.info.owned_particles, stride // 4
    buf = sentinel_rows(n + 2, w)                                                # one guard row in front, one behind
    view = buf[1:-1, :3]
    assert view.stride(0) * 4 == stride and view.data_ptr() == buf.data_ptr() + stride
    packed = body.exportTensors(("pos",))["pos"]
    body.exportTensors(("pos",), out={"pos": view})
    torch.cuda.synchronize()
    assert np.array_equal(bits(view), bits(packed)) and np.array_equal(bits(packed), bits(body.pos))
    assert is_sentinel(buf[0]) and is_sentinel(buf[-1])
    assert is_sentinel(buf[1:-1, 3:])
    if body.solver == "polar":                                                   # four floats per row, 20 bytes apart
        nt = body.info.local_elems
        qbuf = sentinel_rows(nt + 2, 5)
        body.exportTensors(("quats",), out={"quats": qbuf[1:-1, :4]})
        torch.cuda.synchronize()
        assert np.array_equal(bits(qbuf[1:-1, :4]), bits(body.quats))
        assert is_sentinel(qbuf[0]) and is_sentinel(qbuf[-1]) and is_sentinel(qbuf[1:-1, 4:])


@pytest.mark.parametrize("side_stream", [False, True], ids=["default-stream", "side-stream"])
@pytest.mark.parametrize("kind", ["polar-fast", "nh-fast"])
def test_a_reused_tensor_is_ordered_on_its_stream(kind, side_stream):
    """export, clone, step, export into the same tensor -- one synchronisation at the end.  The references come from a twin body."""
    body, pp = make_body("dragon", kind, visual=False)
    twin, _ = make_body("dragon", kind, visual=False)
    twin.simulateSubsteps(20, DT, pp)
    first = twin.pos
    twin.simulateSubsteps(20, DT, pp)
    second = twin.pos
    assert not np.array_equal(bits(first), bits(second))
    stream = torch.cuda.Stream() if side_stream else torch.cuda.current_stream()
    with torch.cuda.stream(stream):
        body.simulateSubsteps(20, DT, pp)
        t = body.exportTensors(("pos",))["pos"]
        kept = t.clone()
        body.simulateSubsteps(20, DT, pp)
        t2 = body.exportTensors(("pos",), stream=stream if side_stream else None)["pos"]
    torch.cuda.synchronize()
    assert t2 is t
    assert np.array_equal(bits(kept), bits(first))
    assert np.array_equal(bits(t), bits(second))


def seeded_state(body, seed):
    rng = np.random.default_rng(seed)
    pos = (body.pos + rng.normal(0.0, 0.003, (body.info.owned_particles, 3)) + [0.0, 0.25, 0.0]).astype(np.float32)
    vel = rng.normal(0.0, 0.2, pos.shape).astype(np.float32)
    return pos, vel


@pytest.mark.parametrize("strided", [False, True], ids=["packed", "strided"])
@pytest.mark.parametrize("kind", list(KINDS))
@pytest.mark.parametrize("mesh", ["dragon", "lat4"])
def test_import_equals_write_state(mesh, kind, strided):
    a, pp = make_body(mesh, kind, visual=False)
    b, _ = make_body(mesh, kind, visual=False)
    for x in (a, b):
        x.simulateSubsteps(5, DT, pp)                                            # (not a pristine state: velocities, a prediction made for DT)
    pos, vel = seeded_state(a, 3)
    a.writeState(pos, vel)
    if strided:
        tp, tv = sentinel_rows(len(pos), 4), sentinel_rows(len(pos), 8)
        tp[:, :3] = torch.from_numpy(pos).cuda()
        tv[:, :3] = torch.from_numpy(vel).cuda()
        b.importTensors(tp[:, :3], tv[:, :3])
    else:
        b.importTensors(torch.from_numpy(pos).cuda(), torch.from_numpy(vel).cuda())
    assert np.array_equal(bits(a.pos), bits(b.pos)) and np.array_equal(bits(a.vel), bits(b.vel))
    assert np.array_equal(bits(b.pos), bits(pos)) and np.array_equal(bits(b.vel), bits(vel))
    for x in (a, b):
        x.simulateSubsteps(20, DT, pp)
    assert np.array_equal(bits(a.pos), bits(b.pos))
    assert np.array_equal(bits(a.vel), bits(b.vel))
    assert not np.array_equal(bits(a.pos), bits(pos))
    if a.solver == "polar":
        assert np.array_equal(bits(a.quats), bits(b.quats))


@pytest.mark.parametrize("kind", ["nh-precise-coloured", "nh-fast"])
@pytest.mark.parametrize("mesh", ["dragon", "lat4"])
def test_neohookean_hand_over_from_body_to_body(mesh, kind):
    """Positions and velocities are the whole Neo-Hookean state between calls: a fresh body that imports them continues as the first."""
    a, pp = make_body(mesh, kind, visual=False)
    b, _ = make_body(mesh, kind, visual=False)
    a.simulateSubsteps(20, DT, pp)
    out = a.exportTensors(("pos", "vel"))
    b.importTensors(out["pos"], out["vel"])
    for x in (a, b):
        x.simulateSubsteps(20, DT, pp)
    assert np.array_equal(bits(a.pos), bits(b.pos))
    assert np.array_equal(bits(a.vel), bits(b.vel))


def test_errors_leave_dst_and_the_state_alone():
    L = capi.lib()
    polar, pp = make_body("dragon", "polar-fast")
    nh, _ = make_body("dragon", "nh-precise-coloured")
    bare, _ = make_body("lat4", "polar-fast", visual=False)
    v, t = load_mesh("dragon")
    notris = SoftBodyHIP(v, t, None, dict(PP), load_f32("dragon_vis.f32").reshape(-1, 4), solver="neohookean")
    for x in (polar, nh, bare, notris):
        x.simulateSubsteps(20, DT, pp)
    rows = max(polar.info.owned_particles, polar.info.local_elems, polar.info.num_vis_verts)
    dst = sentinel_rows(rows, 4)
    dst2 = sentinel_rows(rows, 4)
    F = capi.TetSimDeviceField

    def export(body, fields, count=None, code=capi.EINVAL, text=""):
        arr = (F * max(1, len(fields)))(*fields)
        rc = L.tetsim_export_device(body._h, arr if fields else None, len(fields) if count is None else count, None)
        assert rc == code, (rc, code, L.tetsim_last_error(body._h))
        assert text.encode() in L.tetsim_last_error(body._h), L.tetsim_last_error(body._h)
        torch.cuda.synchronize()
        assert is_sentinel(dst) and is_sentinel(dst2)

    p = dst.data_ptr()
    ok = F(capi.FIELD_POSITIONS, 0, p, 0)
    export(polar, [], count=1, text="fields is null")
    export(polar, [ok], count=0, text="count")
    export(polar, [ok] * 9, text="count")
    export(polar, [F(capi.FIELD_POSITIONS, 0, None, 0)], text="dst is null")
    export(polar, [F(7, 0, p, 0)], text="unknown field")
    export(polar, [F(-1, 0, p, 0)], text="unknown field")
    export(polar, [F(capi.FIELD_POSITIONS, 1, p, 0)], text="reserved")
    export(polar, [F(capi.FIELD_POSITIONS, 0, p, 8)], text="row_stride")
    export(polar, [F(capi.FIELD_POSITIONS, 0, p, 14)], text="row_stride")
    export(polar, [F(capi.FIELD_QUATS, 0, p, 12)], text="row_stride")
    export(polar, [F(capi.FIELD_POSITIONS, 0, p + 2, 0)], text="aligned")
    export(polar, [F(capi.FIELD_VELOCITIES, 0, dst2.data_ptr(), 16), F(capi.FIELD_POSITIONS, 0, p, 8)], text="field 1")   # the good field in front is not written either
    export(polar, [F(capi.FIELD_PREV_POSITIONS, 0, p, 0)], code=capi.ESTATE, text="prevPos")
    export(nh, [F(capi.FIELD_QUATS, 0, p, 0)], code=capi.ESTATE, text="quaternions")
    export(nh, [F(capi.FIELD_VISUAL_NORMALS, 0, p, 0)], code=capi.ESTATE, text="normals need")
    for field in (capi.FIELD_VISUAL_POSITIONS, capi.FIELD_VISUAL_NORMALS, capi.FIELD_VISUAL_VERTEX_NORMALS):
        export(bare, [F(field, 0, p, 0)], code=capi.ESTATE, text="no visual mesh")
    export(notris, [F(capi.FIELD_VISUAL_VERTEX_NORMALS, 0, p, 0)], code=capi.ESTATE, text="no visual triangles")

    before = {x: (x.pos, x.vel) for x in (polar, nh)}
    for x in (polar, nh):
        for args, text in (((None, 0, p, 0), "null"), ((p, 0, None, 0), "null"), ((p, 8, p, 0), "stride"), ((p, 0, p, 18), "stride"), ((p + 1, 0, p, 0), "aligned"),
                           ((p, 0, p + 2, 16), "aligned")):
            assert L.tetsim_import_device(x._h, *args, None) == capi.EINVAL
            assert text.encode() in L.tetsim_last_error(x._h), L.tetsim_last_error(x._h)
        assert np.array_equal(bits(x.pos), bits(before[x][0])) and np.array_equal(bits(x.vel), bits(before[x][1]))
    with pytest.raises(ValueError):
        polar.exportTensors(("pos",), out={"pos": dst[:polar.info.owned_particles, :3].double()})
    with pytest.raises(ValueError):
        polar.importTensors(dst[:3, :3], dst[:3, :3])
    assert is_sentinel(dst) and is_sentinel(dst2)

    # ... and the next good call is right, in step with a twin that was never refused anything
    twin, _ = make_body("dragon", "polar-fast")
    twin.simulateSubsteps(20, DT, pp)
    for x in (polar, twin):
        x.simulateSubsteps(5, DT, pp)
    out = polar.exportTensors(fields_of(polar))
    torch.cuda.synchronize()
    for n in fields_of(polar):
        assert np.array_equal(bits(out[n]), bits(host_read(polar, n))), n
        assert np.array_equal(bits(out[n]), bits(host_read(twin, n))), n
    got = nh.exportTensors(("pos", "prevPos"))
    torch.cuda.synchronize()
    assert np.array_equal(bits(got["pos"]), bits(nh.pos)) and np.array_equal(bits(got["prevPos"]), bits(nh.prevPos))


def test_a_partitioned_body_is_refused():
    v, t = load_mesh("lat4")
    parts = [SoftBodyHIP(v, t, None, dict(PP), solver="polar", precision="fast", part_count=2, part_index=i) for i in range(2)]
    for part in parts:
        n = part.info.owned_particles
        dst = sentinel_rows(n, 3)
        with pytest.raises(TetSimError) as e:
            part.exportTensors(("pos",), out={"pos": dst})
        assert e.value.code == capi.ESTATE and "partitioned" in str(e.value)
        with pytest.raises(TetSimError) as e:
            part.importTensors(dst, dst)
        assert e.value.code == capi.ESTATE and "partitioned" in str(e.value)
        torch.cuda.synchronize()
        assert is_sentinel(dst)
