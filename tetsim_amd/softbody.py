"""Host-side mirror of the reference's solver objects over the C ABI (include/tetsim.h).

`SoftBodyHIP` keeps the constructor + simulate()/endFrame()/grab surface of the reference's
`SoftBody` (/root/reference/src/Softbody.js:3-298) and `SoftBodyGPU` (SoftbodyGPU.js:4-712) so the
caller's loop (main.js:79-89) is unchanged:

    body = SoftBodyHIP(vertices, tetIds, tetEdgeIds, physicsParams, visVerts, visTriIds, visMaterial, world)
    for step in range(numSubsteps): body.simulate(dt, physicsParams)
    body.endFrame()

Only the physics is here (display meshes are three.js objects of the JavaScript host; the N-API twin of this
class, tetsim_amd/node/SoftBodyHIP.js, owns those).  All compute happens in libtetsim_hip.so on the GPU.
"""
import ctypes as C

import numpy as np

from . import _capi as capi
from ._capi import TetSimError  # noqa: F401


def _f32(a):
    return np.ascontiguousarray(a, dtype=np.float32)


def _fp(a):
    return a.ctypes.data_as(C.POINTER(C.c_float))


def _ip(a):
    return a.ctypes.data_as(C.POINTER(C.c_int32))


_COLLIDER_KINDS = {"sphere": capi.COLLIDER_SPHERE, "capsule": capi.COLLIDER_CAPSULE, "box": capi.COLLIDER_BOX, "plane": capi.COLLIDER_PLANE}


def _vec(v, n=3):
    """[x, y, z] or {x, y, z} (a list of n/3 of either for n > 3) -> n floats."""
    if isinstance(v, dict):
        return [float(v["x"]), float(v["y"]), float(v["z"])]
    a = np.asarray(v, dtype=np.float64).reshape(-1) if not isinstance(v[0], dict) else np.asarray([_vec(r) for r in v], dtype=np.float64).reshape(-1)
    if a.size != n:
        raise ValueError("expected %d numbers, got %d" % (n, a.size))
    return [float(x) for x in a]


def make_colliders(colliders):
    """list of dicts -> (TetSimCollider * n).  Each dict: kind ("sphere" / "capsule" / "box" / "plane") and the fields of
    include/tetsim.h TetSimCollider that the kind uses -- a, b, axes (3 rows), radius, friction, velocity; absent ones are 0
    (axes: the world axes)."""
    arr = (capi.TetSimCollider * max(1, len(colliders)))()
    for c, d in zip(arr, colliders):
        kind = d["kind"]
        c.kind = _COLLIDER_KINDS[kind] if isinstance(kind, str) else int(kind)
        c.reserved = int(d.get("reserved", 0))
        c.a[:] = _vec(d.get("a", (0.0, 0.0, 0.0)))
        c.b[:] = _vec(d.get("b", (0.0, 0.0, 0.0)))
        c.axes[:] = _vec(d.get("axes", ((1.0, 0.0, 0.0), (0.0, 1.0, 0.0), (0.0, 0.0, 1.0))), 9)
        c.radius = float(d.get("radius", 0.0))
        c.friction = float(d.get("friction", 0.0))
        c.velocity[:] = _vec(d.get("velocity", (0.0, 0.0, 0.0)))
    return arr


def body_collider_rows(lists, per_body=None):
    """A list per body of the dicts make_colliders takes -> float32 [bodies, per_body, 24], the rows of setBodyColliders /
    setBodyCollidersDevice (include/tetsim.h: TETSIM_BODY_COLLIDER_FLOATS -- kind as a value, a, b, axes, radius, friction, velocity,
    three unread floats).  per_body: slots per body, 1 .. 8 (None = the longest list, at least 1); a body's unused slots are empty
    rows (kind -1).  torch.from_numpy(rows).to(device) is the tensor setBodyCollidersDevice reads."""
    lists = [list(cs) for cs in lists]
    longest = max([len(cs) for cs in lists] + [1])
    per_body = longest if per_body is None else int(per_body)
    if not 1 <= per_body <= capi.MAX_COLLIDERS or longest > per_body:
        raise ValueError("per_body must be 1 .. %d and hold the longest list (%d)" % (capi.MAX_COLLIDERS, longest))
    rows = np.zeros((len(lists), per_body, capi.BODY_COLLIDER_FLOATS), dtype=np.float32)
    rows[:, :, 0] = -1.0
    for b, cs in enumerate(lists):
        for k, c in enumerate(make_colliders(cs)[:len(cs)]):
            if c.reserved != 0:
                raise ValueError("body %d, slot %d: a row has no `reserved` field" % (b, k))
            rows[b, k, :21] = [c.kind] + list(c.a) + list(c.b) + list(c.axes) + [c.radius, c.friction] + list(c.velocity)
    return rows


BODY_PARAM_FIELDS = ("gravity", "friction", "devCompliance", "volCompliance")   # then worldBounds: lo xyz, hi xyz


def body_param_rows(bodies, defaults):
    """A dict per body with the keys of physicsParams (gravity, friction, devCompliance, volCompliance, worldBounds), or None -> float64
    [bodies, 10], the rows of setBodyParams / setBodyParamsDevice (include/tetsim.h: TETSIM_BODY_PARAMS_WIDTH -- the fields of
    TetSimParams in its order).  A None entry, and a key a dict leaves out, come from `defaults`, a dict with all five keys.
    torch.from_numpy(rows).to(device) is the tensor setBodyParamsDevice reads."""
    rows = np.empty((len(bodies), capi.BODY_PARAMS_WIDTH), dtype=np.float64)
    for b, d in enumerate(bodies):
        d = dict(defaults, **(d or {}))
        rows[b, :4] = [float(d[k]) for k in BODY_PARAM_FIELDS]
        rows[b, 4:] = _vec(d["worldBounds"], 6)
    return rows


# tetsim_raycast_visual's records as numpy sees them (include/tetsim.h: TetSimRay, TetSimRayHit)
RAY_DTYPE = np.dtype([("origin", "<f8", (3,)), ("direction", "<f8", (3,)), ("near", "<f8"), ("far", "<f8")])
RAY_HIT_DTYPE = np.dtype([("hit", "<i4"), ("body", "<i4"), ("triangle", "<i4"), ("reserved", "<i4"), ("distance", "<f8"), ("point", "<f8", (3,))])


def make_rays(origins, directions, near=0.0, far=np.inf):
    """[n, 3] origins and directions (one of them may be a single vector), near / far scalars or [n] -> TetSimRay records."""
    o, d = np.asarray(origins, dtype=np.float64).reshape(-1, 3), np.asarray(directions, dtype=np.float64).reshape(-1, 3)
    n = max(len(o), len(d))
    rays = np.empty(n, dtype=RAY_DTYPE)
    rays["origin"], rays["direction"], rays["near"], rays["far"] = o, d, near, far
    return rays


def rays_tensor(origins, directions, near=0.0, far=np.inf, device="cuda"):
    """make_rays on a torch device: the float64 [count, 8] tensor raycastVisualDevice reads (columns: origin xyz, direction xyz,
    near, far -- a TetSimRay per row)."""
    import torch
    rays = make_rays(origins, directions, near, far)
    return torch.from_numpy(rays.view(np.float64).reshape(-1, 8).copy()).to(device)


# tetsim_closest_visual's records as numpy sees them (include/tetsim.h: TetSimPointQuery, TetSimClosest)
POINT_QUERY_DTYPE = np.dtype([("point", "<f8", (3,)), ("max_distance", "<f8")])
CLOSEST_DTYPE = np.dtype([("found", "<i4"), ("body", "<i4"), ("triangle", "<i4"), ("region", "<i4"), ("distance", "<f8"), ("point", "<f8", (3,)),
                          ("v", "<f8"), ("w", "<f8")])


def make_point_queries(points, max_distance=np.inf):
    """[n, 3] points, max_distance a scalar or [n] -> TetSimPointQuery records."""
    p = np.asarray(points, dtype=np.float64).reshape(-1, 3)
    queries = np.empty(len(p), dtype=POINT_QUERY_DTYPE)
    queries["point"], queries["max_distance"] = p, max_distance
    return queries


def point_queries_tensor(points, max_distance=np.inf, device="cuda"):
    """make_point_queries on a torch device: the float64 [count, 4] tensor closestPointsDevice reads (columns: point xyz, max_distance --
    a TetSimPointQuery per row)."""
    import torch
    queries = make_point_queries(points, max_distance)
    return torch.from_numpy(queries.view(np.float64).reshape(-1, 4).copy()).to(device)


def place_rows(q, pivot=(0.0, 0.0, 0.0), offset=(0.0, 0.0, 0.0), linear=(0.0, 0.0, 0.0), angular=(0.0, 0.0, 0.0)):
    """float32 [bodies, 16] rows of placeBodies / placeBodiesDevice (include/tetsim.h: TETSIM_PLACE_*): q [bodies, 4] xyzw (any length
    but 0), pivot, offset, linear, angular [bodies, 3] -- each of them may be a single vector for all bodies.  torch.from_numpy(rows)
    .to(device) is the tensor placeBodiesDevice reads."""
    q = np.asarray(q, dtype=np.float32).reshape(-1, 4)
    parts = [np.asarray(a, dtype=np.float32).reshape(-1, 3) for a in (pivot, offset, linear, angular)]
    n = max([len(q)] + [len(a) for a in parts])
    rows = np.empty((n, capi.PLACE_WIDTH), dtype=np.float32)
    rows[:, capi.PLACE_Q:capi.PLACE_Q + 4] = q
    for at, a in zip((capi.PLACE_PIVOT, capi.PLACE_OFFSET, capi.PLACE_LINEAR, capi.PLACE_ANGULAR), parts):
        rows[:, at:at + 3] = a
    return rows


def prep_pin_slots(particles, targets, body_particles):
    """The pin table's normalisation on the host (include/tetsim.h: tetsim_prep_pin_slots): particles int [B, K] (index inside the body,
    -1 = unused), targets float [B, K, 3], body_particles [B] particles of every body.  Returns int32 [sum(body_particles)]: for every
    particle, in body order, the row b * K + k that holds it, -1 = free -- a row outside its body or with a non-finite target holds
    nothing, the lowest row wins a particle that several name."""
    p = np.ascontiguousarray(particles, dtype=np.int32)
    t = _f32(targets)
    n = np.ascontiguousarray(body_particles, dtype=np.uint32).reshape(-1)
    if p.ndim != 2 or p.shape[0] != len(n) or p.shape[1] < 1 or t.shape != p.shape + (3,):
        raise ValueError("particles must be [%d, per_body >= 1] and targets [%d, per_body, 3]" % (len(n), len(n)))
    out = np.empty(int(n.sum(dtype=np.uint64)), dtype=np.int32)
    capi.check(capi.lib().tetsim_prep_pin_slots(_ip(p.reshape(-1)), _fp(t.reshape(-1)), len(n), p.shape[1], n.ctypes.data_as(C.POINTER(C.c_uint32)), _ip(out)))
    return out


def boundary_surface(tets, nv, verts=None):
    """(visVerts [rows, 4], visTriIds [triangles, 3]) of the tet mesh's boundary, oriented outward, in the reference's visual-mesh
    format -- for bodies without an artist's mesh (include/tetsim.h: tetsim_prep_boundary_surface).  Host only, no GPU needed.
    verts: rest positions, to orient tets of either handedness; None takes every tet as positively oriented."""
    L = capi.lib()
    t = np.ascontiguousarray(np.asarray(tets).reshape(-1), dtype=np.int32)
    v = None if verts is None else _f32(verts).reshape(-1)
    nr, ntri = C.c_uint32(), C.c_uint32()
    args = (_fp(v) if v is not None else None, _ip(t), t.size // 4, int(nv))
    capi.check(L.tetsim_prep_boundary_surface(*args, None, None, C.byref(nr), C.byref(ntri)))
    vis, tri = np.empty(4 * nr.value, dtype=np.float32), np.empty(3 * ntri.value, dtype=np.int32)
    capi.check(L.tetsim_prep_boundary_surface(*args, _fp(vis), _ip(tri), C.byref(nr), C.byref(ntri)))
    return vis.reshape(-1, 4), tri.reshape(-1, 3)


def make_params(physicsParams):
    """physicsParams object (main.js:22-36) -> TetSimParams."""
    p = capi.TetSimParams()
    capi.lib().tetsim_default_params(C.byref(p))
    g = physicsParams.get if isinstance(physicsParams, dict) else (lambda k, d=None: getattr(physicsParams, k, d))
    for k in ("gravity", "friction", "devCompliance", "volCompliance"):
        v = g(k, None)
        if v is not None:
            setattr(p, k, float(v))
    wb = g("worldBounds", None)
    if wb is not None:
        for i in range(6):
            p.worldBounds[i] = float(wb[i])
    return p


# exportTensors: name -> (TETSIM_FIELD_*, the TetSimInfo count of its rows, floats per row)
_EXPORT_FIELDS = {"pos": (capi.FIELD_POSITIONS, "owned_particles", 3), "vel": (capi.FIELD_VELOCITIES, "owned_particles", 3),
                  "prevPos": (capi.FIELD_PREV_POSITIONS, "owned_particles", 3), "quats": (capi.FIELD_QUATS, "local_elems", 4),
                  "visPos": (capi.FIELD_VISUAL_POSITIONS, "num_vis_verts", 3), "visNormals": (capi.FIELD_VISUAL_NORMALS, "num_vis_verts", 3),
                  "visVertexNormals": (capi.FIELD_VISUAL_VERTEX_NORMALS, "num_vis_verts", 3)}


# names of the channels of a tet's strain row (visualStrainDevice): F<row><column> is stored column-major
_STRAIN_CHANNELS = dict({"F%d%d" % (i, j): capi.STRAIN_F + 3 * j + i for i in range(3) for j in range(3)}, J=capi.STRAIN_J, dev=capi.STRAIN_DEV,
                        stretch0=capi.STRAIN_STRETCH, stretch1=capi.STRAIN_STRETCH + 1, stretch2=capi.STRAIN_STRETCH + 2, green=capi.STRAIN_GREEN)


def _check_rows(torch, t, dev, n, width, name):
    """A tensor the device hand-over may read or write: float32 [n, width] on dev, every row contiguous, rows not overlapping."""
    if (not isinstance(t, torch.Tensor) or t.dtype != torch.float32 or t.device != dev or tuple(t.shape) != (n, width)
            or (n and t.stride(1) != 1) or (n > 1 and t.stride(0) < width)):
        raise ValueError("%s must be a float32 tensor on %s of shape (%d, %d) with contiguous, non-overlapping rows" % (name, dev, n, width))


class Snapshot:
    """The complete solver state of one SoftBodyHIP in device memory (include/tetsim.h: tetsim_snapshot_*): made by body.snapshot(),
    refreshed by body.capture(snap, ...), written back by body.restore(snap, ...).  close() frees it; the body's close() frees the
    snapshots that are left."""

    def __init__(self, body, handle):
        self._body, self._s = body, handle

    def close(self):
        if self._s is not None and getattr(self._body, "_h", None):
            self._body._L.tetsim_snapshot_destroy(self._s)
            self._body._snapshots.remove(self)
        self._s = None

    def __del__(self):
        try:
            self.close()
        except Exception:
            pass


class SoftBodyHIP:
    """Drop-in for `new SoftBody(...)` / `new SoftBodyGPU(...)`; `solver` picks which one is mirrored.

    solver="polar"  -> SoftBodyGPU's shape-matching Jacobi (default, like the reference's GPU path)
    solver="neohookean" -> SoftBody's Neo-Hookean XPBD Gauss-Seidel
    """

    def __init__(self, vertices, tetIds, tetEdgeIds=None, physicsParams=None, visVerts=None, visTriIds=None,
                 visMaterial=None, world=None, *, solver="polar", precision="precise", order="original",
                 ref_slot_table=True, ref_fixed_bounds=True, gather=False, constant_rest_shape=False, ref_grab_texel=False, deep_ghosts=False, ref_rotation_exit=False,
                 lean_state=False,
                 device=0, part_count=1, part_index=0, vert_owner=None, tet_colour=None, mesh_file=None, batch=None):
        L = capi.lib()
        self.physicsParams = physicsParams if physicsParams is not None else {}
        self._batch = None
        if batch is not None:   # SoftBodyHIP.batch: several independent bodies behind one handle (tetsim_create_batch)
            self._batch = [(_f32(v).reshape(-1), np.ascontiguousarray(np.asarray(t).reshape(-1), dtype=np.int32)) for v, t in batch]
            offs = np.concatenate([[0], np.cumsum([len(v) // 3 for v, _ in self._batch])])
            vertices = np.concatenate([v for v, _ in self._batch])
            tetIds = np.concatenate([t + int(offs[i]) for i, (_, t) in enumerate(self._batch)])
        if mesh_file is not None:   # SoftBodyHIP.fromFile: arrays come from the .tetsim container
            from .meshfile import MeshFile
            with MeshFile(mesh_file) as mf:
                vertices, tetIds = mf.verts.copy(), mf.tets.copy()
                if visVerts is None and mf.vis_verts is not None:
                    visVerts = mf.vis_verts.copy()
                    if visTriIds is None and mf.vis_tri_ids is not None:
                        visTriIds = mf.vis_tri_ids.copy()
        self._verts = _f32(vertices).reshape(-1)
        self._tets = np.ascontiguousarray(np.asarray(tetIds).reshape(-1), dtype=np.int32)
        if self._verts.size % 3 or self._tets.size % 4:
            raise ValueError("vertices must hold 3 floats per particle and tetIds 4 ids per tet")
        self.numParticles = self._verts.size // 3   # Softbody.js:9
        self.numElems = self._tets.size // 4        # Softbody.js:10
        self.visVerts = visVerts
        self.grabId = -1
        self.grabPos = np.zeros(3, dtype=np.float32)
        o = capi.TetSimOptions()
        L.tetsim_default_options(C.byref(o))
        o.solver = {"polar": capi.SOLVER_POLAR_JACOBI, "neohookean": capi.SOLVER_NEOHOOKEAN_GS}[solver]
        o.precision = {"precise": capi.PRECISE, "fast": capi.FAST}[precision]
        o.order = {"original": capi.ORDER_ORIGINAL, "coloured": capi.ORDER_COLOURED, "clustered": capi.ORDER_CLUSTERED}[order]
        o.flags = ((capi.FLAG_REF_SLOT_TABLE if ref_slot_table else 0) | (capi.FLAG_REF_FIXED_BOUNDS if ref_fixed_bounds else 0)
                   | (capi.FLAG_GATHER_FORMULATION if gather else 0)
                   | (capi.FLAG_CONSTANT_REST_SHAPE if constant_rest_shape else 0)
                   | (capi.FLAG_REF_GRAB_TEXEL if ref_grab_texel else 0) | (capi.FLAG_DEEP_GHOSTS if deep_ghosts else 0)
                   | (capi.FLAG_REF_ROTATION_EXIT if ref_rotation_exit else 0) | (capi.FLAG_LEAN_STATE if lean_state else 0))
        o.device = device
        d = self.physicsParams.get("density", 1000.0) if isinstance(self.physicsParams, dict) else getattr(self.physicsParams, "density", 1000.0)
        o.density = float(d)
        o.part_count, o.part_index = part_count, part_index
        self._owner = None
        if vert_owner is not None:
            self._owner = np.ascontiguousarray(vert_owner, dtype=np.int32)
            o.vert_owner = _ip(self._owner)
        self._colour = None
        if tet_colour is not None:
            self._colour = np.ascontiguousarray(tet_colour, dtype=np.int32)
            if self._colour.size != self.numElems:
                raise ValueError("tet_colour needs one entry per tet")
            o.tet_colour = _ip(self._colour)
        self.solver = solver
        self._h = C.c_void_p()
        if mesh_file is not None:   # the library maps the file itself and picks up a stored colouring / partition map
            capi.check(L.tetsim_create_from_file(str(mesh_file).encode(), C.byref(o), C.byref(self._h)))
        elif self._batch is not None:
            n = len(self._batch)
            vp = (C.POINTER(C.c_float) * n)(*[_fp(v) for v, _ in self._batch])
            tp = (C.POINTER(C.c_int32) * n)(*[_ip(t) for _, t in self._batch])
            nvs = (C.c_uint32 * n)(*[len(v) // 3 for v, _ in self._batch])
            nts = (C.c_uint32 * n)(*[len(t) // 4 for _, t in self._batch])
            capi.check(L.tetsim_create_batch(vp, nvs, tp, nts, n, C.byref(o), C.byref(self._h)))
        else:
            capi.check(L.tetsim_create(_fp(self._verts), self.numParticles, _ip(self._tets), self.numElems,
                                       C.byref(o), C.byref(self._h)))
        self.info = capi.TetSimInfo()
        capi.check(L.tetsim_get_info(self._h, C.byref(self.info)), self._h)
        self._L = L
        self._export_cache = {}   # exportTensors: name -> the tensor it allocated
        self._snapshots = []      # the live Snapshot objects of this handle
        self.numVisVerts = 0
        if visVerts is not None and len(visVerts):   # Softbody.js:46-47: rows (tetNr, b0, b1, b2); a partition keeps the rows of the tets it owns (visualIds)
            if mesh_file is not None:   # tetsim_create_from_file attached the stored visual mesh already
                self.numVisVerts, self._has_normals = self.info.num_vis_verts, False
            else:
                self.setVisualMesh(visVerts)
            if visTriIds is not None and len(visTriIds) and part_count <= 1:   # Softbody.js:48-50: enables visualVertexNormals() (unpartitioned bodies)
                self.setVisualTriangles(visTriIds)

    @classmethod
    def batch(cls, bodies, physicsParams=None, **kw):
        """Several INDEPENDENT bodies `[(vertices, tetIds), ...]` behind one handle: one launch per kernel steps them all (the
        reference steps softBodies[] one after the other, main.js:80-84).  `.pos` etc. are the concatenation; `bodyRanges` gives
        each body's particle / tet range.  Every body's results equal its solo run bit for bit."""
        return cls(None, None, None, physicsParams, batch=list(bodies), **kw)

    @property
    def bodyRanges(self):
        n = self.info.num_bodies
        fp_, fe = (C.c_uint32 * (n + 1))(), (C.c_uint32 * (n + 1))()
        capi.check(self._L.tetsim_get_batch_layout(self._h, fp_, fe), self._h)
        return [((fp_[b], fp_[b + 1]), (fe[b], fe[b + 1])) for b in range(n)]

    @classmethod
    def fromFile(cls, path, physicsParams=None, visMaterial=None, world=None, **kw):
        """Build the body from a .tetsim container (tetsim_amd/meshfile.py) instead of the five Dragon.js arrays."""
        return cls(None, None, None, physicsParams, None, None, visMaterial, world, mesh_file=path, **kw)

    # -- lifecycle ------------------------------------------------------------------------------------
    def close(self):
        if getattr(self, "_h", None):
            for snap in getattr(self, "_snapshots", ()):   # (tetsim_destroy frees them with the handle)
                snap._s = None
            self._snapshots = []
            self._L.tetsim_destroy(self._h)
            self._h = None

    def __del__(self):
        try:
            self.close()
        except Exception:
            pass

    # -- the hot path ---------------------------------------------------------------------------------
    def simulate(self, dt, physicsParams=None):
        """One substep (Softbody.js:195 / SoftbodyGPU.js:610).  Asynchronous."""
        pp = self.physicsParams if physicsParams is None else physicsParams
        if isinstance(pp, dict) and self.solver == "polar":
            pp["dt"] = dt  # SoftbodyGPU.js:611 writes dt back into the caller's object
        capi.check(self._L.tetsim_step(self._h, float(dt), C.byref(make_params(pp))), self._h)

    def simulateSubsteps(self, n, dt, physicsParams=None):
        """The caller's whole substep loop (main.js:79-84) as ONE FFI crossing / one HIP-graph launch."""
        pp = self.physicsParams if physicsParams is None else physicsParams
        capi.check(self._L.tetsim_step_n(self._h, int(n), float(dt), C.byref(make_params(pp))), self._h)

    def endFrame(self):
        """Softbody.js:244-247 refreshes the display meshes from .pos; here: make the frame's results visible."""
        capi.check(self._L.tetsim_sync(self._h), self._h)

    def sync(self):
        capi.check(self._L.tetsim_sync(self._h), self._h)

    # -- state ----------------------------------------------------------------------------------------
    def _read3(self, fn, n):
        out = np.empty(3 * n, dtype=np.float32)
        capi.check(fn(self._h, _fp(out)), self._h)
        return out.reshape(-1, 3)

    @property
    def pos(self):
        return self._read3(self._L.tetsim_read_positions, self.info.owned_particles)

    @property
    def posPinned(self):
        """Zero-copy read-back: a numpy VIEW of the handle's pinned host buffer (valid until close(), refreshed by every
        access): one device pack kernel + one DMA, no intermediate host copy."""
        ptr = C.POINTER(C.c_float)()
        capi.check(self._L.tetsim_read_positions_pinned(self._h, C.byref(ptr)), self._h)
        return np.ctypeslib.as_array(ptr, shape=(self.info.owned_particles, 3))

    @property
    def prevPos(self):
        return self._read3(self._L.tetsim_read_prev_positions, self.info.owned_particles)

    @property
    def vel(self):
        return self._read3(self._L.tetsim_read_velocities, self.info.owned_particles)

    @property
    def quats(self):
        out = np.empty(4 * self.info.local_elems, dtype=np.float32)
        capi.check(self._L.tetsim_read_quats(self._h, _fp(out)), self._h)
        return out.reshape(-1, 4)

    @property
    def quatsPinned(self):
        """Zero-copy twin of `quats`: a numpy VIEW of the handle's pinned host buffer, refreshed by every access."""
        ptr = C.POINTER(C.c_float)()
        capi.check(self._L.tetsim_read_quats_pinned(self._h, C.byref(ptr)), self._h)
        return np.ctypeslib.as_array(ptr, shape=(self.info.local_elems, 4))

    def saveState(self):
        """The complete solver state (positions, velocities, per-tet quaternions and carried rest shape) as bytes."""
        n = C.c_uint64()
        capi.check(self._L.tetsim_state_size(self._h, C.byref(n)), self._h)
        buf = (C.c_char * n.value)()
        capi.check(self._L.tetsim_save_state(self._h, buf, n.value), self._h)
        return bytes(buf.raw)

    def loadState(self, blob):
        """Resume from saveState() of a body with the same mesh and options: the trajectory continues bit for bit."""
        capi.check(self._L.tetsim_load_state(self._h, bytes(blob), len(blob)), self._h)

    @property
    def volError(self):
        v = C.c_double()
        capi.check(self._L.tetsim_read_vol_error(self._h, C.byref(v)), self._h)
        return v.value

    @property
    def invMass(self):
        out = np.empty(self.numParticles, dtype=np.float32)
        capi.check(self._L.tetsim_read_inv_mass(self._h, _fp(out)), self._h)
        return out

    @property
    def ownedIds(self):
        out = np.empty(self.info.owned_particles, dtype=np.int32)
        capi.check(self._L.tetsim_get_owned_ids(self._h, _ip(out)), self._h)
        return out

    @property
    def localTets(self):
        out = np.empty(self.info.local_elems, dtype=np.int32)
        capi.check(self._L.tetsim_get_local_tets(self._h, _ip(out)), self._h)
        return out

    @property
    def tetOrder(self):
        out = np.empty(self.numElems, dtype=np.int32)
        capi.check(self._L.tetsim_get_tet_order(self._h, _ip(out)), self._h)
        return out

    @property
    def levelOffsets(self):
        out = np.empty(self.info.num_levels + 1, dtype=np.int32)
        capi.check(self._L.tetsim_get_level_offsets(self._h, _ip(out)), self._h)
        return out

    def writeState(self, pos, vel):
        p, v = _f32(pos).reshape(-1), _f32(vel).reshape(-1)
        capi.check(self._L.tetsim_write_state(self._h, _fp(p), _fp(v)), self._h)

    # -- device-side hand-over to PyTorch (include/tetsim.h: tetsim_export_device / tetsim_import_device) -----------
    def _torch_stream(self, torch, stream):
        dev = torch.device("cuda", self.info.device)
        if stream is None:
            return dev, torch.cuda.current_stream(dev).cuda_stream
        return dev, int(getattr(stream, "cuda_stream", stream))

    def _out_rows(self, torch, dev, key, out, shape, dtype, name="out", align=None, packed=False):
        """Where a device-side call writes: the tensor cached under `key` (allocated once; anew when its first dimension changed), or the
        caller's `out` behind the checks -- dtype, device, shape (rows,) or (rows, width); rows contiguous and not overlapping, the row
        stride free unless `packed`; align: rows and row stride multiples of that many bytes."""
        n = shape[0]
        if out is None:
            out = self._export_cache.get(key)
            if out is None or out.shape[0] != n:
                out = self._export_cache[key] = torch.empty(shape, dtype=dtype, device=dev)
            return out
        ok = isinstance(out, torch.Tensor) and out.dtype == dtype and out.device == dev and tuple(out.shape) == tuple(shape)
        if ok and len(shape) == 2:
            ok = not (n and out.stride(1) != 1) and not (n > 1 and out.stride(0) < shape[1])
        if ok:
            ok = not (n > 1 and out.stride(0) < 1) and not (packed and not out.is_contiguous())
        if ok and align:
            ok = not (n > 1 and out.stride(0) * out.element_size() % align) and not (n and out.data_ptr() % align)
        if not ok:
            raise ValueError("%s must be a %s tensor on %s of shape %s with contiguous, non-overlapping%s rows"
                             % (name, dtype, dev, tuple(shape), ", %d-byte aligned" % align if align else ""))
        return out

    def exportTensors(self, fields=("pos",), out=None, stream=None):
        """{name: torch.Tensor} of the named fields (_EXPORT_FIELDS: pos, vel, prevPos, quats, visPos, visNormals, visVertexNormals) on
        the handle's device, float32 [rows, 3] ([rows, 4] for quats), bit for bit what the host read of the same name returns -- without
        a host copy and without synchronising: the tensors are valid for work enqueued on `stream` (a torch stream or a raw
        hipStream_t; None = torch's current stream of that device) after this returns.  All fields leave in one kernel launch.
        The tensors are allocated once and reused by later calls unless `out` supplies them ({name: tensor}; rows may be strided:
        the row stride is out[name].stride(0), anything between the rows is left alone)."""
        import torch
        dev, s = self._torch_stream(torch, stream)
        names = [fields] if isinstance(fields, str) else list(fields)
        arr = (capi.TetSimDeviceField * max(1, len(names)))()
        res = {}
        for f, name in zip(arr, names):
            field, rows, width = _EXPORT_FIELDS[name]
            n = int(getattr(self.info, rows))
            # (the cached tensor is made anew when num_vis_verts changed: a visual mesh was attached)
            t = self._out_rows(torch, dev, name, out.get(name) if out is not None else None, (n, width), torch.float32, "out[%r]" % name)
            f.field, f.reserved, f.dst = field, 0, t.data_ptr()
            f.row_stride = 4 * t.stride(0) if n > 1 else 0
            res[name] = t
        capi.check(self._L.tetsim_export_device(self._h, arr, len(names), s), self._h)
        return res

    def importTensors(self, pos, vel, stream=None):
        """writeState from device tensors: float32 [owned_particles, 3] on the handle's device, rows contiguous (the rows themselves may
        be strided).  No host copy, no synchronisation: the state is written behind the substeps enqueued so far once `stream` (None =
        torch's current stream) has produced the tensors, and `stream` may reuse them afterwards."""
        import torch
        dev, s = self._torch_stream(torch, stream)
        n = self.info.owned_particles
        _check_rows(torch, pos, dev, n, 3, "pos")
        _check_rows(torch, vel, dev, n, 3, "vel")
        capi.check(self._L.tetsim_import_device(self._h, pos.data_ptr(), 4 * pos.stride(0) if n > 1 else 0,
                                                vel.data_ptr(), 4 * vel.stride(0) if n > 1 else 0, s), self._h)

    # -- device snapshots (include/tetsim.h: tetsim_snapshot_*): the complete state, kept on the device, for chosen bodies ---------
    def _body_mask(self, torch, dev, bodies):
        """(address or None, the tensor to keep alive) of `bodies`: None = all; a torch.bool / torch.uint8 tensor of num_bodies on the
        body's device, used as it is; or a host sequence of truth values, copied to such a tensor (and the copy awaited)."""
        if bodies is None:
            return None, None
        n = self.info.num_bodies
        if isinstance(bodies, torch.Tensor):
            if bodies.dtype not in (torch.bool, torch.uint8) or bodies.device != dev or bodies.numel() != n or not bodies.is_contiguous():
                raise ValueError("bodies must be a contiguous torch.bool / torch.uint8 tensor of %d elements on %s" % (n, dev))
            return bodies.data_ptr(), bodies
        host = np.asarray([bool(b) for b in bodies], dtype=np.bool_)
        if host.size != n:
            raise ValueError("bodies must name every one of the %d bodies" % n)
        t = torch.from_numpy(host).to(dev)
        torch.cuda.current_stream(dev).synchronize()   # (a pageable copy: the mask is complete whatever stream the call names)
        return t.data_ptr(), t

    def snapshot(self, stream=None):
        """A Snapshot of the current state of every body, behind the substeps enqueued so far.  Allocates (may block).  `stream` is
        accepted for symmetry with capture / restore: a fresh snapshot has nothing to order against the caller."""
        s = C.c_void_p()
        capi.check(self._L.tetsim_snapshot_create(self._h, C.byref(s)), self._h)
        snap = Snapshot(self, s)
        self._snapshots.append(snap)
        return snap

    def _masked_call(self, bodies, stream, call):
        """A device-side call that takes a body mask: `stream` and `bodies` resolved (_torch_stream, _body_mask), then call(torch, dev, mask
        address or None, stream) -- which checks its own arguments and returns the library's code -- and the mask kept alive."""
        import torch
        dev, s = self._torch_stream(torch, stream)
        ptr, keep = self._body_mask(torch, dev, bodies)
        capi.check(call(torch, dev, ptr, s), self._h)
        self._mask_keep = keep   # (a converted host sequence lives until the next call: the kernel may not have read it yet)

    def _snapshot_call(self, fn, snap, bodies, stream):
        if not isinstance(snap, Snapshot) or snap._s is None:
            raise ValueError("snap must be a live Snapshot")
        self._masked_call(bodies, stream, lambda torch, dev, mask, s: fn(self._h, snap._s, mask, s))

    def capture(self, snap, bodies=None, stream=None):
        """Overwrite the chosen bodies' part of `snap` with their current state.  bodies: None = all, a torch.bool / torch.uint8 tensor
        [num_bodies] on the body's device (produced on `stream`; reusable on it right after the call), or a host sequence of truth values.
        No host copy of the state and, with a tensor, no synchronisation; `stream` as in exportTensors."""
        self._snapshot_call(self._L.tetsim_snapshot_capture, snap, bodies, stream)

    def restore(self, snap, bodies=None, stream=None):
        """Overwrite the chosen bodies' current state with their part of `snap`: with bodies=None what loadState(saveState() of the capture's
        moment) leaves, bit for bit; with a mask the other bodies are not written.  Arguments as in capture."""
        self._snapshot_call(self._L.tetsim_snapshot_restore, snap, bodies, stream)

    # -- placement (include/tetsim.h: tetsim_place_bodies / _device): a rigid motion of chosen bodies' complete state ----------------
    def placeBodiesDevice(self, rows, bodies=None, keep_velocity=False, stream=None):
        """Give every chosen body the rigid motion of its row: rows torch.float32 [num_bodies, 16] on the handle's device (place_rows;
        rows contiguous, the row stride is passed through), produced on `stream` (as in exportTensors; reusable on it right after the
        call).  Positions, velocities, predictions, quaternions and carried shapes move together (definition: include/tetsim.h), behind
        the substeps enqueued so far, with no host copy and no synchronisation.  bodies: a mask as in restore -- a body it leaves out is
        not written.  keep_velocity: the body's velocities are turned and kept under the row's linear and angular velocity.  A row
        with a non-finite value or a zero quaternion leaves its body untouched."""
        n = self.info.num_bodies

        def call(torch, dev, mask, s):
            _check_rows(torch, rows, dev, n, capi.PLACE_WIDTH, "rows")
            return self._L.tetsim_place_bodies_device(self._h, rows.data_ptr(), 4 * rows.stride(0) if n > 1 else 0, mask,
                                                      capi.PLACE_KEEP_VELOCITY if keep_velocity else 0, s)
        self._masked_call(bodies, stream, call)

    def placeBodies(self, rows, bodies=None, keep_velocity=False):
        """placeBodiesDevice from host arrays: rows float32 [num_bodies, 16] (place_rows), bodies None or a sequence of num_bodies truth
        values.  Raises TetSimError(EINVAL) for a chosen body's row with a non-finite value or a zero quaternion, and changes nothing."""
        n = self.info.num_bodies
        r = _f32(rows).reshape(-1)
        if r.size != capi.PLACE_WIDTH * n:
            raise ValueError("rows must hold %d rows of %d floats" % (n, capi.PLACE_WIDTH))
        m = None
        if bodies is not None:
            m = np.ascontiguousarray([bool(b) for b in bodies], dtype=np.uint8)
            if m.size != n:
                raise ValueError("bodies must name every one of the %d bodies" % n)
        capi.check(self._L.tetsim_place_bodies(self._h, _fp(r), m.ctypes.data_as(C.POINTER(C.c_uint8)) if m is not None else None,
                                               capi.PLACE_KEEP_VELOCITY if keep_velocity else 0), self._h)

    # -- per-body observations (include/tetsim.h: tetsim_observe_bodies_device): one row of _capi.OBS_WIDTH doubles per body -------
    def observeBodies(self, out=None, stream=None):
        """torch.float64 [num_bodies, 20] on the handle's device: per body its mass, mass centre and velocity, volume, rest volume, worst
        volume ratio, inverted tets, box, fastest particle and non-finite particles (columns: _capi.OBS_*; definitions: include/tetsim.h).
        No host copy and no synchronisation; valid for work enqueued on `stream` (as in exportTensors) after this returns.  The tensor is
        allocated once and reused by later calls unless `out` supplies it (rows may be strided: anything between them is left alone)."""
        import torch
        dev, s = self._torch_stream(torch, stream)
        n, w = self.info.num_bodies, capi.OBS_WIDTH
        out = self._out_rows(torch, dev, "observations", out, (n, w), torch.float64)
        capi.check(self._L.tetsim_observe_bodies_device(self._h, out.data_ptr(), 8 * out.stride(0) if n > 1 else 0, s), self._h)
        return out

    def bodyObservations(self):
        """observeBodies() on the host: a numpy float64 [num_bodies, 20] array.  Synchronises."""
        out = np.empty((self.info.num_bodies, capi.OBS_WIDTH), dtype=np.float64)
        capi.check(self._L.tetsim_read_body_observations(self._h, out.ctypes.data_as(C.POINTER(C.c_double))), self._h)
        return out

    # -- per-body pose (include/tetsim.h: tetsim_body_poses_device): one row of _capi.POSE_WIDTH doubles per body --------------------
    def observePoses(self, out=None, stream=None):
        """torch.float64 [num_bodies, 48] on the handle's device: per body the mass moments [0..25] and what follows from them -- mass
        centre and its velocity, the rotation that best maps the rest shape onto the current one (xyzw, w >= 0: what place_rows takes
        as q), angular velocity and angular momentum about the mass centre, the rms distance to the best rigid fit and the eigenvalue gap
        that says how well defined the rotation is (columns: _capi.POSE_*; definitions: include/tetsim.h).  `out` and `stream` as in
        observeBodies: no host copy, no synchronisation, the tensor allocated once and reused unless `out` supplies it."""
        import torch
        dev, s = self._torch_stream(torch, stream)
        n, w = self.info.num_bodies, capi.POSE_WIDTH
        out = self._out_rows(torch, dev, "poses", out, (n, w), torch.float64)
        capi.check(self._L.tetsim_body_poses_device(self._h, out.data_ptr(), 8 * out.stride(0) if n > 1 else 0, s), self._h)
        return out

    def bodyPoses(self):
        """observePoses() on the host: a numpy float64 [num_bodies, 48] array.  Synchronises."""
        out = np.empty((self.info.num_bodies, capi.POSE_WIDTH), dtype=np.float64)
        capi.check(self._L.tetsim_read_body_poses(self._h, out.ctypes.data_as(C.POINTER(C.c_double))), self._h)
        return out

    # -- touch sensing (include/tetsim.h: tetsim_touch_bodies_device / _particles_device): the bodies' contacts with their colliders --
    def touchBodies(self, margin, out=None, stream=None):
        """torch.float64 [num_bodies, 100] on the handle's device: per body the particles that touch a collider of the list its substeps
        walk (signed distance below `margin`, metres), the least distance and its slot, the list's length, and per slot its kind, the
        touching particles, the least distance, the centroid, the mean normal and the mean velocity relative to the collider (columns:
        _capi.TOUCH_*; definitions: include/tetsim.h).  Read-only.  `out` and `stream` as in observeBodies: no host copy, no
        synchronisation, the tensor allocated once and reused unless `out` supplies it."""
        import torch
        dev, s = self._torch_stream(torch, stream)
        n = self.info.num_bodies
        out = self._out_rows(torch, dev, "touch", out, (n, capi.TOUCH_WIDTH), torch.float64)
        capi.check(self._L.tetsim_touch_bodies_device(self._h, float(margin), out.data_ptr(), 8 * out.stride(0) if n > 1 else 0, s), self._h)
        return out

    def bodyTouch(self, margin):
        """touchBodies(margin) on the host: a numpy float64 [num_bodies, 100] array.  Synchronises."""
        out = np.empty((self.info.num_bodies, capi.TOUCH_WIDTH), dtype=np.float64)
        capi.check(self._L.tetsim_read_body_touch(self._h, float(margin), out.ctypes.data_as(C.POINTER(C.c_double))), self._h)
        return out

    def touchParticlesDevice(self, margin, out=None, stream=None):
        """torch.float32 [num_particles, 8] on the handle's device, row i = particle i of the caller's numbering: the signed distance to
        the nearest collider of its body's list, that collider's outward normal, its slot (-1: none) and the number of slots the
        particle touches (columns: _capi.TOUCH_P_*).  `margin`, `out` and `stream` as in touchBodies."""
        import torch
        dev, s = self._torch_stream(torch, stream)
        n, w = self.info.owned_particles, capi.TOUCH_PARTICLE_WIDTH
        out = self._out_rows(torch, dev, "touch_particles", out, (n, w), torch.float32)
        capi.check(self._L.tetsim_touch_particles_device(self._h, float(margin), out.data_ptr(), 4 * out.stride(0) if n > 1 else 0, s), self._h)
        return out

    # -- per-tet strain (include/tetsim.h: tetsim_tet_strain_device / _body_strain_device / _visual_strain_device) -----------------
    def tetStrainDevice(self, out=None, stream=None):
        """torch.float32 [num_elems, 16] on the handle's device, row t = tet t of the caller's numbering: the deformation gradient F
        (9, column-major), J = det F, DEV (the reference's r_s), the principal stretches (3, descending) and the norm of the Green
        strain (columns: _capi.STRAIN_*; definitions: include/tetsim.h); a degenerate tet's row is NaN.  No host copy and no
        synchronisation; `out` and `stream` as in observeBodies."""
        import torch
        dev, s = self._torch_stream(torch, stream)
        n, w = self.info.num_elems, capi.STRAIN_WIDTH
        out = self._out_rows(torch, dev, "tetStrain", out, (n, w), torch.float32)
        capi.check(self._L.tetsim_tet_strain_device(self._h, out.data_ptr(), 4 * out.stride(0) if n > 1 else 0, s), self._h)
        return out

    def tetStrain(self):
        """tetStrainDevice() on the host: a numpy float32 [num_elems, 16] array.  Synchronises."""
        out = np.empty((self.info.num_elems, capi.STRAIN_WIDTH), dtype=np.float32)
        capi.check(self._L.tetsim_read_tet_strain(self._h, _fp(out.reshape(-1))), self._h)
        return out

    def bodyStrainDevice(self, out=None, stream=None):
        """torch.float64 [num_bodies, 8] on the handle's device: per body the largest and the smallest stretch, min and max J, max GREEN,
        the sums of |V0| * GREEN^2 and of |V0|, and the number of tets left out (degenerate or non-finite).  The tet rows are not
        materialised.  `out` and `stream` as in observeBodies."""
        import torch
        dev, s = self._torch_stream(torch, stream)
        n, w = self.info.num_bodies, capi.STRAIN_BODY_WIDTH
        out = self._out_rows(torch, dev, "bodyStrain", out, (n, w), torch.float64)
        capi.check(self._L.tetsim_body_strain_device(self._h, out.data_ptr(), 8 * out.stride(0) if n > 1 else 0, s), self._h)
        return out

    def visualStrainDevice(self, channel, out=None, stream=None):
        """torch.float32 [num_vis_verts] on the handle's device: for every attached visual vertex the value `channel` of the tet that
        carries it -- what a renderer colours the skinned mesh by.  channel: an index 0..14 or one of _STRAIN_CHANNELS ("J", "dev",
        "stretch0".."stretch2", "green", "F00".."F22" as F<row><column>).  `out` and `stream` as in observeBodies."""
        import torch
        dev, s = self._torch_stream(torch, stream)
        if isinstance(channel, str):
            if channel not in _STRAIN_CHANNELS:
                raise ValueError("channel must be an index 0..14 or one of %s" % sorted(_STRAIN_CHANNELS))
            channel = _STRAIN_CHANNELS[channel]
        n = self.info.num_vis_verts
        out = self._out_rows(torch, dev, "visualStrain", out, (n,), torch.float32)
        capi.check(self._L.tetsim_visual_strain_device(self._h, int(channel), out.data_ptr(), 4 * out.stride(0) if n > 1 else 0, s), self._h)
        return out

    # -- embedded visual mesh (Softbody.js:259-277 / SoftbodyGPU.js:424-448), skinned on the device ---------------
    def setVisualMesh(self, visVerts, restNormals=None):
        vv = _f32(visVerts).reshape(-1)
        n0 = None if restNormals is None else _f32(restNormals).reshape(-1)
        capi.check(self._L.tetsim_set_visual_mesh(self._h, _fp(vv), vv.size // 4, _fp(n0) if n0 is not None else None), self._h)
        self._has_normals = n0 is not None
        capi.check(self._L.tetsim_get_info(self._h, C.byref(self.info)), self._h)
        self.numVisVerts = self.info.num_vis_verts   # (a partition keeps the rows of the tets it owns: visualIds)

    @property
    def visualIds(self):
        """Row of the caller's visVerts behind each attached visual vertex (identity when unpartitioned; a partition: its own rows)."""
        out = np.empty(self.numVisVerts, dtype=np.int32)
        capi.check(self._L.tetsim_get_visual_ids(self._h, _ip(out)), self._h)
        return out

    def refreshFinalGhosts(self):
        """RCCL partitions, every rank together, after the frame's last substep and before visualPositions(): the ghost particles'
        end-of-substep positions from their owners (in-process groups: group_refresh_final).  The read itself never communicates."""
        capi.check(self._L.tetsim_halo_refresh_final(self._h), self._h)

    def visualPositions(self, with_normals=False):
        out = np.empty(3 * self.numVisVerts, dtype=np.float32)
        nrm = np.empty(3 * self.numVisVerts, dtype=np.float32) if with_normals else None
        capi.check(self._L.tetsim_read_visual_mesh(self._h, _fp(out), _fp(nrm) if with_normals else None), self._h)
        return (out.reshape(-1, 3), nrm.reshape(-1, 3)) if with_normals else out.reshape(-1, 3)

    def setVisualTriangles(self, visTriIds):
        """The visual mesh's triangle list (the reference's `visTriIds`, Softbody.js:48-50): enables visualVertexNormals()."""
        tri = np.ascontiguousarray(np.asarray(visTriIds).reshape(-1), dtype=np.int32)
        capi.check(self._L.tetsim_set_visual_triangles(self._h, tri.ctypes.data_as(C.POINTER(C.c_int32)), tri.size // 3), self._h)

    def visualVertexNormals(self):
        """`visMesh.geometry.computeVertexNormals()` (Softbody.js:273) evaluated on the device, bit-exact with three.js r160."""
        out = np.empty(3 * self.numVisVerts, dtype=np.float32)
        capi.check(self._L.tetsim_read_visual_vertex_normals(self._h, _fp(out)), self._h)
        return out.reshape(-1, 3)

    def visualVertexNormalsFrom(self, allPositions):
        """computeVertexNormals of THIS body's rows from a complete set of visual positions [rows of visVerts, 3] -- a partition: the
        ranks' skins put together (visualPositions() scattered by visualIds); include/tetsim.h: tetsim_visual_vertex_normals_from."""
        ap = _f32(allPositions).reshape(-1)
        out = np.empty(3 * self.numVisVerts, dtype=np.float32)
        capi.check(self._L.tetsim_visual_vertex_normals_from(self._h, _fp(ap), _fp(out)), self._h)
        return out.reshape(-1, 3)

    # -- caller-provided transports (include/tetsim.h: tetsim_get_halo_plan / tetsim_halo_export / tetsim_halo_import) --
    def haloPlan(self):
        """[(neighbour rank, global ids sent, global ids received)] in neighbour-slot order."""
        n = self.info.num_neighbours
        if n == 0:
            return []
        neigh, sc, rc = (np.empty(n, dtype=np.int32) for _ in range(3))
        capi.check(self._L.tetsim_get_halo_plan(self._h, _ip(neigh), _ip(sc), _ip(rc), None, None), self._h)
        sid, rid = np.empty(int(sc.sum()), dtype=np.int32), np.empty(int(rc.sum()), dtype=np.int32)
        capi.check(self._L.tetsim_get_halo_plan(self._h, _ip(neigh), _ip(sc), _ip(rc), _ip(sid), _ip(rid)), self._h)
        so, ro = np.concatenate([[0], np.cumsum(sc)]), np.concatenate([[0], np.cumsum(rc)])
        return [(int(neigh[i]), sid[so[i]:so[i + 1]].copy(), rid[ro[i]:ro[i + 1]].copy()) for i in range(n)]

    def haloExport(self, slot, count):
        """Predicted positions (x, y, z, w) this handle owes neighbour slot `slot`, as a host array [count, 4]."""
        out = np.empty(4 * count, dtype=np.float32)
        capi.check(self._L.tetsim_halo_export(self._h, int(slot), _fp(out)), self._h)
        return out.reshape(-1, 4)

    def haloImport(self, slot, xyzw):
        """Install the ghost predictions received from neighbour slot `slot`."""
        a = _f32(xyzw).reshape(-1)
        capi.check(self._L.tetsim_halo_import(self._h, int(slot), _fp(a)), self._h)

    # -- grab (Softbody.js:279-298) -------------------------------------------------------------------
    def startGrab(self, pos):
        p = _f32([pos["x"], pos["y"], pos["z"]] if isinstance(pos, dict) else pos)
        gid = C.c_int32(-1)
        capi.check(self._L.tetsim_start_grab(self._h, _fp(p), C.byref(gid)), self._h)
        self.grabId = gid.value
        self.grabPos[:] = p
        return self.grabId

    # -- picking (include/tetsim.h: tetsim_raycast_visual; Grabber.start, Softbody.js:440-456) -------------
    def raycastVisual(self, origins, directions, near=0.0, far=np.inf):
        """three.js `Raycaster(origin, direction, near, far).intersectObject(visMesh)[0]` for every ray, on the device, bit for bit:
        a structured array (RAY_HIT_DTYPE: hit, body, triangle = faceIndex, distance, point)."""
        rays = make_rays(origins, directions, near, far)
        hits = np.zeros(len(rays), dtype=RAY_HIT_DTYPE)
        capi.check(self._L.tetsim_raycast_visual(self._h, rays.ctypes.data, len(rays), hits.ctypes.data), self._h)
        return hits

    def startGrabRay(self, origin, direction, near=0.0, far=np.inf):
        """Grabber.start in one call: cast the ray, grab the particle nearest to the hit point.  Returns (grabId, hit record);
        a miss leaves the grab as it was and returns (-1, record with hit 0)."""
        ray = make_rays(origin, direction, near, far)
        hit = np.zeros(1, dtype=RAY_HIT_DTYPE)
        gid = C.c_int32(-1)
        capi.check(self._L.tetsim_start_grab_ray(self._h, ray.ctypes.data_as(C.POINTER(capi.TetSimRay)), hit.ctypes.data_as(C.POINTER(capi.TetSimRayHit)),
                                                 C.byref(gid)), self._h)
        if hit["hit"][0]:
            self.grabId = gid.value
            self.grabPos[:] = (ray["origin"][0] + ray["direction"][0] * hit["distance"][0]).astype(np.float32)
        return gid.value, hit[0]

    def visualBoundingSphere(self):
        """`visMesh.geometry.computeBoundingSphere()` (Softbody.js:256,276) on the device: (centre [3] f64, radius)."""
        c, r = np.empty(3, dtype=np.float64), C.c_double()
        capi.check(self._L.tetsim_read_visual_bounding_sphere(self._h, c.ctypes.data_as(C.POINTER(C.c_double)), C.byref(r)), self._h)
        return c, float(r.value)

    # -- range sensors (include/tetsim.h: tetsim_raycast_visual_device / tetsim_visual_bounding_spheres_device) -----
    def raycastVisualDevice(self, rays, bodies=None, out=None, stream=None):
        """raycastVisual from and into device memory, with no host copy and no synchronisation.  rays: torch.float64 [count, 8] on the
        handle's device (rays_tensor; the rows may be strided); bodies: torch.int32 [count] -- ray i is cast against body bodies[i]
        ALONE and gets what that body would give on its own, `triangle` counted in this handle's list -- or None: every ray against the
        whole mesh, exactly raycastVisual.  Returns views onto one torch.uint8 [count, 48] buffer of TetSimRayHit records (`raw`: cached
        like the export tensors, or `out`, whose rows may be strided): hit, body, triangle (int32 [count]), distance (float64 [count]),
        point (float64 [count, 3]).  An invalid ray or body gets hit = _capi.RAY_INVALID instead of an exception.  Rays grouped by body
        are the fast case.  Valid for work enqueued on `stream` (as in exportTensors) after this returns."""
        return self._raycastDevice(self._L.tetsim_raycast_visual_device, rays, bodies, out, stream)

    def raycastVisualBvhDevice(self, rays, bodies=None, out=None, stream=None):
        """raycastVisualDevice through a tree of boxes per body that is refitted on the device at every call (include/tetsim.h:
        tetsim_raycast_visual_bvh_device): the same arguments and the same views.  Many rays cost orders of magnitude less, and they need
        not be grouped by body.  The answer has a definition of its own (tests/raycast_bvh_ref.py), which differs from raycastVisualDevice's
        only for hits that are numerically meaningless -- a ray nearly in a triangle's plane.  The handle's first such call builds the
        tree's topology on the host and may block."""
        return self._raycastDevice(self._L.tetsim_raycast_visual_bvh_device, rays, bodies, out, stream)

    def _raycastDevice(self, call, rays, bodies, out, stream):
        import torch
        out = self._recordsDevice(call, "rays", rays, 8, bodies, "rayHits", 48, out, stream)
        i32, f64 = out.view(torch.int32), out.view(torch.float64)   # (rows of 12 / 6 of them; a strided `out` keeps its row stride)
        return {"hit": i32[:, 0], "body": i32[:, 1], "triangle": i32[:, 2], "distance": f64[:, 2], "point": f64[:, 3:6], "raw": out}

    def _recordsDevice(self, call, name, records, width, bodies, key, out_bytes, out, stream):
        """What the device calls on records share: `records` is checked (float64 [count, width], `name` in the refusal), `bodies` too, the
        uint8 [count, out_bytes] answer is `out` or the cached tensor `key`, and `call` gets pointers and strides by the ABI's rules (no
        pointer for no rows, stride 0 for at most one).  Returns the answer's tensor."""
        import torch
        dev, s = self._torch_stream(torch, stream)
        if (not isinstance(records, torch.Tensor) or records.dtype != torch.float64 or records.device != dev or records.dim() != 2 or records.shape[1] != width
                or (records.shape[0] and records.stride(1) != 1) or (records.shape[0] > 1 and records.stride(0) < width)):
            raise ValueError("%s must be a float64 tensor on %s of shape (count, %d) with contiguous, non-overlapping rows" % (name, dev, width))
        n = int(records.shape[0])
        if bodies is not None and (not isinstance(bodies, torch.Tensor) or bodies.dtype != torch.int32 or bodies.device != dev
                                   or tuple(bodies.shape) != (n,) or not bodies.is_contiguous()):
            raise ValueError("bodies must be a contiguous int32 tensor on %s of shape (%d,)" % (dev, n))
        out = self._out_rows(torch, dev, key, out, (n, out_bytes), torch.uint8, align=8)
        capi.check(call(self._h, records.data_ptr() if n else None, 8 * records.stride(0) if n > 1 else 0, bodies.data_ptr() if bodies is not None and n else None, n,
                        out.data_ptr() if n else None, out.stride(0) if n > 1 else 0, s), self._h)
        return out

    # -- closest points (include/tetsim.h: tetsim_closest_visual_device / tetsim_closest_visual) --------------------
    def closestPointsDevice(self, queries, bodies=None, out=None, stream=None):
        """The nearest point of a body's skinned surface to every query point, from and into device memory, with no host copy and no
        synchronisation, through the refitted tree of raycastVisualBvhDevice.  queries: torch.float64 [count, 4] on the handle's device
        (point_queries_tensor: point xyz, max_distance; the rows may be strided); bodies: torch.int32 [count] -- query i is answered by
        body bodies[i] ALONE, `triangle` counted in this handle's list -- or None: by the whole mesh.  Returns views onto one torch.uint8
        [count, 64] buffer of TetSimClosest records (`raw`: cached like the export tensors, or `out`, whose rows may be strided): found,
        body, triangle, region (int32 [count]), distance (float64 [count]), point (float64 [count, 3]), v, w (float64 [count]).  An invalid
        query or body gets found = _capi.CLOSEST_INVALID instead of an exception.  The handle's first tree call builds the topology on the
        host and may block.  Valid for work enqueued on `stream` (as in exportTensors) after this returns."""
        import torch
        out = self._recordsDevice(self._L.tetsim_closest_visual_device, "queries", queries, 4, bodies, "closestPoints", 64, out, stream)
        i32, f64 = out.view(torch.int32), out.view(torch.float64)   # (rows of 16 / 8 of them; a strided `out` keeps its row stride)
        return {"found": i32[:, 0], "body": i32[:, 1], "triangle": i32[:, 2], "region": i32[:, 3], "distance": f64[:, 2], "point": f64[:, 3:6],
                "v": f64[:, 6], "w": f64[:, 7], "raw": out}

    def closestPoints(self, points, max_distance=np.inf, bodies=None):
        """closestPointsDevice for host arrays: points [n, 3], max_distance a scalar or [n], bodies [n] int or None -> a structured array
        (CLOSEST_DTYPE).  Synchronises; an invalid query raises TetSimError(EINVAL)."""
        queries = make_point_queries(points, max_distance)
        b = None if bodies is None else np.ascontiguousarray(bodies, dtype=np.int32)
        if b is not None and b.shape != (len(queries),):
            raise ValueError("bodies must have one entry per point")
        out = np.zeros(len(queries), dtype=CLOSEST_DTYPE)
        capi.check(self._L.tetsim_closest_visual(self._h, queries.ctypes.data, None if b is None else b.ctypes.data, len(queries), out.ctypes.data), self._h)
        return out

    def visualBoundingSpheresDevice(self, out=None, stream=None):
        """torch.float64 [num_bodies, 4] on the handle's device: (centre x, y, z, radius) of every body's visual rows -- what
        visualBoundingSphere() returns for that body alone, bit for bit; a body without rows: zeros.  No host copy and no synchronisation;
        `out` and `stream` as in observeBodies."""
        import torch
        dev, s = self._torch_stream(torch, stream)
        n = self.info.num_bodies
        out = self._out_rows(torch, dev, "visualSpheres", out, (n, 4), torch.float64)
        capi.check(self._L.tetsim_visual_bounding_spheres_device(self._h, out.data_ptr(), 8 * out.stride(0) if n > 1 else 0, s), self._h)
        return out

    def nearestParticle(self, pos):
        """(global id, squared distance) of the owned particle nearest to pos -- the building block of startGrab for partitioned
        bodies: min over the partitions (ties: lowest id), then setGrab(id, pos) on each."""
        p = _f32([pos["x"], pos["y"], pos["z"]] if isinstance(pos, dict) else pos)
        gid, d2 = C.c_int32(), C.c_double()
        capi.check(self._L.tetsim_nearest_particle(self._h, _fp(p), C.byref(gid), C.byref(d2)), self._h)
        return int(gid.value), float(d2.value)

    def setGrab(self, gid, pos):
        p = _f32(pos)
        capi.check(self._L.tetsim_set_grab(self._h, int(gid), _fp(p)), self._h)
        self.grabId = int(gid)
        self.grabPos[:] = p

    def moveGrabbed(self, pos):
        p = _f32([pos["x"], pos["y"], pos["z"]] if isinstance(pos, dict) else pos)
        self.setGrab(self.grabId, p)

    def endGrab(self):
        capi.check(self._L.tetsim_set_grab(self._h, -1, None), self._h)
        self.grabId = -1

    # -- kinematic colliders (include/tetsim.h tetsim_set_colliders) ---------------------------------
    def setColliders(self, colliders):
        """Replace the body's obstacles: a list of at most 8 dicts (make_colliders); [] clears.  They take effect at the next step
        call and stay fixed for its substeps; move one by calling this again between frames (and give it `velocity` so friction
        acts on the motion relative to it).  Raises TetSimError(EINVAL) for an invalid list, which leaves the previous one."""
        arr = make_colliders(list(colliders))
        capi.check(self._L.tetsim_set_colliders(self._h, arr, len(colliders)), self._h)

    # -- body grabs (include/tetsim.h: tetsim_set_body_grabs / _device, tetsim_nearest_particles_device) ---------------
    def setBodyGrabs(self, particles, targets):
        """Hold one particle of every body: particles int32 [num_bodies], the index INSIDE the body (-1 = not held), targets float32
        [num_bodies, 3].  Body b then steps exactly as it would alone with setGrab(particles[b], targets[b]), bit for bit.  None
        switches body grabs off.  Raises TetSimError(EINVAL) for an index outside its body or a non-finite target (the previous table
        stays in force), TetSimError(ESTATE) while a handle grab is set."""
        if particles is None:
            capi.check(self._L.tetsim_set_body_grabs(self._h, None, None), self._h)
            return
        n = self.info.num_bodies
        p = np.ascontiguousarray(particles, dtype=np.int32).reshape(-1)
        t = _f32(targets).reshape(-1)
        if p.size != n or t.size != 3 * n:
            raise ValueError("particles must hold %d indices and targets %d rows of xyz" % (n, n))
        capi.check(self._L.tetsim_set_body_grabs(self._h, _ip(p), _fp(t)), self._h)

    def setBodyGrabsDevice(self, particles, targets, bodies=None, stream=None):
        """setBodyGrabs from device tensors, with no host copy and no synchronisation: particles torch.int32 [num_bodies] (contiguous),
        targets torch.float32 [num_bodies, 3] (rows contiguous; the row stride is passed through), both on the handle's device and
        produced on `stream` (as in exportTensors; reusable on it right after the call).  bodies: a mask as in restore -- a body it leaves
        out keeps its row.  A row the table cannot hold (an index outside its body, a non-finite target) means "not held" for that body."""
        n = self.info.num_bodies

        def call(torch, dev, mask, s):
            if (not isinstance(particles, torch.Tensor) or particles.dtype != torch.int32 or particles.device != dev or tuple(particles.shape) != (n,)
                    or not particles.is_contiguous()):
                raise ValueError("particles must be a contiguous int32 tensor on %s of shape (%d,)" % (dev, n))
            _check_rows(torch, targets, dev, n, 3, "targets")
            return self._L.tetsim_set_body_grabs_device(self._h, particles.data_ptr(), targets.data_ptr(), 4 * targets.stride(0) if n > 1 else 0, mask, s)
        self._masked_call(bodies, stream, call)

    # -- body pins (include/tetsim.h: tetsim_set_body_pins / _device) -------------------------------------------------------
    def setBodyPins(self, particles, targets):
        """Hold up to K particles of every body: particles int32 [num_bodies, K], indices INSIDE the body (-1 = unused row), targets
        float32 [num_bodies, K, 3].  Every particle a row names is held at its target exactly as setGrab holds its particle; if two
        rows of a body name one particle the lowest row wins.  None, None switches pins off.  Raises TetSimError(EINVAL) for an index
        outside its body or a non-finite target (the previous table stays in force), TetSimError(ESTATE) while a handle grab or body
        grabs are set.  A call with another K than the last one makes the table anew and may block."""
        if particles is None:
            capi.check(self._L.tetsim_set_body_pins(self._h, None, None, 0), self._h)
            return
        n = self.info.num_bodies
        p = np.ascontiguousarray(particles, dtype=np.int32)
        t = _f32(targets)
        if p.ndim != 2 or p.shape[0] != n or t.shape != p.shape + (3,):
            raise ValueError("particles must be [%d, per_body] and targets [%d, per_body, 3]" % (n, n))
        capi.check(self._L.tetsim_set_body_pins(self._h, _ip(p.reshape(-1)), _fp(t.reshape(-1)), p.shape[1]), self._h)

    def setBodyPinsDevice(self, particles, targets, bodies=None, stream=None):
        """setBodyPins from device tensors, with no host copy and no synchronisation (a call with another K than the last one makes the
        table anew and may block): particles torch.int32 [num_bodies, K] (contiguous), targets torch.float32 [num_bodies, K, 3] -- or the
        [..., :3] view of a [num_bodies, K, 4] tensor: rows evenly spaced, the stride is passed through -- both on the handle's device
        and produced on `stream` (as in exportTensors; reusable on it right after the call).  bodies: a mask as in restore -- a body it
        leaves out keeps all its rows.  A row the table cannot hold (an index outside its body, a non-finite target) holds nothing and
        disturbs no other row."""
        n = self.info.num_bodies

        def call(torch, dev, mask, s):
            if (not isinstance(particles, torch.Tensor) or particles.dtype != torch.int32 or particles.device != dev or particles.dim() != 2
                    or particles.shape[0] != n or particles.shape[1] < 1 or not particles.is_contiguous()):
                raise ValueError("particles must be a contiguous int32 tensor on %s of shape (%d, per_body >= 1)" % (dev, n))
            k = int(particles.shape[1])
            ok = (isinstance(targets, torch.Tensor) and targets.dtype == torch.float32 and targets.device == dev and tuple(targets.shape) == (n, k, 3)
                  and targets.stride(2) == 1)
            if ok:
                step = targets.stride(1) if k > 1 else (targets.stride(0) if n > 1 else 3)
                ok = step >= 3 and (n == 1 or k == 1 or targets.stride(0) == k * step)
            if not ok:
                raise ValueError("targets must be a float32 tensor on %s of shape (%d, %d, 3) with a contiguous last dimension and evenly spaced rows" % (dev, n, k))
            return self._L.tetsim_set_body_pins_device(self._h, particles.data_ptr(), targets.data_ptr(), 4 * step if n * k > 1 else 0, k, mask, s)
        self._masked_call(bodies, stream, call)

    # -- body colliders (include/tetsim.h: tetsim_set_body_colliders / _device) ---------------------------------------------
    def setBodyColliders(self, lists_or_rows):
        """Give every body its own obstacles: a list per body of the dicts setColliders takes (at most 8 each), or the float32
        [num_bodies, per_body, 24] rows body_collider_rows makes of them.  Body b then steps exactly as it would alone with
        setColliders of its rows, bit for bit.  None switches body colliders off.  Raises TetSimError(EINVAL) for a row setColliders
        would refuse (the previous table stays in force), TetSimError(ESTATE) while the handle's own list is set."""
        if lists_or_rows is None:
            capi.check(self._L.tetsim_set_body_colliders(self._h, None, 0), self._h)
            return
        n = self.info.num_bodies
        rows = lists_or_rows if isinstance(lists_or_rows, np.ndarray) else body_collider_rows(lists_or_rows)
        rows = _f32(rows)
        if rows.ndim != 3 or rows.shape[0] != n or rows.shape[2] != capi.BODY_COLLIDER_FLOATS:
            raise ValueError("rows must be [%d, per_body, %d]" % (n, capi.BODY_COLLIDER_FLOATS))
        capi.check(self._L.tetsim_set_body_colliders(self._h, _fp(rows.reshape(-1)), rows.shape[1]), self._h)

    def setBodyCollidersDevice(self, rows, bodies=None, stream=None):
        """setBodyColliders from a device tensor, with no host copy and no synchronisation: rows torch.float32 [num_bodies, per_body, w]
        with w >= 24 and a contiguous last dimension, the rows evenly spaced in memory (a [..., :24] view of a wider tensor is fine:
        nothing outside a row's 24 floats is read), on the handle's device and produced on `stream` (as in exportTensors; reusable on
        it right after the call).  bodies: a mask as in setBodyGrabsDevice -- a body it leaves out keeps its whole list.  A row the
        table cannot hold (what setColliders would refuse) is an empty slot for that body and disturbs no other row."""
        n, w = self.info.num_bodies, capi.BODY_COLLIDER_FLOATS

        def call(torch, dev, mask, s):
            ok = (isinstance(rows, torch.Tensor) and rows.dtype == torch.float32 and rows.device == dev and rows.dim() == 3 and rows.shape[0] == n
                  and 1 <= rows.shape[1] and rows.shape[2] >= w and rows.stride(2) == 1)
            if ok:
                per_body = int(rows.shape[1])
                step = rows.stride(1) if per_body > 1 else (rows.stride(0) if n > 1 else w)
                ok = step >= w and (n == 1 or per_body == 1 or rows.stride(0) == per_body * step)
            if not ok:
                raise ValueError("rows must be a float32 tensor on %s of shape (%d, per_body, >= %d) with a contiguous last dimension and evenly spaced rows" % (dev, n, w))
            return self._L.tetsim_set_body_colliders_device(self._h, rows.data_ptr(), 4 * step if n * per_body > 1 else 0, per_body, mask, s)
        self._masked_call(bodies, stream, call)

    # -- body parameters (include/tetsim.h: tetsim_set_body_params / _device) ------------------------------------------------
    def setBodyParams(self, rows_or_dicts):
        """Give every body its own physicsParams: [num_bodies, 10] rows (an array, a host tensor, nested lists), or a list per body of dicts (None entries and missing
        keys come from the handle's physicsParams; body_param_rows).  Body b then steps exactly as it would alone with its row as
        physicsParams, bit for bit; the physicsParams of the step calls are not looked at.  None switches body parameters off.  Raises
        TetSimError(EINVAL) for a row with a non-finite value (the previous table stays in force)."""
        if rows_or_dicts is None:
            capi.check(self._L.tetsim_set_body_params(self._h, None), self._h)
            return
        n = self.info.num_bodies
        if isinstance(rows_or_dicts, (list, tuple)) and all(d is None or isinstance(d, dict) for d in rows_or_dicts):
            rows = body_param_rows(list(rows_or_dicts), self.physicsParams)
        else:   # rows: an array, a host tensor, nested sequences of numbers
            try:
                rows = np.ascontiguousarray(rows_or_dicts, dtype=np.float64)
            except (TypeError, ValueError):
                raise ValueError("rows must be [%d, %d] numbers, or a list per body of dicts and None" % (n, capi.BODY_PARAMS_WIDTH)) from None
        if rows.shape != (n, capi.BODY_PARAMS_WIDTH):
            raise ValueError("rows must be [%d, %d]" % (n, capi.BODY_PARAMS_WIDTH))
        capi.check(self._L.tetsim_set_body_params(self._h, rows.ctypes.data_as(capi.C.POINTER(capi.C.c_double))), self._h)

    def setBodyParamsDevice(self, rows, bodies=None, stream=None):
        """setBodyParams from a device tensor, with no host copy and no synchronisation: rows torch.float64 [num_bodies, w] with w >= 10
        and a contiguous last dimension (a [:, :10] view of a wider tensor is fine: nothing outside a row's ten doubles is read), on the
        handle's device and produced on `stream` (as in exportTensors; reusable on it right after the call).  bodies: a mask as in
        setBodyGrabsDevice -- a body it leaves out keeps its row.  A row with a non-finite value leaves its body's previous row in place."""
        n, w = self.info.num_bodies, capi.BODY_PARAMS_WIDTH

        def call(torch, dev, mask, s):
            ok = (isinstance(rows, torch.Tensor) and rows.dtype == torch.float64 and rows.device == dev and rows.dim() == 2 and rows.shape[0] == n
                  and rows.shape[1] >= w and rows.stride(1) == 1 and (n == 1 or rows.stride(0) >= w))
            if not ok:
                raise ValueError("rows must be a float64 tensor on %s of shape (%d, >= %d) with a contiguous last dimension" % (dev, n, w))
            return self._L.tetsim_set_body_params_device(self._h, rows.data_ptr(), 8 * rows.stride(0) if n > 1 else 0, mask, s)
        self._masked_call(bodies, stream, call)

    def nearestParticlesDevice(self, points, out_ids=None, out_dist2=None, stream=None):
        """(ids, dist2): per body the index INSIDE the body of its particle nearest to points[b], torch.int32 [num_bodies], and the squared
        distance, torch.float64 [num_bodies] -- what nearestParticle returns for that body alone in the same state, bit for bit (-1 and
        DBL_MAX for a body with no pickable particle).  points: torch.float32 [num_bodies, 3] on the handle's device, rows contiguous.
        No host copy and no synchronisation; `ids` goes straight into setBodyGrabsDevice.  The outputs are allocated once and reused by
        later calls unless out_ids / out_dist2 supply them (contiguous); `stream` as in exportTensors."""
        import torch
        dev, s = self._torch_stream(torch, stream)
        n = self.info.num_bodies
        _check_rows(torch, points, dev, n, 3, "points")
        outs = []
        for key, out, dtype in (("nearestIds", out_ids, torch.int32), ("nearestDist2", out_dist2, torch.float64)):
            outs.append(self._out_rows(torch, dev, key, out, (n,), dtype, key, packed=True))
        capi.check(self._L.tetsim_nearest_particles_device(self._h, points.data_ptr(), 4 * points.stride(0) if n > 1 else 0,
                                                           outs[0].data_ptr(), outs[1].data_ptr(), s), self._h)
        return outs[0], outs[1]

    # -- measurement ----------------------------------------------------------------------------------
    def profile(self, n, dt, physicsParams=None):
        pp = self.physicsParams if physicsParams is None else physicsParams
        pr = capi.TetSimProfile()
        capi.check(self._L.tetsim_profile(self._h, int(n), float(dt), C.byref(make_params(pp)), C.byref(pr)), self._h)
        return dict(total_ms=pr.total_ms, tet_ms=pr.kernel_ms[capi.K_TET], vertex_ms=pr.kernel_ms[capi.K_VERTEX],
                    tet_launches=pr.launches[capi.K_TET], vertex_launches=pr.launches[capi.K_VERTEX], substeps=pr.substeps,
                    tets_per_tet_launch=pr.tets_per_tet_launch)

    def timeKernels(self, reps, dt, physicsParams=None):
        """Kernel-only timing (back-to-back launches, one event pair per kernel class).  Scratch bodies only."""
        pp = self.physicsParams if physicsParams is None else physicsParams
        pr = capi.TetSimProfile()
        capi.check(self._L.tetsim_time_kernels(self._h, int(reps), float(dt), C.byref(make_params(pp)), C.byref(pr)), self._h)
        return dict(tet_us=pr.kernel_ms[capi.K_TET] / pr.launches[capi.K_TET] * 1e3,
                    vertex_us=pr.kernel_ms[capi.K_VERTEX] / pr.launches[capi.K_VERTEX] * 1e3,
                    tet_launches_per_substep=pr.launches[capi.K_TET] // reps)

    def timeSubsteps(self, n, dt, physicsParams=None):
        pp = self.physicsParams if physicsParams is None else physicsParams
        ms = C.c_double()
        capi.check(self._L.tetsim_time_step_n(self._h, int(n), float(dt), C.byref(make_params(pp)), C.byref(ms)), self._h)
        return ms.value


def halo_probe(body, reps=100):
    """{min, median, max} microseconds of one halo exchange of this rank with its real neighbours and message sizes (a collective of
    all ranks, between steps; include/tetsim.h: tetsim_halo_probe)."""
    a, b, c = C.c_double(), C.c_double(), C.c_double()
    capi.check(capi.lib().tetsim_halo_probe(body._h, int(reps), C.byref(a), C.byref(b), C.byref(c)), body._h)
    return {"min": a.value, "median": b.value, "max": c.value}


def halo_p2p_probe(body, reps=100):
    """{min, median, max} microseconds of one hand-over of the peer-to-peer halo with all neighbours at once (a collective of all ranks,
    between steps; include/tetsim.h: tetsim_halo_p2p_probe)."""
    a, b, c = C.c_double(), C.c_double(), C.c_double()
    capi.check(capi.lib().tetsim_halo_p2p_probe(body._h, int(reps), C.byref(a), C.byref(b), C.byref(c)), body._h)
    return {"min": a.value, "median": b.value, "max": c.value}


def comm_unique_id():
    """128-byte RCCL unique id (rank 0 creates it; the host distributes it to every rank)."""
    buf = (C.c_char * 128)()
    capi.check(capi.lib().tetsim_comm_unique_id(buf))
    return bytes(buf.raw)


def comm_init(body, uid, rank, nranks):
    capi.check(capi.lib().tetsim_comm_init(body._h, bytes(uid), int(rank), int(nranks)), body._h)


def comm_info(body):
    """What RCCL reports for this body's communicator + the halo volume of this partition (include/tetsim.h TetSimCommInfo)."""
    ci = capi.TetSimCommInfo()
    capi.check(capi.lib().tetsim_comm_info(body._h, C.byref(ci)), body._h)
    return {"rccl_ranks": ci.rccl_ranks, "rccl_rank": ci.rccl_rank, "neighbours": ci.neighbours,
            "send_bytes_per_substep": ci.send_bytes_per_substep, "recv_bytes_per_substep": ci.recv_bytes_per_substep,
            "max_message_bytes": ci.max_message_bytes, "loopback": bool(ci.loopback), "p2p": bool(ci.p2p)}


def comm_selftest(body):
    capi.check(capi.lib().tetsim_comm_selftest(body._h), body._h)


def measure_copy_bandwidth(nbytes, reps=20, device=0):
    g = C.c_double()
    capi.check(capi.lib().tetsim_measure_copy_bandwidth(device, int(nbytes), int(reps), C.byref(g)))
    return g.value


def measure_stream_bandwidth(nbytes, kind="copy", reps=20, device=0):
    """GB/s of the tuned streaming probe (include/tetsim.h: tetsim_measure_stream_bandwidth): kind copy (read + write bytes), read, write."""
    g = C.c_double()
    capi.check(capi.lib().tetsim_measure_stream_bandwidth(device, int(nbytes), int(reps), {"copy": 0, "read": 1, "write": 2}[kind], C.byref(g)))
    return g.value


def group_step_n(bodies, n, dt, physicsParams):
    """n substeps of every partition of one decomposition (same choreography as the RCCL path, in-process copies)."""
    arr = (C.c_void_p * len(bodies))(*[b._h for b in bodies])
    capi.check(capi.lib().tetsim_group_step_n(arr, len(bodies), int(n), float(dt), C.byref(make_params(physicsParams))))


def group_visual_vertex_normals(bodies, num_rows):
    """(positions, normals) of the WHOLE visual mesh [num_rows, 3] from the partitions of one process (after group_refresh_final):
    tetsim_group_read_visual_vertex_normals."""
    arr = (C.c_void_p * len(bodies))(*[b._h for b in bodies])
    pos, nrm = np.empty(3 * num_rows, dtype=np.float32), np.empty(3 * num_rows, dtype=np.float32)
    capi.check(capi.lib().tetsim_group_read_visual_vertex_normals(arr, len(bodies), _fp(pos), _fp(nrm)))
    return pos.reshape(-1, 3), nrm.reshape(-1, 3)


def group_refresh_final(bodies):
    """In-process group: every partition's ghost particles get their END-OF-SUBSTEP positions from their owners (what the visual mesh
    of a partition needs at the frame's end; the per-substep halo carries predictions)."""
    arr = (C.c_void_p * len(bodies))(*[b._h for b in bodies])
    capi.check(capi.lib().tetsim_group_refresh_final(arr, len(bodies)))


P2P_BLOB_BYTES = 512


def p2p_export(body):
    """This partition's buffers for the peer-to-peer halo (include/tetsim.h: tetsim_halo_p2p_export): TETSIM_P2P_BLOB_BYTES bytes
    that the host hands to every other rank."""
    buf = (C.c_char * P2P_BLOB_BYTES)()
    capi.check(capi.lib().tetsim_halo_p2p_export(body._h, buf), body._h)
    return bytes(buf.raw)


def p2p_connect(body, blobs):
    """blobs: one per partition, in rank order (a loopback body: its own, alone).  From the next step on the boundary-particle kernel
    stores the halo straight into the neighbours' ghost ranges; every rank must have connected before any of them steps."""
    raw = b"".join(bytes(b) for b in blobs)
    assert len(raw) == P2P_BLOB_BYTES * len(blobs)
    capi.check(capi.lib().tetsim_halo_p2p_connect(body._h, raw, len(blobs)), body._h)


def group_p2p_connect(bodies):
    """All partitions of one decomposition living in this process: switch their halo to peer-to-peer stores."""
    blobs = [p2p_export(b) for b in bodies]
    for b in bodies:
        p2p_connect(b, blobs)


def halo_exchange_local(bodies):
    arr = (C.c_void_p * len(bodies))(*[b._h for b in bodies])
    capi.check(capi.lib().tetsim_halo_exchange_local(arr, len(bodies)))
