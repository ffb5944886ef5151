"""three.js r160 ray cast and bounding sphere of an indexed mesh, restated in numpy f64 (the definition in include/tetsim.h:
tetsim_raycast_visual, tetsim_read_visual_bounding_sphere).  Every multiply and add is a separate f64 operation, sums run left
to right.  tests/test_raycast_cpu.py pins this file to fixtures recorded from three itself, bit for bit.

What three does for `new Raycaster(origin, direction, near, far).intersectObject(mesh)` on a Mesh with an identity world
matrix and a front-side material (Mesh.raycast, checkGeometryIntersection, Ray.intersectTriangle):
  1. the bounding-sphere cull, with the ray recast by `near` and the direction AS GIVEN;
  2. the ray is taken to the mesh's local space: the origin is unchanged, the direction goes through
     Vector3.transformDirection, which NORMALISES it (d * (1 / (|d| || 1))) -- a unit vector may change in its last bits;
  3. per triangle Ray.intersectTriangle with that local direction, back faces culled; distance = |origin - point|, kept iff
     near <= distance <= far;
  4. a stable sort by distance: the first entry is the smallest distance, the lowest triangle index among equals.
"""
import numpy as np

HIT_DTYPE = np.dtype([("hit", "<i4"), ("body", "<i4"), ("triangle", "<i4"), ("reserved", "<i4"), ("distance", "<f8"), ("point", "<f8", (3,))])


def _dot(u, v):
    return u[..., 0] * v[..., 0] + u[..., 1] * v[..., 1] + u[..., 2] * v[..., 2]


def _cross(a, b):
    return np.stack([a[..., 1] * b[..., 2] - a[..., 2] * b[..., 1], a[..., 2] * b[..., 0] - a[..., 0] * b[..., 2],
                     a[..., 0] * b[..., 1] - a[..., 1] * b[..., 0]], axis=-1)


def bounding_sphere(positions):
    """BufferGeometry.computeBoundingSphere(): (centre[3], radius) in f64 of f32 positions [n, 3]."""
    P = np.asarray(positions, dtype=np.float32).astype(np.float64).reshape(-1, 3)
    centre = (P.min(axis=0) + P.max(axis=0)) * 0.5
    d = centre[None, :] - P
    r2 = max(0.0, float((d[:, 0] * d[:, 0] + d[:, 1] * d[:, 1] + d[:, 2] * d[:, 2]).max()))
    return centre, float(np.sqrt(r2))


def _sphere_culls(o, d, near, far, centre, radius):
    """Mesh.raycast's first test: True when three gives up before it looks at a triangle."""
    o2 = o + d * near                                   # Ray.recast(near) = at(near)
    radius2 = radius * radius
    v = o2 - centre
    if _dot(v, v) <= radius2:                           # Sphere.containsPoint
        return False
    v = centre - o2                                     # Ray.intersectSphere
    tca = _dot(v, d)
    d2 = _dot(v, v) - tca * tca
    if d2 > radius2:
        return True
    thc = np.sqrt(radius2 - d2)
    t0, t1 = tca - thc, tca + thc
    if t1 < 0:
        return True
    at = o2 + d * (t1 if t0 < 0 else t0)
    w = o2 - at                                         # distanceToSquared
    span = far - near
    return bool(_dot(w, w) > span * span)


def local_direction(d):
    """Vector3.transformDirection by the identity: the direction normalised as three does it."""
    length = np.sqrt(d[0] * d[0] + d[1] * d[1] + d[2] * d[2])
    if length == 0 or length != length:
        length = 1.0
    return d * (1.0 / length)


def raycast(positions, triangles, origins, directions, near=0.0, far=np.inf, sphere=None):
    """First hit of every ray: structured array (HIT_DTYPE; body 0 on a hit; a miss is hit 0, body -1, triangle -1, zeros)."""
    P = np.asarray(positions, dtype=np.float32).astype(np.float64).reshape(-1, 3)
    T = np.asarray(triangles, dtype=np.int64).reshape(-1, 3)
    O = np.asarray(origins, dtype=np.float64).reshape(-1, 3)
    D = np.asarray(directions, dtype=np.float64).reshape(-1, 3)
    N, F = np.broadcast_to(np.asarray(near, np.float64), len(O)), np.broadcast_to(np.asarray(far, np.float64), len(O))
    centre, radius = sphere if sphere is not None else bounding_sphere(P)
    a = P[T[:, 0]]
    e1, e2 = P[T[:, 1]] - a, P[T[:, 2]] - a
    n = _cross(e1, e2)
    out = np.zeros(len(O), dtype=HIT_DTYPE)
    out["body"] = -1
    out["triangle"] = -1
    with np.errstate(all="ignore"):
        for i in range(len(O)):
            o, near_i, far_i = O[i], N[i], F[i]
            if _sphere_culls(o, D[i], near_i, far_i, centre, radius):
                continue
            d = local_direction(D[i])
            DdN = _dot(d[None, :], n)
            front = DdN < 0                              # DdN > 0: back face, culled; == 0: parallel
            DdN = -DdN                                   # sign = -1
            diff = o[None, :] - a
            DdQxE2 = -_dot(d[None, :], _cross(diff, e2))
            DdE1xQ = -_dot(d[None, :], _cross(e1, diff))
            QdN = _dot(diff, n)                          # -sign * diff.n
            ok = front & (DdQxE2 >= 0) & (DdE1xQ >= 0) & (DdQxE2 + DdE1xQ <= DdN) & (QdN >= 0)
            idx = np.flatnonzero(ok)
            if not len(idx):
                continue
            t = QdN[idx] / DdN[idx]
            pt = o[None, :] + d[None, :] * t[:, None]
            w = o[None, :] - pt
            dist = np.sqrt(w[:, 0] * w[:, 0] + w[:, 1] * w[:, 1] + w[:, 2] * w[:, 2])
            keep = (dist >= near_i) & (dist <= far_i)
            if not keep.any():
                continue
            idx, dist, pt = idx[keep], dist[keep], pt[keep]
            k = int(np.argmin(dist))                     # the first minimum: the lowest triangle index among equals
            out[i] = (1, 0, idx[k], 0, dist[k], pt[k])
    return out
