"""tetsim_raycast_visual_bvh_device restated in numpy f64 (the definition in include/tetsim.h): plain brute force over all triangles, one
ray at a time -- tests/raycast_ref.py's steps with two more predicates per triangle, the padded slab interval of the triangle's own box.
No tree appears here: the definition is independent of it.  Every multiply and add is a separate f64 operation.

Also the adversarial ray set of tests/test_raycast_bvh_cpu.py and tests/test_gpu_raycast_bvh.py (adversarial_rays) and the axis-aligned
cube surface they use beside the Dragon."""
import numpy as np

import raycast_device_ref
import raycast_ref
from raycast_ref import _cross, _dot

PAD = 2.0 ** -20


def padding(o, centre, radius):
    w = o - centre
    return PAD * (radius + np.sqrt(_dot(w, w)))


def slab(o, d, lo, hi, e):
    """(every axis passes [n], tn [n], tf [n]) of the boxes lo / hi [n, 3] (f64 values of f32 numbers) padded by e, for the ray o + t d."""
    n = len(lo)
    ok = np.ones(n, bool)
    tn, tf = np.full(n, -np.inf), np.full(n, np.inf)
    with np.errstate(all="ignore"):
        for k in range(3):
            L, H = lo[:, k] - e, hi[:, k] + e
            inv = np.float64(1.0) / d[k]
            if d[k] == 0.0 or np.isinf(inv):
                ok &= (L <= o[k]) & (o[k] <= H)
                continue
            t1, t2 = (L - o[k]) * inv, (H - o[k]) * inv
            mn, mx = np.where(t1 < t2, t1, t2), np.where(t1 > t2, t1, t2)
            tn = np.where(mn > tn, mn, tn)
            tf = np.where(mx < tf, mx, tf)
    return ok, tn, tf


def raycast(positions, triangles, origins, directions, near=0.0, far=np.inf, sphere=None, stats=None):
    """raycast_ref.raycast with the definition's two predicates.  stats (a dict, optional) counts over all rays: `accepted`, the hits
    Ray.intersectTriangle and the window accept; `removed`, those of them that are no candidate or lie outside [tn, tf]."""
    P = np.asarray(positions, dtype=np.float32).astype(np.float64).reshape(-1, 3)
    T = np.asarray(triangles, dtype=np.int64).reshape(-1, 3)
    O = np.asarray(origins, dtype=np.float64).reshape(-1, 3)
    D = np.asarray(directions, dtype=np.float64).reshape(-1, 3)
    N, F = np.broadcast_to(np.asarray(near, np.float64), len(O)), np.broadcast_to(np.asarray(far, np.float64), len(O))
    centre, radius = sphere if sphere is not None else raycast_ref.bounding_sphere(P)
    a, b, c = P[T[:, 0]], P[T[:, 1]], P[T[:, 2]]
    e1, e2 = b - a, c - a
    n = _cross(e1, e2)
    lo, hi = np.minimum(np.minimum(a, b), c), np.maximum(np.maximum(a, b), c)
    out = np.zeros(len(O), dtype=raycast_ref.HIT_DTYPE)
    out["body"] = -1
    out["triangle"] = -1
    with np.errstate(all="ignore"):
        for i in range(len(O)):
            o, near_i, far_i = O[i], N[i], F[i]
            if raycast_ref._sphere_culls(o, D[i], near_i, far_i, centre, radius):
                continue
            d = raycast_ref.local_direction(D[i])
            DdN = _dot(d[None, :], n)
            front = DdN < 0
            DdN = -DdN
            diff = o[None, :] - a
            DdQxE2 = -_dot(d[None, :], _cross(diff, e2))
            DdE1xQ = -_dot(d[None, :], _cross(e1, diff))
            QdN = _dot(diff, n)
            ok = front & (DdQxE2 >= 0) & (DdE1xQ >= 0) & (DdQxE2 + DdE1xQ <= DdN) & (QdN >= 0)
            idx = np.flatnonzero(ok)
            if not len(idx):
                continue
            t = QdN[idx] / DdN[idx]
            pt = o[None, :] + d[None, :] * t[:, None]
            w = o[None, :] - pt
            dist = np.sqrt(w[:, 0] * w[:, 0] + w[:, 1] * w[:, 1] + w[:, 2] * w[:, 2])
            keep = (dist >= near_i) & (dist <= far_i)
            idx, dist, pt = idx[keep], dist[keep], pt[keep]
            passes, tn, tf = slab(o, d, lo[idx], hi[idx], padding(o, centre, radius))
            counts = passes & (tn <= tf) & (tn <= dist) & (dist <= tf)
            if stats is not None:
                stats["accepted"] = stats.get("accepted", 0) + len(idx)
                stats["removed"] = stats.get("removed", 0) + int((~counts).sum())
            if not counts.any():
                continue
            idx, dist, pt = idx[counts], dist[counts], pt[counts]
            k = int(np.argmin(dist))                     # the first minimum: the lowest triangle index among equals
            out[i] = (1, 0, idx[k], 0, dist[k], pt[k])
    return out


def raycast_device(positions, triangles, row_body, num_bodies, origins, directions, near=0.0, far=np.inf, bodies=None):
    """The records of the device call: the frame of raycast_device_ref.raycast (invalid rays; a ray with a body is cast against that body
    ALONE, its own rows, triangles and sphere; `triangle` counted in the whole list) around the definition above."""
    P = np.asarray(positions, np.float32).reshape(-1, 3)
    T = np.asarray(triangles, np.int64).reshape(-1, 3)
    O, D = np.asarray(origins, np.float64).reshape(-1, 3), np.asarray(directions, np.float64).reshape(-1, 3)
    N, F = np.broadcast_to(np.asarray(near, np.float64), len(O)), np.broadcast_to(np.asarray(far, np.float64), len(O))
    rb = np.asarray(row_body, np.int64)
    bad = raycast_device_ref.invalid_rays(O, D, N, F, bodies, num_bodies)
    out = np.zeros(len(O), dtype=raycast_ref.HIT_DTYPE)
    out["body"] = -1
    out["triangle"] = -1
    out["hit"][bad] = raycast_device_ref.RAY_INVALID
    good = np.flatnonzero(~bad)
    if bodies is None:
        if len(good):
            h = raycast(P, T, O[good], D[good], N[good], F[good])
            h["body"] = np.where(h["hit"] == 1, rb[T[np.maximum(h["triangle"], 0), 0]], -1)
            out[good] = h
        return out
    B = np.asarray(bodies, np.int64)
    for b in np.unique(B[good]):
        sel = good[B[good] == b]
        rows, tri_at = np.flatnonzero(rb == b), raycast_device_ref.body_triangles(T, rb, b)
        if not len(rows) or not len(tri_at):
            continue                                                             # a miss
        local = np.full(len(P), -1, np.int64)
        local[rows] = np.arange(len(rows))
        h = raycast(P[rows], local[T[tri_at]], O[sel], D[sel], N[sel], F[sel])
        hit = h["hit"] == 1
        h["triangle"][hit] = tri_at[h["triangle"][hit]]
        h["body"][hit] = b
        out[sel] = h
    return out


# ---- the meshes and the adversarial rays ---------------------------------------------------------------------------------------------
def cube_surface(n=2, size=1.0, shift=(0.25, -0.5, 0.125)):
    """(positions [m, 3] f32, triangles [k, 3]) of an axis-aligned cube's surface, n x n squares a face, two triangles each, outward: every
    triangle's box is flat, and many share a plane.  n = 2: 48 triangles."""
    g = np.linspace(0.0, size, n + 1)
    pts, index, tris = [], {}, []

    def vid(p):
        key = tuple(np.round(p, 9))
        if key not in index:
            index[key] = len(pts)
            pts.append(p)
        return index[key]

    for axis in range(3):
        u, v = (axis + 1) % 3, (axis + 2) % 3
        for side, w in ((0, 0.0), (1, size)):
            for i in range(n):
                for j in range(n):
                    q = []
                    for du, dv in ((0, 0), (1, 0), (1, 1), (0, 1)):
                        p = np.zeros(3)
                        p[axis], p[u], p[v] = w, g[i + du], g[j + dv]
                        q.append(vid(p))
                    if side == 0:
                        q = q[::-1]
                    tris += [[q[0], q[1], q[2]], [q[0], q[2], q[3]]]
    return (np.asarray(pts) + np.asarray(shift)).astype(np.float32), np.asarray(tris, np.int32)


ADVERSARIAL_SEED = 2025
ADVERSARIAL_PER_KIND = 40


def adversarial_rays(positions, triangles, seed=ADVERSARIAL_SEED, per_kind=ADVERSARIAL_PER_KIND):
    """(origins, directions, near, far) [8 * per_kind]: aimed at vertices, edge midpoints and centroids from the front; lying in a triangle's
    plane tilted by 1e-9; from 1e4 away; axis-aligned with exact zeros; from inside the body; with `near` behind the first surface."""
    rng = np.random.default_rng(seed)
    P = np.asarray(positions, np.float32).astype(np.float64).reshape(-1, 3)
    T = np.asarray(triangles, np.int64).reshape(-1, 3)
    c, r = raycast_ref.bounding_sphere(P)
    pick = lambda: T[rng.integers(0, len(T), per_kind)]   # noqa: E731
    normal = lambda t: _unit(_cross(P[t[:, 1]] - P[t[:, 0]], P[t[:, 2]] - P[t[:, 0]]))   # noqa: E731

    def _unit(v):
        return v / np.linalg.norm(v, axis=1, keepdims=True)

    def toward(target, t, dist):
        """from the front of triangle t, a little off its normal, aimed exactly at `target`"""
        o = target + dist * _unit(normal(t) + 0.2 * rng.standard_normal((len(t), 3)))
        return o, _unit(target - o)

    O, D, N, F = [], [], [], []

    def add(o, d, near=0.0, far=np.inf):
        O.append(o), D.append(d)
        N.append(np.broadcast_to(np.asarray(near, np.float64), len(o)).copy()), F.append(np.broadcast_to(np.asarray(far, np.float64), len(o)).copy())

    t = pick()
    add(*toward(P[t[:, 0]], t, 2.0 * r))                                           # vertices
    t = pick()
    add(*toward((P[t[:, 0]] + P[t[:, 1]]) * 0.5, t, 2.0 * r))                      # edge midpoints
    t = pick()
    cen = (P[t[:, 0]] + P[t[:, 1]] + P[t[:, 2]]) / 3.0
    add(*toward(cen, t, 2.0 * r))                                                  # centroids
    t = pick()                                                                     # in the triangle's plane, tilted by 1e-9 towards its front
    cen = (P[t[:, 0]] + P[t[:, 1]] + P[t[:, 2]]) / 3.0
    along = _unit(P[t[:, 1]] - P[t[:, 0]])
    o = cen - 2.0 * r * along + 2.0 * r * 1e-9 * normal(t)
    add(o, _unit(cen - o))
    t = pick()
    cen = (P[t[:, 0]] + P[t[:, 1]] + P[t[:, 2]]) / 3.0
    add(*toward(cen, t, 1e4))                                                      # origins 1e4 away
    t = pick()                                                                     # axis-aligned directions with exact zeros, at a point of the triangle
    w = rng.dirichlet([1.0, 1.0, 1.0], per_kind)
    target = w[:, :1] * P[t[:, 0]] + w[:, 1:2] * P[t[:, 1]] + w[:, 2:] * P[t[:, 2]]
    axis = np.argmax(np.abs(normal(t)), axis=1)
    d = np.zeros((per_kind, 3))
    d[np.arange(per_kind), axis] = -np.sign(normal(t)[np.arange(per_kind), axis])
    add(target - 2.0 * r * d, d)
    inside = c + 0.05 * r * rng.standard_normal((per_kind, 3))                     # an origin inside the body
    add(inside, _unit(rng.standard_normal((per_kind, 3))))
    t = pick()                                                                     # near behind the first surface: the second must win
    cen = (P[t[:, 0]] + P[t[:, 1]] + P[t[:, 2]]) / 3.0
    o, d = toward(cen, t, 2.0 * r)
    first = raycast_ref.raycast(P, T, o, d)
    near = np.where(first["hit"] == 1, first["distance"] + 1e-6 * r, 0.0)
    add(o, d, near)
    return np.concatenate(O), np.concatenate(D), np.concatenate(N), np.concatenate(F)
