"""tetsim_raycast_visual_device / tetsim_visual_bounding_spheres_device restated over tests/raycast_ref.py (include/tetsim.h: "range
sensors"): a ray with a body is cast against that body's own rows and triangles by raycast_ref.raycast -- literally the body alone --,
the triangle counted in the whole list; an invalid ray gets hit -1.  Also the ray sets of tests/test_gpu_raycast_device.py, defined
here so that tests/test_raycast_device_cpu.py can hold every one of them to the hit-share condition without a GPU."""
import numpy as np

import raycast_ref
from tetsim_amd import boundary_surface, make_lattice

RAY_INVALID = -1
LATTICES = (2, 5, 12)          # 48, 300, 1,728 boundary triangles: below one tile of 256, just over one, several with a ragged end
MIN_HIT_SHARE, MIN_MISS_SHARE = 0.25, 0.02


def seeded_rays(pos, n, seed):
    """tests/test_gpu_raycast.py: from a sphere of three radii aimed at a point inside the bounding sphere, and straight at a vertex."""
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


def invalid_rays(origins, directions, near, far, bodies=None, num_bodies=1):
    """[count] bool: what the device refuses (check_rays' conditions, and a body outside [0, num_bodies))."""
    O, D = np.asarray(origins, np.float64).reshape(-1, 3), np.asarray(directions, np.float64).reshape(-1, 3)
    N, F = np.broadcast_to(np.asarray(near, np.float64), len(O)), np.broadcast_to(np.asarray(far, np.float64), len(O))
    with np.errstate(all="ignore"):
        bad = ~(np.isfinite(O).all(axis=1) & np.isfinite(D).all(axis=1))
        bad |= (D == 0.0).all(axis=1)
        bad |= np.isnan(N) | np.isnan(F) | (N < 0.0) | (F < N)
    if bodies is not None:
        b = np.asarray(bodies, np.int64)
        bad |= (b < 0) | (b >= num_bodies)
    return bad


def body_triangles(triangles, row_body, b):
    """positions in the list of the triangles of body b (the body of a triangle: that of its rows), in list order"""
    T = np.asarray(triangles, np.int64).reshape(-1, 3)
    return np.flatnonzero(np.asarray(row_body)[T[:, 0]] == b)


def bounding_spheres(positions, row_body, num_bodies):
    """[num_bodies, 4]: raycast_ref.bounding_sphere of every body's rows; a body without rows: zeros."""
    out = np.zeros((num_bodies, 4), np.float64)
    for b in range(num_bodies):
        rows = np.flatnonzero(np.asarray(row_body) == b)
        if len(rows):
            c, r = raycast_ref.bounding_sphere(np.asarray(positions)[rows])
            out[b] = [c[0], c[1], c[2], r]
    return out


def raycast(positions, triangles, row_body, num_bodies, origins, directions, near=0.0, far=np.inf, bodies=None):
    """HIT_DTYPE records of the device call.  bodies=None: raycast_ref.raycast on the whole mesh, body = that of the triangle's first row."""
    P = np.asarray(positions, np.float32).reshape(-1, 3)
    T = np.asarray(triangles, np.int64).reshape(-1, 3)
    O, D = np.asarray(origins, np.float64).reshape(-1, 3), np.asarray(directions, np.float64).reshape(-1, 3)
    N, F = np.broadcast_to(np.asarray(near, np.float64), len(O)), np.broadcast_to(np.asarray(far, np.float64), len(O))
    rb = np.asarray(row_body, np.int64)
    bad = invalid_rays(O, D, N, F, bodies, num_bodies)
    out = np.zeros(len(O), dtype=raycast_ref.HIT_DTYPE)
    out["body"] = -1
    out["triangle"] = -1
    out["hit"][bad] = RAY_INVALID
    good = np.flatnonzero(~bad)
    if bodies is None:
        if len(good):
            h = raycast_ref.raycast(P, T, O[good], D[good], N[good], F[good])
            h["body"] = np.where(h["hit"] == 1, rb[T[np.maximum(h["triangle"], 0), 0]], -1)
            out[good] = h
        return out
    B = np.asarray(bodies, np.int64)
    for b in np.unique(B[good]):
        sel = good[B[good] == b]
        rows, tri_at = np.flatnonzero(rb == b), body_triangles(T, rb, b)
        if not len(rows) or not len(tri_at):
            continue                                                             # a miss
        local = np.full(len(P), -1, np.int64)
        local[rows] = np.arange(len(rows))
        h = raycast_ref.raycast(P[rows], local[T[tri_at]], O[sel], D[sel], N[sel], F[sel])   # the body ALONE
        hit = h["hit"] == 1
        h["triangle"][hit] = tri_at[h["triangle"][hit]]
        h["body"][hit] = b
        out[sel] = h
    return out


# ---- the fixtures and ray sets of the GPU tests ---------------------------------------------------------------------------
def lattice_surface(n):
    """(verts, tets, visVerts, visTriIds, rest visual positions) of make_lattice(n) with its boundary as the visual mesh."""
    v, t = make_lattice(n)
    vis, tris = boundary_surface(t, len(v), v)
    w = np.concatenate([vis[:, 1:4], (np.float32(1) - vis[:, 1] - vis[:, 2] - vis[:, 3])[:, None]], axis=1)
    rest = v[t[vis[:, 0].astype(np.int64), np.argmax(w, axis=1)]]                # every row sits on a particle (one weight is 1)
    return v, t, vis, tris, rest


BATCH_SHIFTS = ((-0.25, 0.0, 0.0), (0.0, 0.25, 0.125), (0.25, 0.0, -0.125))      # the three lattices overlap in space; exact in f32
BATCH_RAYS = {2: (334, 21), 5: (333, 22), 12: (333, 23)}                         # lattice -> (rays, seed): 1,000 in all
COUNT_RAYS = (7000, 10, 31)                                                      # on lattice 2: 7,000 rays, ten times over, shuffled (count_rays)
COUNTS = (0, 1, 63, 64, 65, 257, 70000)
INVALID_RAYS = (96, 41)                                                          # on the batch, body by body as BATCH_RAYS
STREAM_RAYS = (512, 51)                                                          # on lattice 5


def batch_bodies():
    """[(verts, tets, visVerts, visTriIds, rest visual positions)] of the three-lattice batch, shifted as BATCH_SHIFTS"""
    out = []
    for n, s in zip(LATTICES, BATCH_SHIFTS):
        v, t, vis, tris, rest = lattice_surface(n)
        s = np.asarray(s, np.float32)
        out.append(((v + s).astype(np.float32), t, vis, tris, (rest + s).astype(np.float32)))
    return out


def batch_rays(per_body=None, shuffle_seed=7):
    """(origins, directions, bodies) of the batch test: every body's rays aimed at ITS rest surface, then shuffled."""
    bodies = batch_bodies()
    o, d, b = [], [], []
    for k, n in enumerate(LATTICES):
        count, seed = BATCH_RAYS[n] if per_body is None else per_body[n]
        ok, dk = seeded_rays(bodies[k][4], count, seed)
        o.append(ok), d.append(dk), b.append(np.full(count, k, np.int32))
    o, d, b = np.concatenate(o), np.concatenate(d), np.concatenate(b)
    perm = np.random.default_rng(shuffle_seed).permutation(len(o))
    return o[perm], d[perm], b[perm]


def count_rays():
    """(origins, directions, index of each in the base set): the 70,000 rays of the counts test, every smaller count a prefix.  Ten shuffled
    copies of 7,000 rays, so that the CPU reference of the whole set costs a tenth."""
    base, copies, seed = COUNT_RAYS
    o, d = seeded_rays(lattice_surface(2)[4], base, seed)
    at = np.random.default_rng(seed + 1).permutation(base * copies) % base
    return o[at], d[at], at


def hit_share_ok(hit):
    hit = np.asarray(hit)
    n = len(hit)
    return int((hit == 1).sum()) >= MIN_HIT_SHARE * n and int((hit == 0).sum()) >= MIN_MISS_SHARE * n
