"""tetsim_closest_visual_device restated in numpy f64 (the definition in include/tetsim.h): plain brute force over all triangles, one query
at a time -- three.js r160's Triangle.closestPointToPoint per triangle (tests/test_closest_cpu.py pins it to fixtures recorded from three
itself, bit for bit), the squared distance, the padded box bound of the triangle's own corners, the lexicographic winner.  No tree appears
in the definition.  Every multiply and add is a separate f64 operation, sums run left to right.

Also: `traverse`, a walk of the library's own tree topology (tetsim_prep_bvh) under the skip rules the header allows, with which the CPU
test shows that a conservative tree reproduces the definition; and the adversarial query set both test files use."""
import numpy as np

import raycast_device_ref
import raycast_ref
from raycast_ref import _dot

PAD = 2.0 ** -20
CLOSEST_INVALID = -1
CLOSEST_DTYPE = np.dtype([("found", "<i4"), ("body", "<i4"), ("triangle", "<i4"), ("region", "<i4"), ("distance", "<f8"), ("point", "<f8", (3,)),
                          ("v", "<f8"), ("w", "<f8")])
FACE, VERTEX_A, VERTEX_B, VERTEX_C, EDGE_AB, EDGE_AC, EDGE_BC = range(7)


def closest_on_triangles(a, b, c, p):
    """Triangle.closestPointToPoint for the triangles a, b, c [n, 3] and the point p [3] (or [n, 3]): (q [n, 3], region [n], v [n], w [n]),
    q = a + v (b - a) + w (c - a) in exact terms.  All seven exits are evaluated for every triangle and the first that applies, in the
    method's order, is chosen -- the arithmetic of each is the method's own."""
    p = np.broadcast_to(np.asarray(p, np.float64), a.shape)
    with np.errstate(all="ignore"):
        ab, ac, ap = b - a, c - a, p - a
        d1, d2 = _dot(ab, ap), _dot(ac, ap)
        bp = p - b
        d3, d4 = _dot(ab, bp), _dot(ac, bp)
        vc = d1 * d4 - d3 * d2
        cp = p - c
        d5, d6 = _dot(ab, cp), _dot(ac, cp)
        vb = d5 * d2 - d1 * d6
        va = d3 * d6 - d5 * d4
        v_ab = d1 / (d1 - d3)
        w_ac = d2 / (d2 - d6)
        w_bc = (d4 - d3) / ((d4 - d3) + (d5 - d6))
        denom = 1.0 / (va + vb + vc)
        v_f, w_f = vb * denom, vc * denom
        conds = [(d1 <= 0) & (d2 <= 0), (d3 >= 0) & (d4 <= d3), (vc <= 0) & (d1 >= 0) & (d3 <= 0), (d6 >= 0) & (d5 <= d6),
                 (vb <= 0) & (d2 >= 0) & (d6 <= 0), (va <= 0) & ((d4 - d3) >= 0) & ((d5 - d6) >= 0)]
        order = [VERTEX_A, VERTEX_B, EDGE_AB, VERTEX_C, EDGE_AC, EDGE_BC]
        zero, one = np.zeros(len(a)), np.ones(len(a))
        answers = {VERTEX_A: (a, zero, zero), VERTEX_B: (b, one, zero), VERTEX_C: (c, zero, one),
                   EDGE_AB: (a + ab * v_ab[:, None], v_ab, zero), EDGE_AC: (a + ac * w_ac[:, None], zero, w_ac),
                   EDGE_BC: (b + (c - b) * w_bc[:, None], 1.0 - w_bc, w_bc),
                   FACE: ((a + ab * v_f[:, None]) + ac * w_f[:, None], v_f, w_f)}
    q, v, w = (x.copy() for x in answers[FACE])
    region = np.full(len(a), FACE, np.int32)
    for cond, r in reversed(list(zip(conds, order))):        # the earliest exit wins: apply the later ones first
        q[cond], v[cond], w[cond], region[cond] = answers[r][0][cond], answers[r][1][cond], answers[r][2][cond], r
    return q, region, v, w


def dist2(p, q):
    w = np.asarray(p, np.float64) - q
    return w[..., 0] * w[..., 0] + w[..., 1] * w[..., 1] + w[..., 2] * w[..., 2]


def padding(p, centre, radius):
    w = p - centre
    return PAD * (radius + np.sqrt(_dot(w, w)))


def box_bound(p, lo, hi, e):
    """lb [n] of the boxes lo / hi [n, 3] (f64 values of f32 numbers) padded by e, for the point p"""
    g = np.maximum(np.maximum((lo - e) - p, p - (hi + e)), 0.0)
    return g[..., 0] * g[..., 0] + g[..., 1] * g[..., 1] + g[..., 2] * g[..., 2]


def corners(positions, triangles):
    P = np.asarray(positions, dtype=np.float32).astype(np.float64).reshape(-1, 3)
    T = np.asarray(triangles, dtype=np.int64).reshape(-1, 3)
    return P, T, P[T[:, 0]], P[T[:, 1]], P[T[:, 2]]


def empty_records(n):
    out = np.zeros(n, dtype=CLOSEST_DTYPE)
    out["body"] = out["triangle"] = out["region"] = -1
    return out


def closest(positions, triangles, points, max_distance=np.inf, sphere=None, stats=None):
    """The definition for one mesh and valid queries: CLOSEST_DTYPE records (body 0 where found).  stats (a dict, optional) counts over all
    queries: `within`, the triangles with d2 <= max_distance^2; `rejected`, those of them whose box bound exceeds d2."""
    P, T, a, b, c = corners(positions, triangles)
    Q = np.asarray(points, np.float64).reshape(-1, 3)
    M = np.broadcast_to(np.asarray(max_distance, np.float64), len(Q))
    centre, radius = sphere if sphere is not None else raycast_ref.bounding_sphere(P)
    lo, hi = np.minimum(np.minimum(a, b), c), np.maximum(np.maximum(a, b), c)
    out = empty_records(len(Q))
    if not len(T):
        return out
    with np.errstate(all="ignore"):
        for i in range(len(Q)):
            p = Q[i]
            q, region, v, w = closest_on_triangles(a, b, c, p)
            d2 = dist2(p, q)
            lb = box_bound(p, lo, hi, padding(p, centre, radius))
            within = d2 <= M[i] * M[i]
            counts = within & (lb <= d2)
            if stats is not None:
                stats["within"] = stats.get("within", 0) + int(within.sum())
                stats["rejected"] = stats.get("rejected", 0) + int((within & ~counts).sum())
            idx = np.flatnonzero(counts)
            if not len(idx):
                continue
            k = idx[int(np.argmin(d2[idx]))]                 # the first minimum: the lowest triangle index among equals
            out[i] = (1, 0, k, region[k], np.sqrt(d2[k]), q[k], v[k], w[k])
    return out


def invalid_queries(points, max_distance, bodies=None, num_bodies=1):
    """[count] bool: what the device refuses"""
    Q = np.asarray(points, np.float64).reshape(-1, 3)
    M = np.broadcast_to(np.asarray(max_distance, np.float64), len(Q))
    with np.errstate(all="ignore"):
        bad = ~np.isfinite(Q).all(axis=1) | np.isnan(M) | (M < 0.0)
    if bodies is not None:
        b = np.asarray(bodies, np.int64)
        bad |= (b < 0) | (b >= num_bodies)
    return bad


def closest_device(positions, triangles, row_body, num_bodies, points, max_distance=np.inf, bodies=None, stats=None):
    """The records of the device call.  bodies=None: the definition over the whole mesh, body = that of the winner's first row.  Otherwise a
    query is answered by its body ALONE -- its own rows, triangles and sphere --, `triangle` counted in the whole list."""
    P = np.asarray(positions, np.float32).reshape(-1, 3)
    T = np.asarray(triangles, np.int64).reshape(-1, 3)
    Q = np.asarray(points, np.float64).reshape(-1, 3)
    M = np.broadcast_to(np.asarray(max_distance, np.float64), len(Q))
    rb = np.asarray(row_body, np.int64)
    bad = invalid_queries(Q, M, bodies, num_bodies)
    out = empty_records(len(Q))
    out["found"][bad] = CLOSEST_INVALID
    good = np.flatnonzero(~bad)
    if bodies is None:
        if len(good):
            h = closest(P, T, Q[good], M[good], stats=stats)
            h["body"] = np.where(h["found"] == 1, rb[T[np.maximum(h["triangle"], 0), 0]] if len(T) else -1, -1)
            out[good] = h
        return out
    B = np.asarray(bodies, np.int64)
    for b in np.unique(B[good]):
        sel = good[B[good] == b]
        rows, tri_at = np.flatnonzero(rb == b), raycast_device_ref.body_triangles(T, rb, b)
        if not len(rows) or not len(tri_at):
            continue                                                             # found = 0
        local = np.full(len(P), -1, np.int64)
        local[rows] = np.arange(len(rows))
        h = closest(P[rows], local[T[tri_at]], Q[sel], M[sel], stats=stats)     # the body ALONE
        hit = h["found"] == 1
        h["triangle"][hit] = tri_at[h["triangle"][hit]]
        h["body"][hit] = b
        out[sel] = h
    return out


# ---- a walk of the library's tree under the skip rules of the header ------------------------------------------------------------------
def traverse(positions, triangles, order, ranges, depth, points, max_distance=np.inf, sphere=None, stats=None):
    """One body's tree (tetsim_prep_bvh: order [ntri], ranges [nodes, 2] into order, depth) walked for every query, nearer child first.  A
    node is skipped only if it is empty, lb_node > max_distance^2, or a best exists and lb_node > d2_best (strictly); at a leaf every
    triangle is tested with the box of its own corners.  stats counts `boxes` and `triangles` tested over all queries."""
    P, T, a, b, c = corners(positions, triangles)
    Q = np.asarray(points, np.float64).reshape(-1, 3)
    M = np.broadcast_to(np.asarray(max_distance, np.float64), len(Q))
    centre, radius = sphere if sphere is not None else raycast_ref.bounding_sphere(P)
    order, ranges = np.asarray(order, np.int64), np.asarray(ranges, np.int64)
    tlo, thi = np.minimum(np.minimum(a, b), c), np.maximum(np.maximum(a, b), c)
    nodes = len(ranges)
    nlo, nhi = np.full((nodes, 3), np.inf), np.full((nodes, 3), -np.inf)       # a node's box: the exact min / max of its triangles' corners
    for i in range(nodes - 1, 0, -1):
        if i >= (1 << depth):
            ids = order[ranges[i, 0]:ranges[i, 1]]
            if len(ids):
                nlo[i], nhi[i] = tlo[ids].min(axis=0), thi[ids].max(axis=0)
        else:
            nlo[i], nhi[i] = np.minimum(nlo[2 * i], nlo[2 * i + 1]), np.maximum(nhi[2 * i], nhi[2 * i + 1])
    nlo, nhi = nlo.astype(np.float32).astype(np.float64), nhi.astype(np.float32).astype(np.float64)   # (exact: they are f32 values)
    out = empty_records(len(Q))
    boxes = tris = 0
    with np.errstate(all="ignore"):
        for i in range(len(Q)):
            p, max2, e = Q[i], M[i] * M[i], padding(Q[i], centre, radius)
            best = None                                                          # (d2, triangle)

            def enter(node):
                nonlocal boxes
                if nlo[node, 0] > nhi[node, 0]:
                    return None
                boxes += 1
                lb = float(box_bound(p, nlo[node], nhi[node], e))
                if lb > max2 or (best is not None and lb > best[0]):
                    return None
                return lb

            stack = [1] if nodes > 1 and enter(1) is not None else []
            while stack:
                node = stack.pop()
                if node < (1 << depth):
                    kids = [(lb, k) for k in (2 * node, 2 * node + 1) for lb in [enter(k)] if lb is not None]
                    kids.sort(key=lambda x: x[0])
                    # (a child pushed now is looked at again when it is popped: the best may have improved meanwhile)
                    stack += [k for _, k in reversed(kids)]
                    continue
                lb_now = float(box_bound(p, nlo[node], nhi[node], e))
                if best is not None and lb_now > best[0]:
                    continue
                ids = order[ranges[node, 0]:ranges[node, 1]]
                tris += len(ids)
                q, region, v, w = closest_on_triangles(a[ids], b[ids], c[ids], p)
                d2 = dist2(p, q)
                lb = box_bound(p, tlo[ids], thi[ids], e)
                for j in np.flatnonzero((lb <= d2) & (d2 <= max2)):
                    if best is None or d2[j] < best[0] or (d2[j] == best[0] and ids[j] < best[1]):
                        best = (float(d2[j]), int(ids[j]))
                        out[i] = (1, 0, ids[j], region[j], np.sqrt(d2[j]), q[j], v[j], w[j])
    if stats is not None:
        stats["boxes"] = stats.get("boxes", 0) + boxes
        stats["triangles"] = stats.get("triangles", 0) + tris
    return out


# ---- the adversarial queries -----------------------------------------------------------------------------------------------------------
ADVERSARIAL_SEED = 2026
ADVERSARIAL_PER_KIND = 24
ADVERSARIAL_KINDS = ("vertex", "edge_midpoint", "centroid", "off_surface_1e-9", "far_1e4", "centre", "across_an_edge", "max_below", "max_above")


def shared_edges(triangles, limit, rng):
    """[(triangle, triangle, row, row)]: up to `limit` pairs of triangles that share an edge, chosen by rng"""
    T = np.asarray(triangles, np.int64).reshape(-1, 3)
    seen, pairs = {}, []
    for t in rng.permutation(len(T)):
        for k in range(3):
            e = (int(min(T[t, k], T[t, (k + 1) % 3])), int(max(T[t, k], T[t, (k + 1) % 3])))
            if e in seen and seen[e] != t:
                pairs.append((seen[e], int(t), e[0], e[1]))
            seen[e] = int(t)
        if len(pairs) >= limit:
            break
    return pairs[:limit]


def adversarial_queries(positions, triangles, seed=ADVERSARIAL_SEED, per_kind=ADVERSARIAL_PER_KIND):
    """(points, max_distance) [len(ADVERSARIAL_KINDS) * per_kind]: on vertices, on edge midpoints, at centroids; 1e-9 off the surface along
    the normal; 1e4 away; at and around the body's centre; off a shared edge along the sum of the two triangles' normals, which is
    equidistant from both (exactly so across the edge of an axis-aligned cube: the lowest index must win); with max_distance a
    hair below and a hair above the true distance."""
    rng = np.random.default_rng(seed)
    P, T, a, b, c = corners(positions, triangles)
    centre, r = raycast_ref.bounding_sphere(P)
    n = per_kind

    def unit(v):
        with np.errstate(all="ignore"):
            length = np.linalg.norm(v, axis=-1, keepdims=True)
            return np.where(length > 0, v / np.where(length > 0, length, 1.0), 0.0)

    normal = unit(np.cross(b - a, c - a))
    pick = lambda: rng.integers(0, len(T), n)   # noqa: E731
    pts, mx = [], []

    def add(p, m=np.inf):
        pts.append(np.asarray(p, np.float64).reshape(-1, 3))
        mx.append(np.broadcast_to(np.asarray(m, np.float64), len(pts[-1])).copy())

    t = pick()
    add(P[T[t, rng.integers(0, 3, n)]])                                          # exactly on a vertex
    t, k = pick(), rng.integers(0, 3, n)
    add((P[T[t, k]] + P[T[t, (k + 1) % 3]]) * 0.5)                               # edge midpoints
    t = pick()
    add((a[t] + b[t] + c[t]) / 3.0)                                              # centroids
    t = pick()
    wgt = rng.dirichlet([1.0, 1.0, 1.0], n)
    on = wgt[:, :1] * a[t] + wgt[:, 1:2] * b[t] + wgt[:, 2:] * c[t]
    add(on + 1e-9 * normal[t] * np.where(rng.random(n) < 0.5, -1.0, 1.0)[:, None])   # 1e-9 off the surface, either side
    add(centre + 1e4 * unit(rng.standard_normal((n, 3))))                        # 1e4 away
    add(np.concatenate([centre[None, :], centre + 0.05 * r * rng.standard_normal((n - 1, 3))]))   # the body's centre, and around it
    pairs = shared_edges(T, n, rng)
    across = []
    for j in range(n):
        t0, t1, r0, r1 = pairs[j % len(pairs)]
        s = rng.random()
        across.append((P[r0] * (1.0 - s) + P[r1] * s if j % 2 else (P[r0] + P[r1]) * 0.5) + 0.25 * r * rng.random() * (normal[t0] + normal[t1]))
    add(np.asarray(across))
    probe = centre + (0.6 + rng.random((2 * n, 1))) * r * unit(rng.standard_normal((2 * n, 3)))
    true = closest(P, T, probe)["distance"]
    add(probe[:n], true[:n] * (1.0 - 1e-12))                                     # a hair below the true distance: nothing is found
    add(probe[n:], true[n:] * (1.0 + 1e-12))                                     # a hair above: the same answer as without a limit
    return np.concatenate(pts), np.concatenate(mx)


# ---- the query sets of tests/test_gpu_closest.py -----------------------------------------------------------------------------------------
BATCH_QUERIES = {2: (334, 121), 5: (333, 122), 12: (333, 123)}                   # lattice -> (queries, seed): 1,000 in all, as the batch's rays
STREAM_QUERIES = (512, 151)                                                      # on lattice 5


def seeded_points(pos, n, seed):
    """(points, max_distance) [n]: a row of pos plus an offset of up to one bounding radius in a random direction (every eighth: no offset, the
    point sits on the surface); every fourth has a max_distance of 0.2 .. 1.2 offsets, so that some of them find nothing."""
    rng = np.random.default_rng(seed)
    P = np.asarray(pos, np.float32).astype(np.float64).reshape(-1, 3)
    _, r = raycast_ref.bounding_sphere(P)
    u = rng.standard_normal((n, 3))
    u /= np.linalg.norm(u, axis=1, keepdims=True)
    length = r * rng.random(n)
    length[::8] = 0.0
    points = P[rng.integers(0, len(P), n)] + length[:, None] * u
    limit = np.full(n, np.inf)
    limit[1::4] = length[1::4] * rng.uniform(0.2, 1.2, len(limit[1::4]))
    return points, limit


def batch_queries(per_body=None, shuffle_seed=9):
    """(points, max_distance, bodies) of the batch tests: every body's queries around ITS rest surface (raycast_device_ref.batch_bodies), shuffled"""
    bodies = raycast_device_ref.batch_bodies()
    p, m, b = [], [], []
    for k, n in enumerate(raycast_device_ref.LATTICES):
        count, seed = BATCH_QUERIES[n] if per_body is None else per_body[n]
        pk, mk = seeded_points(bodies[k][4], count, seed)
        p.append(pk), m.append(mk), b.append(np.full(count, k, np.int32))
    p, m, b = np.concatenate(p), np.concatenate(m), np.concatenate(b)
    perm = np.random.default_rng(shuffle_seed).permutation(len(p))
    return p[perm], m[perm], b[perm]


def found_share_ok(found):
    """a set of answers means something: most queries find a point, and some find none"""
    found = np.asarray(found)
    return int((found == 1).sum()) >= 0.5 * len(found) and int((found == 0).sum()) >= 0.02 * len(found)
