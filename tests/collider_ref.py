"""numpy restatement of the kinematic colliders (include/tetsim.h tetsim_set_colliders) and the composed oracle built on it.

Colliders act last on a particle, before its velocity, so "oracle substep, then colliders on its result" is "the library's substep
with colliders": the oracle (oracle/) stays as it is and checks the device bit for bit.

  collide_f32: the polar solver's arithmetic (IEEE f32, every operation rounded, correctly rounded / and sqrt) -- PRECISE polar exactly,
               FAST within tolerance;
  collide_f64: Softbody.js's (f64 on the stored f32 positions and the f64 collider values, f32 stores after the push and the friction);
  collide_exact: the definition in f64 on the f32 inputs and the f32 view's collider values, no intermediate f32 store, with the hits, the
               chosen faces and a decision margin per particle -- what FAST is measured against, one substep at a time, on the scene that
               edge_scene plants on a state's own particles (tests/test_gpu_collider_pass.py).
"""
import numpy as np

KINDS = {"sphere": 0, "capsule": 1, "box": 2, "plane": 3}


def normalised(colliders):
    """The host's view: plane normals and box axes divided by their length in f64 (v / sqrt(v . v)); absent fields 0."""
    out = []
    for d in colliders:
        c = {"kind": KINDS[d["kind"]] if isinstance(d["kind"], str) else int(d["kind"])}
        for k in ("a", "b", "velocity"):
            c[k] = np.asarray(d.get(k, (0.0, 0.0, 0.0)), dtype=np.float64).reshape(3)
        c["axes"] = np.asarray(d.get("axes", np.eye(3)), dtype=np.float64).reshape(3, 3).copy()
        c["radius"] = float(d.get("radius", 0.0)) if c["kind"] in (0, 1) else 0.0
        c["friction"] = float(d.get("friction", 0.0))

        def unit(v):
            return v / np.sqrt((v[0] * v[0] + v[1] * v[1]) + v[2] * v[2])
        if c["kind"] == 3:
            c["b"] = unit(c["b"])
        if c["kind"] == 2:
            c["axes"] = np.stack([unit(c["axes"][j]) for j in range(3)])
        out.append(c)
    return out


def _dot(ax, ay, az, bx, by, bz):
    return (ax * bx + ay * by) + az * bz


def _collide(p, q, colliders, dt, f, store, mask):
    """p, q: [n, 3] f32 (position so far, end of the previous substep); f = the arithmetic's float type; store: the rounding of a
    position store; mask: particles the colliders may touch.  Returns the new positions (f32)."""
    p = np.array(p, dtype=np.float32)
    q = np.asarray(q, dtype=np.float32)
    dt = f(dt)
    zero, one = f(0.0), f(1.0)
    with np.errstate(all="ignore"):
        for c in normalised(colliders):
            x, y, z = (p[:, k].astype(f) for k in range(3))
            a = [f(v) for v in c["a"]]
            b = [f(v) for v in c["b"]]
            u = [[f(v) for v in row] for row in c["axes"]]
            r, fr = f(c["radius"]), f(c["friction"])
            V = [f(v) for v in c["velocity"]]
            if c["kind"] in (0, 1):
                cx, cy, cz = np.full_like(x, a[0]), np.full_like(x, a[1]), np.full_like(x, a[2])
                if c["kind"] == 1:
                    abx, aby, abz = b[0] - a[0], b[1] - a[1], b[2] - a[2]
                    ab2 = _dot(abx, aby, abz, abx, aby, abz)
                    t = np.zeros_like(x) if ab2 == 0 else _dot(x - a[0], y - a[1], z - a[2], abx, aby, abz) / ab2
                    t = np.where(t > zero, t, zero)   # max(t, 0), min(t, 1) (+0 for a zero t: Math.max)
                    t = np.where(t < one, t, one)
                    cx, cy, cz = a[0] + abx * t, a[1] + aby * t, a[2] + abz * t
                dx, dy, dz = x - cx, y - cy, z - cz
                L = np.sqrt(_dot(dx, dy, dz, dx, dy, dz))
                hit = (L < r) & (L > 0)
                nx, ny, nz, depth = dx / L, dy / L, dz / L, r - L
            elif c["kind"] == 2:
                dx, dy, dz = x - a[0], y - a[1], z - a[2]
                l = [_dot(dx, dy, dz, u[j][0], u[j][1], u[j][2]) for j in range(3)]
                g = [b[j] - np.abs(l[j]) for j in range(3)]
                hit = (np.abs(l[0]) < b[0]) & (np.abs(l[1]) < b[1]) & (np.abs(l[2]) < b[2])
                j = np.zeros(x.shape, dtype=np.int64)
                j = np.where(g[1] < np.choose(j, g), 1, j)
                j = np.where(g[2] < np.choose(j, g), 2, j)
                lj = np.choose(j, l)
                sgn = np.where(lj >= 0, one, -one)
                nx, ny, nz = (sgn * np.choose(j, [u[0][k], u[1][k], u[2][k]]) for k in range(3))
                depth = np.choose(j, g)
            else:
                nx, ny, nz = np.full_like(x, b[0]), np.full_like(x, b[1]), np.full_like(x, b[2])
                s = _dot(x - a[0], y - a[1], z - a[2], nx, ny, nz)
                hit = s < 0
                depth = -s
            hit = hit & mask
            px, py, pz = store(x + nx * depth), store(y + ny * depth), store(z + nz * depth)
            Dx = (q[:, 0].astype(f) - px.astype(f)) + V[0] * dt
            Dy = (q[:, 1].astype(f) - py.astype(f)) + V[1] * dt
            Dz = (q[:, 2].astype(f) - pz.astype(f)) + V[2] * dt
            dn = _dot(Dx, Dy, Dz, nx, ny, nz)
            m = dt * fr
            m = m if m < one else one
            px, py, pz = store(px.astype(f) + (Dx - nx * dn) * m), store(py.astype(f) + (Dy - ny * dn) * m), store(pz.astype(f) + (Dz - nz * dn) * m)
            p = np.where(hit[:, None], np.stack([px, py, pz], axis=1), p).astype(np.float32)
    return p


def collide_f32(p, q, colliders, dt, mask=None):
    n = len(p)
    return _collide(p, q, colliders, dt, np.float32, lambda v: np.asarray(v, dtype=np.float32), np.ones(n, bool) if mask is None else mask)


def collide_f64(p, q, colliders, dt, mask=None):
    n = len(p)
    return _collide(p, q, colliders, dt, np.float64, lambda v: np.asarray(v, dtype=np.float32), np.ones(n, bool) if mask is None else mask)


# ---- composed oracles -----------------------------------------------------------------------------------------------------------

def pj_velocity(p, q, dt, gravity):
    """P7 as the device writes it: (p - prev) / dt + (0, gravity, 0) * dt, f32"""
    dt32 = np.float32(dt)
    vel = (p - q) / dt32
    return (vel + np.array([np.float32(0.0) * dt32, np.float32(gravity) * dt32, np.float32(0.0) * dt32], dtype=np.float32)).astype(np.float32)


def pj_substep(orc, dt, pp, colliders, grabbed=()):
    """OraclePJ.simulate, then the colliders on every particle but the grabbed ones, the velocity again, written back with the
    oracle's own writeParticles.  Returns how many particles a collider moved."""
    orc.simulate(dt, pp)
    if not colliders:
        return 0
    p, q = orc.pos, orc.prevPos
    mask = np.ones(len(p), bool)
    mask[[g for g in grabbed if g >= 0]] = False
    p2 = collide_f32(p, q, colliders, dt, mask)
    ch = np.nonzero(np.any(p2.view(np.uint32) != p.view(np.uint32), axis=1))[0]
    if len(ch) == 0:
        return 0
    orc.writeParticles(ch.astype(np.int32), p2[ch], pj_velocity(p2[ch], q[ch], dt, pp["gravity"]))
    return len(ch)


def _nh_view(orc, name):
    ptr = getattr(orc._lib, "orc_nh_" + name)(orc._h)
    return np.ctypeslib.as_array(ptr, shape=(3 * orc.numParticles,)).reshape(-1, 3)


def nh_substep(orc, dt, pp, colliders):
    """OracleNH.simulate, then the colliders in Softbody.js's arithmetic on the oracle's own arrays (writable views), the velocity
    again as Softbody.js:238-239 derives it.  Returns how many particles a collider moved."""
    orc.simulate(dt, pp)
    if not colliders:
        return 0
    pos, prev, vel = _nh_view(orc, "pos"), _nh_view(orc, "prev"), _nh_view(orc, "vel")
    mask = np.ones(len(pos), bool)
    if orc.grabId >= 0:
        mask[orc.grabId] = False
    p2 = collide_f64(pos.copy(), prev.copy(), colliders, dt, mask)
    ch = np.nonzero(np.any(p2.view(np.uint32) != pos.view(np.uint32), axis=1))[0]
    if len(ch) == 0:
        return 0
    pos[ch] = p2[ch]
    inv_dt = 1.0 / float(dt)
    vel[ch] = ((pos[ch].astype(np.float64) - prev[ch].astype(np.float64)) * inv_dt).astype(np.float32)
    return len(ch)


# ---- the high-precision reference with decision margins ---------------------------------------------------------------------------

EPS = 1e-5   # metres: a particle closer than this to a branch of the definition is fragile (its branch may differ in f32)


def f32_view(colliders):
    """The values the f32 view (DevColliderF) holds: normalised() rounded to f32, widened to f64 again."""
    out = []
    for c in normalised(colliders):
        d = dict(c)
        for k in ("a", "b", "velocity", "axes"):
            d[k] = c[k].astype(np.float32).astype(np.float64)
        d["radius"] = float(np.float32(c["radius"]))
        d["friction"] = float(np.float32(c["friction"]))
        out.append(d)
    return out


def collide_exact(p, q, colliders, dt, mask=None):
    """The definition in f64 on the f32 inputs (positions, the f32 view's collider values, dt rounded to f32), no intermediate f32
    store.  Returns a dict of per-particle arrays:
      pos     [n, 3] f64  the final position
      hits    [n, m] bool which entries hit, in list order
      face    [n, m] int  the box face chosen (0..2), its sign in `sign` (+1 / -1); -1 where the entry is no box or did not hit
      normal  [n, m, 3]   the normal of each hit
      margin  [n] f64     the smallest distance (m) to any branch along the path: |L - r| and L (sphere, capsule), every e_k - |l_k| of
                          a box the particle is inside or within EPS of, best against second-best face gap and |l_k| of the chosen
                          face, |s| of a plane
      cond    [n] f64     the largest r / L of its sphere and capsule hits (how ill-conditioned the normal is; 0 without one)"""
    p = np.asarray(p, np.float32).astype(np.float64)
    q = np.asarray(q, np.float32).astype(np.float64)
    n, cols = len(p), f32_view(colliders)
    m = len(cols)
    mask = np.ones(n, bool) if mask is None else np.asarray(mask, bool)
    dt = float(np.float32(dt))
    hits, face, sign = np.zeros((n, m), bool), np.full((n, m), -1), np.zeros((n, m))
    normal = np.zeros((n, m, 3))
    margin, cond = np.full(n, np.inf), np.zeros(n)
    with np.errstate(all="ignore"):
        for k, c in enumerate(cols):
            a, b, u, r = c["a"], c["b"], c["axes"], c["radius"]
            if c["kind"] in (0, 1):
                centre = np.broadcast_to(a, p.shape)
                if c["kind"] == 1:
                    ab = b - a
                    ab2 = float(ab @ ab)
                    t = np.zeros(n) if ab2 == 0.0 else np.clip(((p - a) @ ab) / ab2, 0.0, 1.0)
                    centre = a + t[:, None] * ab
                d = p - centre
                L = np.sqrt((d * d).sum(1))
                hit = (L < r) & (L > 0)
                nrm = d / np.where(L > 0, L, 1.0)[:, None]
                depth = r - L
                here = np.minimum(np.abs(L - r), L)
                cond = np.where(hit & mask, np.maximum(cond, r / np.where(L > 0, L, 1.0)), cond)
            elif c["kind"] == 2:
                l = (p - a) @ u.T
                g = b[None, :] - np.abs(l)
                hit = (g > 0).all(1)
                j = np.argmin(g, axis=1)                              # (the first of equal minima: lowest on ties)
                rows = np.arange(n)
                lj, gs = l[rows, j], np.sort(g, axis=1)
                sg = np.where(lj >= 0, 1.0, -1.0)
                nrm = sg[:, None] * u[j]
                depth = g[rows, j]
                inside = np.minimum(np.abs(g).min(1), np.minimum(gs[:, 1] - gs[:, 0], np.abs(lj)))
                near = (g > -EPS).all(1)
                here = np.where(hit, inside, np.where(near, np.abs(g).min(1), (-g).max(1)))
                face[:, k] = np.where(hit & mask, j, -1)
                sign[:, k] = np.where(hit & mask, sg, 0.0)
            else:
                nrm = np.broadcast_to(b, p.shape)
                s = (p - a) @ b
                hit = s < 0
                depth = -s
                here = np.abs(s)
            margin = np.where(mask, np.minimum(margin, here), margin)
            hit = hit & mask
            p1 = p + nrm * depth[:, None]
            D = (q - p1) + c["velocity"] * dt
            T = D - nrm * (D * nrm).sum(1)[:, None]
            p2 = p1 + T * min(1.0, dt * c["friction"])
            p = np.where(hit[:, None], p2, p)
            hits[:, k] = hit
            normal[:, k] = np.where(hit[:, None], nrm, 0.0)
    return dict(pos=p, hits=hits, face=face, sign=sign, normal=normal, margin=margin, cond=cond)


def decisions(p, q, colliders, dt, restatement, mask=None):
    """Which entries move a particle and which box face they choose, read off one of the stepwise restatements (collide_f32 /
    collide_f64) entry by entry: ([n, m] bool, [n, m] int face or -1, [n, m] sign)."""
    p = np.asarray(p, np.float32)
    n, m = len(p), len(colliders)
    hits, face, sign = np.zeros((n, m), bool), np.full((n, m), -1), np.zeros((n, m))
    for k, c in enumerate(colliders):
        c0 = dict(c, friction=0.0)
        pushed = restatement(p, q, [c0], dt, mask)          # the push alone: along +-u_j for a box
        p2 = restatement(p, q, [c], dt, mask)
        moved = np.any(pushed.view(np.uint32) != p.view(np.uint32), axis=1)
        hits[:, k] = moved | np.any(p2.view(np.uint32) != p.view(np.uint32), axis=1)
        if KINDS.get(c["kind"], c["kind"]) == 2:
            d = pushed.astype(np.float64) - p.astype(np.float64)
            u = normalised([c])[0]["axes"]
            along = d @ u.T
            j = np.argmax(np.abs(along), axis=1)
            face[:, k] = np.where(moved, j, -1)
            sign[:, k] = np.where(moved, np.sign(along[np.arange(n), j]), 0.0)
        p = p2
    return hits, face, sign


# ---- the edge scene: eight colliders planted on the particles of a state -----------------------------------------------------------

def _edges(tets):
    t = np.asarray(tets)
    e = np.concatenate([t[:, [i, j]] for i in range(4) for j in range(i + 1, 4)])
    return np.unique(np.sort(e, axis=1), axis=0)


def _exact_offset(x, d):
    """centre c = x - d per axis in f32, and whether x - c is d exactly (as real numbers: then in f32, in f64 and under fma alike)"""
    x, d = np.asarray(x, np.float32), np.asarray(d, np.float32)
    c = (x - d).astype(np.float32)
    return c, bool(np.array_equal(x.astype(np.float64) - c.astype(np.float64), d.astype(np.float64)))


def edge_scene(p0, prev, tets, dt, skip=()):
    """Eight colliders (TETSIM_MAX_COLLIDERS) whose edge cases are exact in f32 because they are built from the f32 positions p0 that the
    collider pass will see.  Every value is an f32, so rows (setBodyColliders) and doubles (setColliders) are the same numbers.

      0 sphere        centre exactly p0[i]: i is not hit (L == 0); moving, friction 50
      1 sphere        overlaps entry 0 without reaching i; friction 1e4 (dt * friction > 1)
      2 capsule       a == b == p0[j] exactly: t = 0, j is not hit; friction 0
      3 capsule       end points exactly on the two particles of a tet edge whose difference is exact in f32: neither is hit (t = 0, t = 1);
                      particles before a, beyond b, between; friction 1e4
      4 box           axis-aligned, e = (e, e, e2), centre p0[k] - (d, d, 0) with d a power of two: x and y gaps tie, x wins; friction 0
      5 box           e = (e, e, e), centre p0[k3] - (d, d, d): a three-way tie, x wins; friction 0
      6 box           thin in y, centre exactly p0[z]: l_y == +0, the normal is +u_y; friction 0
      7 plane         tilted, through p0[s] exactly (s == 0: no hit), 5-12 % of the body below it; friction 50

    Returns (colliders, planted) with planted = {name: (particle, entry, what)}: what = None for "no entry moves it", else the f32
    displacement (3,) the one entry gives it, exact in every arithmetic (a single rounded add along an axis, friction 0).
    Particles are chosen greedily so that a planted particle lies clearly (EPS) outside every entry but its own; `skip` names particles that
    must not be planted (the held one, a particle no tet references)."""
    p0 = np.asarray(p0, np.float32)
    P = p0.astype(np.float64)
    n = len(P)
    F = lambda v: [float(np.float32(x)) for x in np.asarray(v).reshape(-1)]
    E = _edges(tets)
    h = float(np.median(np.linalg.norm(P[E[:, 0]] - P[E[:, 1]], axis=1)))
    d = np.float32(2.0 ** np.floor(np.log2(h)))                      # a power of two in (h / 2, h]
    e, e2, thin = np.float32(1.3 * h), np.float32(2.0 * h), np.float32(0.3 * h)
    R = float(np.float32(1.7 * h))
    ok = np.isfinite(P).all(1)
    ok[[s for s in skip]] = False
    ok[np.setdiff1d(np.arange(n), np.unique(tets))] = False
    centre = P[ok].mean(0)
    order = [int(i) for i in np.argsort(np.linalg.norm(P - centre, axis=1)) if ok[i]]   # interior particles first

    # the plane first: everything else is planted above it
    nrm = np.array([0.2, 1.0, 0.1])
    un = f32_view([dict(kind="plane", b=nrm)])[0]["b"]
    height = P @ un
    want = np.sort(height[ok])[int(0.08 * ok.sum())]
    s_id = min((i for i in order), key=lambda i: abs(height[i] - want))
    cols = [None] * 8
    cols[7] = dict(kind="plane", a=F(p0[s_id]), b=F(nrm), friction=50.0)
    planted = {"plane point": (s_id, 7, None)}
    above = height - height[s_id]

    def outside_all(i, entries, push=None):
        """particle i clearly outside every entry placed so far (but `entries`' own), where it is and where its own entry pushes it"""
        cs = [c for k, c in enumerate(cols) if c is not None and k not in entries]
        if not cs:
            return True
        at = p0[i:i + 1] if push is None else np.stack([p0[i], (p0[i] + push).astype(np.float32)])
        one = collide_exact(at, at, cs, dt)
        return not one["hits"].any() and one["margin"].min() > 10 * EPS

    def place(names, entries, make, what, count=10):
        """the first particle (interior first) for which make(i) gives entries that leave every planted particle alone, that lies outside
        all other entries, and whose entries hit >= count particles each"""
        for i in order:
            if above[i] < 10 * EPS or any(i == v[0] for v in planted.values()):
                continue
            made = make(i)
            if made is None:
                continue
            new, ids = made
            if any(j == v[0] for v in planted.values() for j in ids) or not all(outside_all(j, ()) for j in ids):
                continue
            for k, c in zip(entries, new):
                cols[k] = c
            good = all(outside_all(j, (k,), w) for j, k, w in list(planted.values()) + [(j, entries[0], w) for j, w in zip(ids, what)])
            if good:
                res = collide_exact(p0, prev, [c for c in cols if c is not None], dt, ok)   # (in list order: earlier entries move particles)
                good = bool((res["hits"].sum(0) >= count).all())
            if good:
                for name, j, w in zip(names, ids, what):
                    planted[name] = (j, entries[0], w)
                return i
            for k in entries:
                cols[k] = None
        raise AssertionError("no particle for " + names[0])

    def spheres(i):
        far = P[i] + 1.3 * R * np.array([0.8, 0.0, 0.6])
        return [dict(kind="sphere", a=F(p0[i]), radius=R, friction=50.0, velocity=[0.25, -0.125, 0.5]),
                dict(kind="sphere", a=F(far), radius=R, friction=1e4)], [i]
    place(["sphere centre"], (0, 1), spheres, [None])
    place(["degenerate capsule"], (2,), lambda i: ([dict(kind="capsule", a=F(p0[i]), b=F(p0[i]), radius=R, friction=0.0)], [i]), [None])

    def capsule(i):
        mine = E[(E == i).any(1)]
        if not len(mine):
            return None
        # b - a must be an f32 in every coordinate: only then is a + (b - a) * 1 the point b itself, in f32 as in f64, and L == 0 on b
        ab = P[mine[:, 0]] - P[mine[:, 1]]
        mine = mine[(ab.astype(np.float32).astype(np.float64) == ab).all(1)]
        if not len(mine):
            return None
        e = mine[np.argmax(np.linalg.norm(P[mine[:, 0]] - P[mine[:, 1]], axis=1))]
        j = int(e[0] if e[1] == i else e[1])
        if not ok[j] or above[j] < 10 * EPS:
            return None
        return [dict(kind="capsule", a=F(p0[i]), b=F(p0[j]), radius=R, friction=1e4)], [i, j]
    place(["capsule end a", "capsule end b"], (3,), capsule, [None, None])

    def tie(off, e):
        def make(i):
            c, exact = _exact_offset(p0[i], off)
            if not exact:
                return None
            return [dict(kind="box", a=F(c), b=F(e), friction=0.0)], [i]
        return make
    push = [np.array([e - d, 0, 0], np.float32)]                 # the gap e - d (exact in f32 and f64) along +x, the lowest tied axis
    place(["box tie two-way"], (4,), tie([d, d, 0], [e, e, e2]), push)
    place(["box tie three-way"], (5,), tie([d, d, d], [e, e, e]), push)
    place(["box zero"], (6,), tie([0, 0, 0], [e2, thin, e2]), [np.array([0, thin, 0], np.float32)])
    return cols, planted


def swapped(cols):
    """the edge scene with its two overlapping spheres in the other list order"""
    return [cols[1], cols[0]] + list(cols[2:])


def exact_velocity(pos, q, dt, gravity=None):
    """the velocity in f64 from exact positions: (p - q) / dt, for polar + (0, gravity, 0) * dt; dt and gravity as the f32 the device holds"""
    dt = float(np.float32(dt))
    v = (np.asarray(pos, np.float64) - np.asarray(q, np.float32).astype(np.float64)) / dt
    if gravity is not None:
        v = v + np.array([0.0, float(np.float32(gravity)) * dt, 0.0])
    return v


__all__ = ["collide_f32", "collide_f64", "collide_exact", "decisions", "edge_scene", "swapped", "exact_velocity", "f32_view", "EPS",
           "normalised", "pj_velocity", "pj_substep", "nh_substep"]
