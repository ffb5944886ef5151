"""numpy restatement of the kinematic colliders (include/tetsim.h tetsim_set_colliders) and the composed oracle built on it.

Colliders act last on a particle, before its velocity, so "oracle substep, then colliders on its result" is "the library's substep
with colliders": the oracle (oracle/) stays as it is and checks the device bit for bit.

  collide_f32: the polar solver's arithmetic (IEEE f32, every operation rounded, correctly rounded / and sqrt) -- PRECISE polar exactly,
               FAST within tolerance;
  collide_f64: Softbody.js's (f64 on the stored f32 positions and the f64 collider values, f32 stores after the push and the friction).
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


__all__ = ["collide_f32", "collide_f64", "normalised", "pj_velocity", "pj_substep", "nh_substep"]
