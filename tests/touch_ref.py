"""numpy restatement of the touch query (include/tetsim.h: tetsim_touch_bodies_device / tetsim_touch_particles_device), value for value.

Three parts, all f64 with every operation rounded on its own (numpy never fuses):
  sd_n            the signed distance and the outward normal of every particle against one collider, as the header defines them;
  particle_rows   the per-particle rows (nearest slot by an ascending scan with <, the touched slots), rounded once to f32;
  body_rows       the per-body rows, the sums taken through an emulation of the documented tree (body_reduce.h): a body's particles in
                  chunks of 256 from its own first one, a chunk padded to 256 with the identities, within each wave of 64 lane l takes
                  lane l + 32, 16, .. 1, the waves combined as (w0 + w1) + (w2 + w3); the chunk rows folded by thread t over rows t,
                  t + 256, .. from the identity, then the same tree.
Collider values come the way the handle holds them (`view`): collider_ref.normalised's f64 normalisation, and for an f32-view handle
every value rounded once to f32 and widened again."""
import numpy as np

import collider_ref

INF = float("inf")
WIDTH, SLOT_WIDTH, PARTICLE_WIDTH, SLOT0, MAX_SLOTS = 100, 12, 8, 4, 8
CHUNK = 256


def view(colliders, f64):
    """dicts as setColliders takes them -> the list a handle holds (f64: PRECISE Neo-Hookean; else the f32 view), values as float64"""
    out = []
    for c in collider_ref.normalised(colliders):
        if not f64:
            c = dict(c)
            for k in ("a", "b", "axes", "velocity"):
                c[k] = c[k].astype(np.float32).astype(np.float64)
            for k in ("radius", "friction"):
                c[k] = float(np.float32(c[k]))
        out.append(c)
    return out


def _dot(ax, ay, az, bx, by, bz):
    return (ax * bx + ay * by) + az * bz


def sd_n(pos, c):
    """pos: [n, 3] f32; c: one entry of view().  Returns (sd [n], normal [n, 3]) in f64."""
    p = np.asarray(pos, np.float32).astype(np.float64)
    x, y, z = p[:, 0], p[:, 1], p[:, 2]
    a, b, u = c["a"], c["b"], c["axes"]
    with np.errstate(all="ignore"):
        if c["kind"] in (0, 1):
            cx, cy, cz = np.full_like(x, a[0]), np.full_like(x, a[1]), np.full_like(x, a[2])
            if c["kind"] == 1:
                abx, aby, abz = b[0] - a[0], b[1] - a[1], b[2] - a[2]
                ab2 = _dot(abx, aby, abz, abx, aby, abz)
                t = np.zeros_like(x) if ab2 == 0 else _dot(x - a[0], y - a[1], z - a[2], abx, aby, abz) / ab2
                nan = np.isnan(t)
                t = np.where(t > 0.0, t, 0.0)                   # Math.max(t, 0), Math.min(.., 1); NaN stays NaN
                t = np.where(t < 1.0, t, 1.0)
                t = np.where(nan, np.nan, t)
                cx, cy, cz = a[0] + abx * t, a[1] + aby * t, a[2] + abz * t
            dx, dy, dz = x - cx, y - cy, z - cz
            L = np.sqrt(_dot(dx, dy, dz, dx, dy, dz))
            sd = L - c["radius"]
            apart = L > 0.0
            n = np.stack([np.where(apart, dx / L, 0.0), np.where(apart, dy / L, 0.0), np.where(apart, dz / L, 0.0)], axis=1)
        elif c["kind"] == 2:
            dx, dy, dz = x - a[0], y - a[1], z - a[2]
            l = [_dot(dx, dy, dz, u[j][0], u[j][1], u[j][2]) for j in range(3)]
            g = [b[j] - np.abs(l[j]) for j in range(3)]
            inside = (g[0] >= 0.0) & (g[1] >= 0.0) & (g[2] >= 0.0)
            j = np.zeros(x.shape, dtype=np.int64)
            j = np.where(g[1] < np.choose(j, g), 1, j)
            j = np.where(g[2] < np.choose(j, g), 2, j)
            plus = np.choose(j, l) >= 0.0
            sd_in = -np.choose(j, g)
            n_in = [np.where(plus, np.choose(j, [u[0][k], u[1][k], u[2][k]]), -np.choose(j, [u[0][k], u[1][k], u[2][k]])) for k in range(3)]
            o = [np.where(np.isnan(g[k]), np.nan, np.where(-g[k] > 0.0, -g[k], 0.0)) for k in range(3)]
            s = [np.where(l[k] >= 0.0, o[k], -o[k]) for k in range(3)]
            sd_out = np.sqrt((o[0] * o[0] + o[1] * o[1]) + o[2] * o[2])
            w = [((0.0 + s[0] * u[0][k]) + s[1] * u[1][k]) + s[2] * u[2][k] for k in range(3)]
            sd = np.where(inside, sd_in, sd_out)
            n = np.stack([np.where(inside, n_in[k], w[k] / sd_out) for k in range(3)], axis=1)
        else:
            sd = _dot(x - a[0], y - a[1], z - a[2], b[0], b[1], b[2])
            n = np.broadcast_to(np.asarray(b, np.float64), p.shape).copy()
    return sd, n


def fmin(a, b):
    """fmin as the device takes it: a NaN loses, -0 is below +0"""
    a, b = np.broadcast_arrays(np.asarray(a, np.float64), np.asarray(b, np.float64))
    r = np.where(np.isnan(a), b, np.where(np.isnan(b), a, np.where(b < a, b, a)))
    zeros = (a == 0.0) & (b == 0.0)
    return np.where(zeros, np.where(np.signbit(a) | np.signbit(b), -0.0, 0.0), r)


# ---- the tree ---------------------------------------------------------------------------------------------------------------------------
def _combine(a, b, minima):
    """rows [.., K]: column k a minimum where minima[k], a sum otherwise"""
    out = a + b
    for k in np.nonzero(minima)[0]:
        out[..., k] = fmin(a[..., k], b[..., k])
    return out


def _identity(minima):
    return np.where(minima, INF, 0.0)


def tree256(rows, minima):
    """[256, K] lanes of a workgroup -> [K], what thread 0 holds behind block_reduce"""
    w = np.asarray(rows, np.float64).reshape(4, 64, -1)
    for off in (32, 16, 8, 4, 2, 1):
        w = _combine(w[:, :off], w[:, off:2 * off], minima)
    w = w[:, 0]
    return _combine(_combine(w[0], w[1], minima), _combine(w[2], w[3], minima), minima)


def reduce_body(terms, minima):
    """[n, K] per-particle terms of ONE body (the identities where a particle contributes nothing) -> [K] through chunks, fold and tree"""
    terms = np.asarray(terms, np.float64)
    minima = np.asarray(minima, bool)
    n, K = terms.shape
    ident = _identity(minima)
    chunks = []
    for at in range(0, n, CHUNK):
        lanes = np.tile(ident, (CHUNK, 1))
        lanes[:min(CHUNK, n - at)] = terms[at:at + CHUNK]
        chunks.append(tree256(lanes, minima))
    acc = np.tile(ident, (CHUNK, 1))
    for at in range(0, len(chunks), CHUNK):                    # thread t: rows t, t + 256, ..
        part = np.asarray(chunks[at:at + CHUNK])
        acc[:len(part)] = _combine(acc[:len(part)], part, minima)
    return tree256(acc, minima)


# ---- the rows ---------------------------------------------------------------------------------------------------------------------------
def particle_rows(pos, cols, margin):
    """one body's particles against its list -> float32 [n, 8]"""
    pos = np.asarray(pos, np.float32)
    n = len(pos)
    best, slot, touches = np.full(n, INF), np.full(n, -1.0), np.zeros(n)
    normal = np.zeros((n, 3))
    for k, c in enumerate(cols):
        sd, nn = sd_n(pos, c)
        with np.errstate(invalid="ignore"):
            better = sd < best
            touches += sd < margin
        best = np.where(better, sd, best)
        normal = np.where(better[:, None], nn, normal)
        slot = np.where(better, float(k), slot)
    out = np.zeros((n, PARTICLE_WIDTH), np.float32)
    with np.errstate(over="ignore"):
        out[:, 0] = best.astype(np.float32)
        out[:, 1:4] = normal.astype(np.float32)
    out[:, 4], out[:, 5] = slot, touches
    return out


def body_row(pos, vel, cols, margin):
    """one body -> float64 [100]"""
    pos, vel = np.asarray(pos, np.float32), np.asarray(vel, np.float32)
    p, v = pos.astype(np.float64), vel.astype(np.float64)
    n = len(pos)
    row = np.zeros(WIDTH)
    nearest, any_touch = np.full(n, INF), np.zeros(n, bool)
    least, least_slot = INF, -1.0
    slot_min = np.array([True] + [False] * 9)
    for k, c in enumerate(cols):
        sd, nn = sd_n(pos, c)
        with np.errstate(invalid="ignore"):
            touch = sd < margin
        nearest = fmin(nearest, sd)
        any_touch |= touch
        terms = np.zeros((n, 10))
        terms[:, 0] = fmin(sd, INF)
        terms[:, 1:4] = np.where(touch[:, None], p, 0.0)
        terms[:, 4:7] = np.where(touch[:, None], nn, 0.0)
        terms[:, 7:10] = np.where(touch[:, None], v - c["velocity"][None, :], 0.0)
        r = reduce_body(terms, slot_min)
        count = int(touch.sum())
        s = row[SLOT0 + SLOT_WIDTH * k:SLOT0 + SLOT_WIDTH * (k + 1)]
        s[0], s[1], s[2] = c["kind"], count, r[0]
        with np.errstate(all="ignore"):
            s[3:12] = r[1:10] / float(count) if count else 0.0
        if r[0] < least:
            least, least_slot = r[0], float(k)
    for k in range(len(cols), MAX_SLOTS):
        row[SLOT0 + SLOT_WIDTH * k], row[SLOT0 + SLOT_WIDTH * k + 2] = -1.0, INF
    row[0] = int(any_touch.sum())
    row[1] = reduce_body(nearest[:, None], np.array([True]))[0]
    row[2], row[3] = least_slot, len(cols)
    return row


def body_rows(pos, vel, lists, margin, first_vert=None):
    """a batch: lists[b] = view() of body b's colliders -> float64 [bodies, 100]"""
    first_vert = [0, len(pos)] if first_vert is None else first_vert
    return np.stack([body_row(pos[first_vert[b]:first_vert[b + 1]], vel[first_vert[b]:first_vert[b + 1]], lists[b], margin) for b in range(len(lists))])


def all_particle_rows(pos, lists, margin, first_vert=None):
    first_vert = [0, len(pos)] if first_vert is None else first_vert
    return np.concatenate([particle_rows(pos[first_vert[b]:first_vert[b + 1]], lists[b], margin) for b in range(len(lists))])
