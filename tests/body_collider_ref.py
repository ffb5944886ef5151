"""Body colliders (include/tetsim.h: tetsim_set_body_colliders / _device) restated in numpy, as far as the tests need them: the rows, the
host's validity rules on one row, the lists a solo twin passes to setColliders, and the collider scene in f32 values.

A row is 24 float32: kind as a value (-1 = empty slot), a, b, axes, radius, friction, velocity, three floats nobody reads.  Every f32 is
exactly a double, so "the same rows widened to double" is a well-defined list for tetsim_set_colliders."""
import numpy as np

FLOATS = 24
KINDS = {"sphere": 0, "capsule": 1, "box": 2, "plane": 3}
NAMES = {v: k for k, v in KINDS.items()}
_IDENTITY = ((1.0, 0.0, 0.0), (0.0, 1.0, 0.0), (0.0, 0.0, 1.0))


def row(c):
    """one collider dict (the fields make_colliders reads) -> 24 float32; a dict with a non-zero `reserved` has no row"""
    if int(c.get("reserved", 0)) != 0:
        raise ValueError("a row has no `reserved` field")
    kind = c["kind"]
    r = np.zeros(FLOATS, np.float32)
    r[0] = KINDS[kind] if isinstance(kind, str) else kind
    r[1:4] = np.asarray(c.get("a", (0.0, 0.0, 0.0)), np.float64).reshape(3)
    r[4:7] = np.asarray(c.get("b", (0.0, 0.0, 0.0)), np.float64).reshape(3)
    r[7:16] = np.asarray(c.get("axes", _IDENTITY), np.float64).reshape(9)
    r[16] = c.get("radius", 0.0)
    r[17] = c.get("friction", 0.0)
    r[18:21] = np.asarray(c.get("velocity", (0.0, 0.0, 0.0)), np.float64).reshape(3)
    return r


def rows(lists, per_body=None):
    """a list per body of collider dicts -> float32 [bodies, per_body, 24]; unused slots are empty rows (kind -1, everything else 0)"""
    longest = max([len(cs) for cs in lists] + [1])
    per_body = longest if per_body is None else per_body
    if not 1 <= per_body <= 8 or longest > per_body:
        raise ValueError("per_body must be 1 .. 8 and hold the longest list")
    out = np.zeros((len(lists), per_body, FLOATS), np.float32)
    out[:, :, 0] = -1.0
    for b, cs in enumerate(lists):
        for k, c in enumerate(cs):
            out[b, k] = row(c)
    return out


def _unit(v):
    l2 = (v[0] * v[0] + v[1] * v[1]) + v[2] * v[2]
    if not l2 > 0.0:
        return None
    return v / np.sqrt(l2)


# why a collider is refused, in the order the library checks (body_rows.h: ColliderRefusal); 0 = accepted
REFUSALS = ("", "unknown kind", "non-finite value", "negative radius or friction", "zero-length plane normal", "negative half-extent", "zero-length box axis",
            "box axes are not orthogonal")


def views(w):
    """The library's one collider routine (body_rows.h: collider_view, collider_f32) on 21 doubles -- kind as a value, a, b, axes, radius,
    friction, velocity, a row's order -- in numpy: (code, the f64 view's 168 bytes, the f32 view's 88 bytes), the views None for a refused
    collider.  Every operation is an f64 one rounded on its own: (x*x + y*y) + z*z, sqrt, /; the f32 view is astype(float32)."""
    w = np.asarray(w, np.float64)
    if w[0] not in (0.0, 1.0, 2.0, 3.0):
        return 1, None, None
    if not np.isfinite(w[1:21]).all():
        return 2, None, None
    kind = int(w[0])
    round_ = kind in (0, 1)
    if w[17] < 0.0 or (round_ and w[16] < 0.0):
        return 3, None, None
    a, b, v = w[1:4].copy(), w[4:7].copy(), w[18:21].copy()
    u = np.zeros(9)
    if kind == 3:
        b = _unit(w[4:7])
        if b is None:
            return 4, None, None
    if kind == 2:
        for j in range(3):
            if w[4 + j] < 0.0:
                return 5, None, None
            uj = _unit(w[7 + 3 * j:10 + 3 * j])
            if uj is None:
                return 6, None, None
            u[3 * j:3 * j + 3] = uj
        for i in range(3):
            for j in range(i + 1, 3):
                ui, uj = u[3 * i:3 * i + 3], u[3 * j:3 * j + 3]
                if abs((ui[0] * uj[0] + ui[1] * uj[1]) + ui[2] * uj[2]) > 1e-5:
                    return 7, None, None
    d = np.concatenate([a, b, u, [w[16] if round_ else 0.0, w[17]], v])
    tail = np.array([kind, 0], "<i4").tobytes()
    return 0, d.astype("<f8").tobytes() + tail, d.astype("<f4").tobytes() + tail


def refusal(r):
    """views' code for one row of 24 floats (f64 arithmetic on the f32 values); an empty slot (kind -1) is not a collider: None"""
    r = np.asarray(r, np.float32).astype(np.float64)
    return None if r[0] == -1.0 else views(r[:21])[0]


def row_ok(r):
    """tetsim_set_colliders' validity rules on one row of 24 floats (f64 arithmetic on the f32 values, in the host's order).  An empty
    slot (kind -1) is not a collider: False."""
    return refusal(r) == 0


def lists_from_rows(rws):
    """float32 [bodies, per_body, >= 24] -> per body the list of dicts for the solo's setColliders: the rows row_ok accepts, in slot order,
    every value the row's f32 widened to a Python float"""
    out = []
    for body in np.asarray(rws, np.float32):
        cs = []
        for r in body:
            if not row_ok(r[:FLOATS]):
                continue
            d = r.astype(np.float64)
            cs.append(dict(kind=NAMES[int(d[0])], a=d[1:4].tolist(), b=d[4:7].tolist(), axes=d[7:16].reshape(3, 3).tolist(), radius=float(d[16]),
                           friction=float(d[17]), velocity=d[18:21].tolist()))
        out.append(cs)
    return out


def f32_scene(v, frame=0):
    """scene() of test_gpu_colliders.py with every value rounded to f32 first: the batch's rows and the twin's doubles are the same numbers"""
    from test_gpu_colliders import scene
    return lists_from_rows(rows([scene(v, frame)]))[0]
