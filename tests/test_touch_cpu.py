"""tests/touch_ref.py against what it restates, without a GPU: the step's own hit test (collider_ref.collide_f64 and the definition in
include/tetsim.h), a brute-force distance to a box, the degenerate shapes, the reduction tree against straight loops and math.fsum, and
the binding's constants against the header."""
import math
import os
import re

import numpy as np
import pytest

import collider_ref
import touch_ref

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
AXES = np.array([[0.6, 0.8, 0.0], [-0.8, 0.6, 0.0], [0.0, 0.0, 1.0]])
SHAPES = {
    "sphere": dict(kind="sphere", a=(0.1, 0.2, -0.1), radius=0.7),
    "capsule": dict(kind="capsule", a=(-0.3, 0.0, 0.1), b=(0.4, 0.2, -0.2), radius=0.5),
    "box": dict(kind="box", a=(0.05, -0.1, 0.2), b=(0.6, 0.4, 0.5), axes=AXES),
    "plane": dict(kind="plane", a=(0.0, 0.1, 0.0), b=(0.1, 1.0, -0.2)),
}


def bits(a):
    return np.ascontiguousarray(a, dtype=np.float64).view(np.uint64)


def seeded_points(seed, n=4000):
    return np.random.default_rng(seed).uniform(-1.2, 1.2, (n, 3)).astype(np.float32)


def push(p, c):
    """The f64 hit test of tetsim_set_colliders (include/tetsim.h), written down once more: (hit, depth, normal)."""
    x, y, z = (p[:, k].astype(np.float64) for k in range(3))
    a, b, u, r = c["a"], c["b"], c["axes"], c["radius"]
    dot = lambda ax, ay, az, bx, by, bz: (ax * bx + ay * by) + az * bz
    with np.errstate(all="ignore"):
        if c["kind"] in (0, 1):
            cx, cy, cz = a[0], a[1], a[2]
            if c["kind"] == 1:
                ab = b - a
                ab2 = dot(ab[0], ab[1], ab[2], ab[0], ab[1], ab[2])
                t = np.zeros_like(x) if ab2 == 0 else dot(x - a[0], y - a[1], z - a[2], ab[0], ab[1], ab[2]) / ab2
                t = np.minimum(np.maximum(t, 0.0), 1.0)
                cx, cy, cz = a[0] + ab[0] * t, a[1] + ab[1] * t, a[2] + ab[2] * t
            dx, dy, dz = x - cx, y - cy, z - cz
            L = np.sqrt(dot(dx, dy, dz, dx, dy, dz))
            return (L < r) & (L > 0), r - L, np.stack([dx / L, dy / L, dz / L], axis=1)
        if c["kind"] == 2:
            dx, dy, dz = x - a[0], y - a[1], z - a[2]
            l = np.stack([dot(dx, dy, dz, u[j][0], u[j][1], u[j][2]) for j in range(3)], axis=1)
            g = b[None, :] - np.abs(l)
            hit = (np.abs(l) < b[None, :]).all(axis=1)
            j = np.zeros(len(x), dtype=np.int64)
            rows = np.arange(len(x))
            j = np.where(g[:, 1] < g[rows, j], 1, j)
            j = np.where(g[:, 2] < g[rows, j], 2, j)
            sgn = np.where(l[rows, j] >= 0, 1.0, -1.0)
            return hit, g[rows, j], sgn[:, None] * u[j]
        s = dot(x - a[0], y - a[1], z - a[2], b[0], b[1], b[2])
        return s < 0, -s, np.broadcast_to(b, (len(x), 3))


@pytest.mark.parametrize("f64", [True, False], ids=["f64-view", "f32-view"])
@pytest.mark.parametrize("shape", list(SHAPES))
def test_where_the_step_pushes_sd_is_minus_its_depth_and_n_its_normal(shape, f64):
    p = seeded_points(3 + len(shape))
    (c,) = touch_ref.view([SHAPES[shape]], f64)
    sd, n = touch_ref.sd_n(p, c)
    hit, depth, normal = push(p, c)
    assert 200 < hit.sum() < len(p) - 200, hit.sum()
    assert (sd[hit] < 0).all() and np.array_equal(bits(-sd[hit]), bits(depth[hit])) and np.array_equal(bits(n[hit]), bits(normal[hit]))
    assert (sd[~hit] >= 0).all()
    if not f64:
        return
    # ... and collider_ref's own f64 push (no friction, q = p: only the push moves a particle) lands where sd and n say
    moved = collider_ref.collide_f64(p, p, [dict(SHAPES[shape], friction=0.0)], 1.0 / 300.0)
    with np.errstate(invalid="ignore"):
        want = np.where(hit[:, None], (p.astype(np.float64) + n * (-sd)[:, None]).astype(np.float32), p)
    assert np.array_equal(moved.view(np.uint32), want.view(np.uint32))
    assert (np.any(moved.view(np.uint32) != p.view(np.uint32), axis=1) <= hit).all()


def ulp_distance(a, b):
    return abs(int(np.float64(a).view(np.int64)) - int(np.float64(b).view(np.int64)))


def test_outside_a_box_sd_is_the_distance_to_the_box():
    (c,) = touch_ref.view([SHAPES["box"]], True)
    a, e, u = c["a"], c["b"], c["axes"]
    local = np.random.default_rng(5).uniform(-1.5, 1.5, (3000, 3))
    # points on a face, on an edge, on a corner, and straight out from each
    special = np.array([[e[0], 0.1, -0.2], [e[0], -e[1], 0.3], [-e[0], e[1], -e[2]], [e[0] + 0.5, 0.1, -0.2], [e[0] + 0.3, -e[1] - 0.4, 0.3],
                        [-e[0] - 0.1, e[1] + 0.2, -e[2] - 0.3]])
    local = np.concatenate([local, special])
    p = (a[None, :] + local @ u).astype(np.float32)
    sd, n = touch_ref.sd_n(p, c)
    # brute force: the local coordinates by the header's dot, clamped to the box; the distance between the point and its clamped image with
    # the squares summed by fsum.  Against it sd has its two sums and half of the squares' roundings on top: 4 ulp covers them.
    d = p.astype(np.float64) - a[None, :]
    l = np.stack([(d[:, 0] * u[k][0] + d[:, 1] * u[k][1]) + d[:, 2] * u[k][2] for k in range(3)], axis=1)
    q = np.clip(l, -e, e)
    brute = np.array([math.sqrt(math.fsum(((l[i] - q[i]) ** 2).tolist())) for i in range(len(p))])
    outside = (np.abs(l) > e[None, :]).any(axis=1)
    assert outside.sum() > 1000
    for i in np.nonzero(outside)[0]:
        assert sd[i] > 0 and ulp_distance(sd[i], brute[i]) <= 4, (i, sd[i], brute[i])
        assert abs(math.sqrt(float(n[i] @ n[i])) - 1.0) < 1e-12
    for i in range(len(local) - 6, len(local) - 3):      # on the face, the edge, the corner: within roundings of 0
        assert abs(sd[i]) < 1e-7, (i, sd[i])
    k = len(local) - 3                                        # straight out of the face, the edge, the corner
    assert abs(sd[k] - 0.5) < 1e-7 and np.allclose(n[k], u[0], atol=1e-6)
    assert abs(sd[k + 1] - 0.5) < 1e-7 and np.allclose(n[k + 1], 0.6 * u[0] - 0.8 * u[1], atol=1e-6)
    assert abs(sd[k + 2] - math.sqrt(0.14)) < 1e-7 and np.allclose(n[k + 2], (-0.1 * u[0] + 0.2 * u[1] - 0.3 * u[2]) / math.sqrt(0.14), atol=1e-6)


def test_outside_sd_equals_the_brute_force_distance_within_4_ulp_on_an_axis_aligned_box():
    """With identity axes l is one exact subtraction in both computations: the only roundings are the squares, their sums and the root."""
    (c,) = touch_ref.view([dict(kind="box", a=(0.25, -0.5, 0.125), b=(0.5, 0.25, 0.75))], True)
    p = seeded_points(17, 5000) * np.float32(1.5)
    sd, _ = touch_ref.sd_n(p, c)
    l = p.astype(np.float64) - c["a"][None, :]
    over = np.maximum(np.abs(l) - c["b"][None, :], 0.0)
    outside = (over > 0).any(axis=1)
    assert outside.sum() > 2000
    for i in np.nonzero(outside)[0]:
        brute = math.sqrt(math.fsum((over[i] ** 2).tolist()))
        assert ulp_distance(sd[i], brute) <= 4, (i, sd[i], brute)


def test_degenerate_capsule_and_the_centre_of_a_sphere():
    ball = dict(kind="sphere", a=(0.5, 0.25, -0.125), radius=0.375)
    stub = dict(kind="capsule", a=(0.5, 0.25, -0.125), b=(0.5, 0.25, -0.125), radius=0.375)
    p = np.concatenate([seeded_points(9, 500), np.array([[0.5, 0.25, -0.125]], np.float32)])
    for f64 in (True, False):
        (cb, cs) = touch_ref.view([ball, stub], f64)
        sd_b, n_b = touch_ref.sd_n(p, cb)
        sd_s, n_s = touch_ref.sd_n(p, cs)
        assert np.array_equal(bits(sd_b), bits(sd_s)) and np.array_equal(bits(n_b), bits(n_s))
        assert sd_b[-1] == -0.375 and not n_b[-1].any()
    rows = touch_ref.particle_rows(p, touch_ref.view([ball], True), 0.0)
    assert rows[-1, 0] == np.float32(-0.375) and not rows[-1, 1:4].any() and rows[-1, 4] == 0 and rows[-1, 5] == 1
    nan = p.copy()
    nan[3] = np.nan
    rows = touch_ref.particle_rows(nan, touch_ref.view(list(SHAPES.values()), True), 1e9)
    assert rows[3, 0] == np.inf and rows[3, 4] == -1 and rows[3, 5] == 0 and (rows[:3, 5] == 4).all()


@pytest.mark.parametrize("n", [1, 255, 256, 257, 70000])
def test_the_tree_counts_and_takes_minima_as_a_loop_and_sums_within_the_bound(n):
    rng = np.random.default_rng(n)
    terms = rng.normal(0.0, 3.0, (n, 3))
    terms[:, 1] = (rng.uniform(size=n) < 0.3).astype(np.float64)        # a count: small integers add up exactly in any order
    terms[rng.integers(0, n, max(1, n // 50)), 0] = np.nan                # NaN is never a minimum
    terms[:, 0] = touch_ref.fmin(terms[:, 0], touch_ref.INF)
    got = touch_ref.reduce_body(terms, [True, False, False])
    loop_min, loop_count = touch_ref.INF, 0
    for v, c in zip(terms[:, 0], terms[:, 1]):
        loop_min = v if v < loop_min else loop_min
        loop_count += int(c)
    assert got[0] == loop_min and got[1] == loop_count
    exact = math.fsum(terms[:, 2].tolist())
    bound = n * 2.0 ** -53 * math.fsum(np.abs(terms[:, 2]).tolist())
    print("n = %d: |tree - fsum| = %.3g, bound %.3g" % (n, abs(got[2] - exact), bound))
    assert abs(got[2] - exact) <= bound
    if n == 70000:
        assert -(-n // 256) > 256                                        # more chunk rows than threads: the fold strides


def test_the_bindings_constants_are_the_headers():
    from tetsim_amd import _capi as capi
    text = open(os.path.join(ROOT, "include", "tetsim.h")).read()
    found = dict(re.findall(r"#define TETSIM_(TOUCH_\w+) (\d+)", text))
    found.update(re.findall(r"TETSIM_(TOUCH_\w+) = (\d+)", text))
    assert len(found) == 19, sorted(found)
    for name, value in found.items():
        assert getattr(capi, name) == int(value), name
    assert (touch_ref.WIDTH, touch_ref.SLOT_WIDTH, touch_ref.PARTICLE_WIDTH, touch_ref.SLOT0) == (capi.TOUCH_WIDTH, capi.TOUCH_SLOT_WIDTH,
                                                                                                  capi.TOUCH_PARTICLE_WIDTH, capi.TOUCH_SLOT0)
    assert capi.TOUCH_WIDTH == capi.TOUCH_SLOT0 + capi.MAX_COLLIDERS * capi.TOUCH_SLOT_WIDTH
    for s in ("tetsim_touch_bodies_device", "tetsim_read_body_touch", "tetsim_touch_particles_device"):
        assert s in capi.SYMBOLS and re.search(r"\bint %s\(" % s, text)
