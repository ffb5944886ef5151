"""Kinematic colliders (include/tetsim.h tetsim_set_colliders), CPU side: the C struct and its ctypes mirror agree, the library exports
the entry point, and the numpy restatement the GPU tests compare against (collider_ref.py) reproduces hand-worked contacts."""
import ctypes as C
import os
import subprocess

import numpy as np
import pytest

from collider_ref import collide_f32, collide_f64
from tetsim_amd import _capi as capi

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
F32 = np.float32

LAYOUT_C = r"""
#include <stddef.h>
#include <stdio.h>
#include "tetsim.h"
int main(void) {
    printf("%zu %zu %zu %zu %zu %zu %zu %zu %zu %d %d %d %d %d\n", sizeof(TetSimCollider), offsetof(TetSimCollider, kind),
           offsetof(TetSimCollider, reserved), offsetof(TetSimCollider, a), offsetof(TetSimCollider, b), offsetof(TetSimCollider, axes),
           offsetof(TetSimCollider, radius), offsetof(TetSimCollider, friction), offsetof(TetSimCollider, velocity),
           TETSIM_COLLIDER_SPHERE, TETSIM_COLLIDER_CAPSULE, TETSIM_COLLIDER_BOX, TETSIM_COLLIDER_PLANE, TETSIM_MAX_COLLIDERS);
    return 0;
}
"""


def test_collider_struct_layout_matches_the_ctypes_mirror(tmp_path):
    src, exe = tmp_path / "layout.c", tmp_path / "layout"
    src.write_text(LAYOUT_C)
    r = subprocess.run(["gcc", "-std=c99", "-Wall", "-Werror", "-I" + os.path.join(ROOT, "include"), str(src), "-o", str(exe)], capture_output=True, text=True)
    assert r.returncode == 0, r.stderr
    got = [int(x) for x in subprocess.run([str(exe)], capture_output=True, text=True, check=True).stdout.split()]
    T = capi.TetSimCollider
    want = [C.sizeof(T)] + [getattr(T, f).offset for f in ("kind", "reserved", "a", "b", "axes", "radius", "friction", "velocity")] + \
        [capi.COLLIDER_SPHERE, capi.COLLIDER_CAPSULE, capi.COLLIDER_BOX, capi.COLLIDER_PLANE, capi.MAX_COLLIDERS]
    assert got == want
    assert got[0] == 168


def test_set_colliders_is_exported_and_the_abi_version_stays():
    L = capi.lib()
    assert hasattr(L, "tetsim_set_colliders")
    assert L.tetsim_abi_version() == 5
    assert "tetsim_set_colliders" in capi.SYMBOLS


def one(p, q, colliders, dt=0.01, f=collide_f32):
    return f(np.asarray([p], F32), np.asarray([q], F32), colliders, dt)[0]


@pytest.mark.parametrize("f", [collide_f32, collide_f64])
def test_sphere_pushes_out_along_the_radius_and_not_at_its_centre(f):
    s = dict(kind="sphere", a=[0.0, 1.0, 0.0], radius=0.5)
    p = one([0.0, 1.25, 0.0], [0.0, 1.25, 0.0], [s], f=f)
    assert np.array_equal(p, F32([0.0, 1.5, 0.0]))
    assert np.array_equal(one([0.0, 1.0, 0.0], [0.0, 2.0, 0.0], [s], f=f), F32([0.0, 1.0, 0.0]))   # L == 0: no hit
    assert np.array_equal(one([0.0, 1.6, 0.0], [0.0, 2.0, 0.0], [s], f=f), F32([0.0, 1.6, 0.0]))   # outside
    # friction: the tangential slip since the previous substep is removed in proportion min(1, dt * friction)
    s["friction"] = 50.0   # dt * friction = 0.5
    p = one([0.2, 1.25, 0.0], [0.0, 1.25, 0.0], [dict(s, a=[0.2, 1.0, 0.0])], f=f)
    assert np.allclose(p, [0.1, 1.5, 0.0], atol=1e-6)


@pytest.mark.parametrize("f", [collide_f32, collide_f64])
def test_capsule_segment_and_end_caps(f):
    c = dict(kind="capsule", a=[-1.0, 0.5, 0.0], b=[1.0, 0.5, 0.0], radius=0.25)
    assert np.allclose(one([0.3, 0.6, 0.0], [0.3, 0.6, 0.0], [c], f=f), [0.3, 0.75, 0.0], atol=1e-7)      # along the segment
    assert np.allclose(one([1.1, 0.5, 0.0], [1.1, 0.5, 0.0], [c], f=f), [1.25, 0.5, 0.0], atol=1e-7)      # beyond B: the cap round B
    assert np.allclose(one([-1.0, 0.5, -0.1], [-1.0, 0.5, -0.1], [c], f=f), [-1.0, 0.5, -0.25], atol=1e-7)  # at A's end, t = 0
    # a degenerate capsule (A == B) is a sphere: t = 0
    d = dict(kind="capsule", a=[0.0, 0.0, 0.0], b=[0.0, 0.0, 0.0], radius=0.5)
    assert np.allclose(one([0.0, 0.3, 0.0], [0.0, 0.3, 0.0], [d], f=f), [0.0, 0.5, 0.0], atol=1e-7)


@pytest.mark.parametrize("f", [collide_f32, collide_f64])
def test_box_nearest_face_and_ties(f):
    b = dict(kind="box", a=[0.0, 0.0, 0.0], b=[1.0, 0.5, 0.25])
    assert np.allclose(one([0.9, 0.0, 0.0], [0.9, 0.0, 0.0], [b], f=f), [1.0, 0.0, 0.0], atol=1e-7)    # +x face is nearest
    assert np.allclose(one([0.0, -0.4, 0.0], [0.0, -0.4, 0.0], [b], f=f), [0.0, -0.5, 0.0], atol=1e-7)  # -y face
    # a tie of the x and y gaps (0.1 each): the lowest axis wins
    t = dict(kind="box", a=[0.0, 0.0, 0.0], b=[0.5, 0.5, 2.0])
    assert np.allclose(one([0.4, 0.4, 0.0], [0.4, 0.4, 0.0], [t], f=f), [0.5, 0.4, 0.0], atol=1e-7)
    # rotated 90 degrees about z: local x = world y
    r = dict(kind="box", a=[0.0, 0.0, 0.0], b=[1.0, 0.2, 5.0], axes=[[0, 1, 0], [-1, 0, 0], [0, 0, 1]])
    assert np.allclose(one([0.1, 0.0, 0.0], [0.1, 0.0, 0.0], [r], f=f), [0.2, 0.0, 0.0], atol=1e-7)
    assert np.array_equal(one([0.3, 0.0, 0.0], [0.3, 0.0, 0.0], [r], f=f), F32([0.3, 0.0, 0.0]))          # outside: untouched


@pytest.mark.parametrize("f", [collide_f32, collide_f64])
def test_tilted_plane(f):
    n = np.array([1.0, 1.0, 0.0])   # not unit length: the host normalises it
    pl = dict(kind="plane", a=[0.0, 0.0, 0.0], b=n)
    p = one([0.0, -0.2, 0.3], [0.0, -0.2, 0.3], [pl], f=f)
    u = n / np.linalg.norm(n)
    assert abs(float(np.dot(p.astype(np.float64), u))) < 1e-6 and np.allclose(p, [0.1, -0.1, 0.3], atol=1e-6)
    # friction with a moving plane: the slip is measured relative to the plane's velocity
    mv = dict(pl, b=[0.0, 1.0, 0.0], friction=1e9, velocity=[2.0, 0.0, 0.0])
    p = one([0.0, -0.1, 0.0], [0.0, 0.0, 0.0], [mv], dt=0.01, f=f)
    assert np.allclose(p, [0.02, 0.0, 0.0], atol=1e-6)   # dragged along: x = prev.x + V dt


def test_plane_y0_is_the_reference_floor_bit_for_bit():
    """In f32, the plane y = 0 with normal (0, 1, 0), no velocity and the call's friction does what the reference's floor does
    (SoftbodyGPU.js:349-353: p.y = 0; p.xz += (prev - p).xz * min(1, dt * friction)), for points below it with non-zero x and z."""
    rng = np.random.default_rng(7)
    n = 4096
    p = rng.uniform(-2.0, 2.0, (n, 3)).astype(F32)
    p[:, 1] = -rng.uniform(1e-6, 0.5, n).astype(F32)
    q = (p + rng.normal(0, 0.05, (n, 3))).astype(F32)
    for dt, friction in ((1.0 / 60.0 / 20.0, 1000.0), (0.004, 100.0), (0.001, 3.0)):
        dt32 = F32(dt)
        fr = min(F32(1.0), dt32 * F32(friction))
        want = p.copy()
        want[:, 1] = 0.0
        F = q - want
        want[:, 0] = want[:, 0] + F[:, 0] * fr
        want[:, 2] = want[:, 2] + F[:, 2] * fr
        got = collide_f32(p, q, [dict(kind="plane", a=[0, 0, 0], b=[0, 1, 0], friction=friction)], dt)
        assert np.array_equal(got + F32(0.0), want + F32(0.0))   # (+0: up to the sign of a zero)


def test_colliders_apply_in_list_order_and_respect_the_mask():
    a = dict(kind="plane", a=[0, 0, 0], b=[0, 1, 0])
    s = dict(kind="sphere", a=[0.0, 0.1, 0.0], radius=0.2)
    p = np.asarray([[0.05, -0.05, 0.0], [0.05, -0.05, 0.0]], F32)
    got = collide_f32(p, p, [a, s], 0.01, mask=np.array([True, False]))
    step = collide_f32(collide_f32(p, p, [a], 0.01), p, [s], 0.01)   # one pass each, in list order: the sphere acts last
    assert np.array_equal(got[0], step[0]) and np.array_equal(got[1], p[1])
    assert got[0][1] < 0.0 and np.linalg.norm(got[0].astype(np.float64) - [0.0, 0.1, 0.0]) >= 0.2 - 1e-6


# ---- the high-precision reference (collide_exact) and the edge scene the GPU tests plant on a body (tests/test_gpu_collider_pass.py) ----

def _oracle_state(case):
    """the CPU oracle's stand-in for the device state of a case of test_gpu_collider_pass.py: (p0, prev, tets, live, colliders, planted, pp)"""
    from oracle import OracleNH, OraclePJ
    from test_gpu_collider_pass import CASES, WARM, _grab, mesh
    from test_gpu_colliders import DT, GRAB_ID
    name, kw, _, pp = CASES[case]
    v, t = mesh(name)
    live = np.zeros(len(v), bool)
    live[np.unique(t)] = True
    vv = v[:live.sum()] if not live.all() else v          # (the oracle divides 0 / 0 on a particle no tet references: it is the last one)
    orc = OracleNH(vv, t, pp) if kw["solver"] == "neohookean" else OraclePJ(vv, t, pp)
    orc.setGrab(*_grab(v))
    for _ in range(WARM):
        orc.simulate(DT, pp)
    prev = np.array(orc.pos, np.float32)
    orc.simulate(DT, pp)
    p0 = np.array(orc.pos, np.float32)
    if not live.all():
        p0, prev = (np.concatenate([x, np.full((1, 3), np.nan, np.float32)]) for x in (p0, prev))
    from collider_ref import edge_scene
    cols, planted = edge_scene(p0, prev, t, DT, skip=[GRAB_ID] + np.nonzero(~live)[0].tolist())
    return p0, prev, t, live, cols, planted, pp


EDGE_CASES = ["quad-dragon", "fused-lat28", "call-loose", "nh-frame-dragon", "nh-clustered-delaunay400", "floor-quad-floor5"]


@pytest.mark.parametrize("case", EDGE_CASES)
def test_edge_scene_is_sized_by_the_reference_alone(case):
    """On the oracle's positions (they agree with the device's to ~1e-4 m): >= 8 hit particles per entry, fragile particles <= 2 % of the
    hit ones, every planted particle in the state its edge demands, the planted offsets exact -- in both list orders of the spheres."""
    from collider_ref import EPS, collide_exact, f32_view, swapped
    from test_gpu_collider_pass import capsule_regions, check_reference
    from test_gpu_colliders import DT, GRAB_ID
    p0, prev, t, live, cols, planted, pp = _oracle_state(case)
    mask = live.copy()
    mask[GRAB_ID] = False
    assert len(cols) == capi.MAX_COLLIDERS
    for c in cols:                                             # every value is an f32: rows and doubles are the same numbers
        for k in ("a", "b", "radius", "friction", "velocity"):
            x = np.asarray(c.get(k, 0.0), np.float64)
            assert np.array_equal(x, x.astype(F32).astype(np.float64)), (c["kind"], k)
    for order, cs in enumerate((cols, swapped(cols))):
        pl = planted if order == 0 else {k: (i, {0: 1, 1: 0}.get(e, e), w) for k, (i, e, w) in planted.items()}
        ex = collide_exact(p0, prev, cs, DT, mask)
        plm, fragile = check_reference(ex, pl, live, cs)
        assert min(capsule_regions(p0, cs[3], ex["hits"][:, 3])) > 0
        print(case, order, "hits per entry", ex["hits"].sum(0), "fragile", int((fragile & ex["hits"].any(1)).sum()), "max r/L %.3g" % ex["cond"].max())
    # the planted offsets are exact as real numbers: the same in f32, in f64 and under fused multiply-adds
    V = f32_view(cols)
    for what, (i, entry, push) in planted.items():
        x, c = p0[i].astype(np.float64), V[entry]
        if c["kind"] == 2:
            l, g = x - c["a"], c["b"] - np.abs(x - c["a"])
            assert np.array_equal(l.astype(F32).astype(np.float64), l)            # (axis-aligned: l is the subtraction)
            j = int(np.argmax(np.abs(push)))
            assert g[j] == g.min() == float(push[j]) and (l[j] > 0 or (l[j] == 0 and not np.signbit(l[j]))), (what, l, g)
            ties = {"box tie two-way": 2, "box tie three-way": 3, "box zero": 1}[what]
            assert (g == g.min()).sum() == ties and j == int(np.argmin(g)), (what, g)
        elif c["kind"] == 3:
            assert np.array_equal(p0[i], c["a"].astype(F32))
        else:
            assert np.array_equal(p0[i], c["a"].astype(F32)) or np.array_equal(p0[i], c["b"].astype(F32))
            ab = c["b"] - c["a"]                                                  # a + (b - a) * 1 is b itself only if b - a is exact
            assert np.array_equal(ab.astype(F32).astype(np.float64), ab), what
    if case.startswith("floor"):
        assert (p0[:, 1] == 0.0).sum() >= 4


@pytest.mark.parametrize("case", ["quad-dragon", "nh-clustered-delaunay400"])
def test_exact_reference_agrees_with_both_restatements_on_every_decision(case):
    """hit / no hit and the chosen box face, entry by entry, on every particle that is not fragile; on the planted particles (decided by
    an exact equality) as well; the positions within f32 rounding"""
    from collider_ref import EPS, collide_exact, decisions
    from test_gpu_colliders import DT, GRAB_ID
    p0, prev, t, live, cols, planted, pp = _oracle_state(case)
    mask = live.copy()
    mask[GRAB_ID] = False
    ex = collide_exact(p0, prev, cols, DT, mask)
    firm = (ex["margin"] >= EPS) & live
    firm[[i for i, _, _ in planted.values()]] = True
    assert firm.sum() > 0.95 * live.sum()
    for f in (collide_f32, collide_f64):
        hits, face, sign = decisions(p0, prev, cols, DT, f, mask)
        assert np.array_equal(hits[firm], ex["hits"][firm])
        assert np.array_equal(face[firm], ex["face"][firm]) and np.array_equal(sign[firm], ex["sign"][firm])
        got = f(p0, prev, cols, DT, mask).astype(np.float64)
        assert np.abs(got[firm] - ex["pos"][firm]).max() < 16 * 2.0 ** -24 * np.abs(p0[live]).max() * max(1.0, ex["cond"].max())
        for what, (i, entry, push) in planted.items():
            want = p0[i] if push is None else (p0[i] + push).astype(F32)
            assert np.array_equal(got[i].astype(F32), want), (what, f.__name__)
    # the restatement of a generic scene too: a random cloud round the colliders of tests/test_gpu_colliders.py
    from test_gpu_colliders import scene
    rng = np.random.default_rng(3)
    cloud = rng.uniform(-0.6, 0.6, (20000, 3)).astype(F32) + F32([0.0, -0.15, 0.0])
    q = (cloud + rng.normal(0, 0.002, cloud.shape)).astype(F32)
    cs = scene(np.array([[-0.5, 0.0, -0.5], [0.5, 1.0, 0.5]], F32))
    ex = collide_exact(cloud, q, cs, DT)
    firm = ex["margin"] >= EPS
    assert firm.mean() > 0.99 and (ex["hits"].sum(0) > 50).all()
    for f in (collide_f32, collide_f64):
        hits, face, sign = decisions(cloud, q, cs, DT, f)
        assert np.array_equal(hits[firm], ex["hits"][firm]) and np.array_equal(face[firm], ex["face"][firm])
