"""Kinematic colliders on the device (include/tetsim.h tetsim_set_colliders), every path against the composed oracle (collider_ref.py:
the oracle's substep, then the colliders restated in numpy): PRECISE bit for bit, FAST within the tolerances below; the cross-path
equalities the library keeps (one call of n substeps = n calls, batch = solo, partitions = whole, restore = continue) with colliders;
no change when the list is empty or out of reach; the validation of the list."""
import ctypes as C

import numpy as np
import pytest

from collider_ref import collide_f32, nh_substep, pj_substep, pj_velocity
from conftest import load_mesh
from oracle import OracleNH, OraclePJ
from tetsim_amd import SoftBodyHIP, TetSimError, group_step_n, make_lattice
from tetsim_amd import _capi as capi
from tetsim_amd.softbody import make_colliders

pytestmark = pytest.mark.gpu
PP = dict(gravity=-9.81, friction=1000.0, density=1000.0, devCompliance=1e-5, volCompliance=0.0,
          worldBounds=[-2.5, -1.0, -2.5, 2.5, 10.0, 2.5])
DT = (1.0 / 60.0) / 20
FRAMES, SUB = 12, 20   # 240 substeps, one call of 20 per frame (main.js:79-84)


def _same(a, b):
    return np.array_equal(np.asarray(a).view(np.uint32), np.asarray(b).view(np.uint32))


def _rot(ax, ay):
    """rows of R_y(ay) R_x(ax): an orthonormal frame, f64"""
    cx, sx, cy, sy = np.cos(ax), np.sin(ax), np.cos(ay), np.sin(ay)
    rx = np.array([[1, 0, 0], [0, cx, -sx], [0, sx, cx]])
    ry = np.array([[cy, 0, sy], [0, 1, 0], [-sy, 0, cy]])
    return (ry @ rx).T


def scene(v, frame=0):
    """A sphere, a capsule, a rotated box and a tilted plane just below the body, in its fall path; the sphere moves (its velocity
    is set, and its centre advances by it every frame)."""
    lo, hi = v.min(0).astype(np.float64), v.max(0).astype(np.float64)
    c, w = (lo + hi) / 2, hi - lo
    yb = lo[1]
    vs = np.array([0.2, 0.0, -0.1])
    t = frame * SUB * DT
    return [
        dict(kind="sphere", a=[c[0] - 0.25 * w[0] + vs[0] * t, yb - 0.13, c[2] + vs[2] * t], radius=0.12, friction=200.0, velocity=vs),
        dict(kind="capsule", a=[c[0] + 0.1 * w[0], yb - 0.06, c[2] - 0.4 * w[2]], b=[c[0] + 0.3 * w[0], yb - 0.09, c[2] + 0.4 * w[2]], radius=0.04, friction=50.0),
        dict(kind="box", a=[c[0], yb - 0.2, c[2] + 0.2 * w[2]], b=[0.3 * w[0], 0.05, 0.15 * w[2]], axes=_rot(0.17, 0.52), friction=1000.0),
        dict(kind="plane", a=[c[0], yb - 0.22, c[2]], b=[0.2, 1.0, 0.1], friction=5.0),
    ]


def _dragon(y0=None):
    v, t = load_mesh("dragon")
    v = v.copy()
    if y0 is not None:
        v[:, 1] += np.float32(y0) - v[:, 1].min()
    return v, t


def _mesh(name):
    if name == "dragon":
        return _dragon(0.3)
    n = int(name[3:])
    return make_lattice(n, y0=0.3)


GRAB_ID = 5


def _grab(v):
    """particle 5 pinned 0.15 m below where it starts: the body hangs from it, low enough to lie on the colliders"""
    return GRAB_ID, (v[GRAB_ID].astype(np.float64) - [0.0, 0.15, 0.0]).tolist()


def _run_pair(body, orc, v, nh, grab=True, frames=FRAMES, sub=SUB):
    """body and composed oracle side by side, one call of `sub` substeps per frame; returns the max |error| per frame and how many
    particle updates a collider changed (the scene is not vacuous)."""
    if grab:
        body.setGrab(*_grab(v))
        orc.setGrab(*_grab(v))
    errs, hits = [], 0
    for f in range(frames):
        cols = scene(v, f)
        body.setColliders(cols)
        body.simulateSubsteps(sub, DT, PP)
        for _ in range(sub):
            if nh:
                hits += nh_substep(orc, DT, PP, cols)
            else:
                hits += pj_substep(orc, DT, PP, cols, grabbed=(orc.grabId,))
        errs.append(float(np.abs(body.pos.astype(np.float64) - orc.pos).max()))
    return errs, hits


# ---- 1. PRECISE: bit for bit against the composed oracle ---------------------------------------------------------------------------

@pytest.mark.parametrize("mesh", ["dragon", "lat8"])
def test_polar_precise_collider_pass_is_the_restatement_bit_for_bit(mesh):
    """Every substep of 240, from the body's own state: the body with colliders ends the substep exactly where its twin without them
    ends it, moved by the f32 restatement (position and velocity, bit for bit).  (Against the oracle over many substeps the polar
    solver is only as exact as sin(): device and glibc differ in the last ulp for some arguments -- tests/test_gpu_polar.py -- and the
    contacts make those arguments appear; the next test bounds that drift.)"""
    v, t = _mesh(mesh)
    a, b = (SoftBodyHIP(v, t, None, dict(PP), solver="polar", precision="precise") for _ in range(2))
    for body in (a, b):
        body.setGrab(*_grab(v))
    mask = np.ones(len(v), bool)
    mask[GRAB_ID] = False
    hits = 0
    for f in range(FRAMES):
        cols = scene(v, f)
        a.setColliders(cols)
        for _ in range(SUB):
            b.loadState(a.saveState())
            prev = a.pos
            a.simulate(DT, PP)
            b.simulate(DT, PP)
            want = collide_f32(b.pos, prev, cols, DT, mask)
            moved = np.any(want.view(np.uint32) != b.pos.view(np.uint32), axis=1)
            hits += int(moved.sum())
            assert _same(a.pos, want), (f, np.nonzero(np.any(a.pos != want, axis=1))[0][:8])
            want_vel = np.where(moved[:, None], pj_velocity(want, prev, DT, PP["gravity"]), b.vel)
            assert _same(a.vel, want_vel), f
    assert hits > 0


@pytest.mark.parametrize("mesh", ["dragon", "lat8"])
def test_polar_precise_follows_the_composed_oracle(mesh):
    v, t = _mesh(mesh)
    body = SoftBodyHIP(v, t, None, dict(PP), solver="polar", precision="precise")
    orc = OraclePJ(v, t, PP)
    errs, hits = _run_pair(body, orc, v, nh=False)
    print("collider PRECISE polar", mesh, "max error per frame", ["%.2e" % e for e in errs])
    # 3x what the MI355X showed: 4.86e-5 (Dragon), 4.33e-5 (lat8) -- sin() ulps met in the violent first contacts, then fed back
    assert max(errs) < 1.5e-4 and hits > 0, errs


@pytest.mark.parametrize("mesh,order", [("dragon", "original"), ("dragon", "coloured"), ("dragon", "clustered"),
                                        ("lat16", "original"), ("lat16", "coloured"), ("lat16", "clustered")])
def test_neohookean_precise_equals_the_composed_oracle_bit_for_bit(mesh, order):
    v, t = _mesh(mesh)
    body = SoftBodyHIP(v, t, None, dict(PP), solver="neohookean", precision="precise", order=order)
    if mesh == "lat16":
        assert body.numParticles > 4096
    orc = OracleNH(v, t[body.tetOrder] if order != "original" else t, PP)
    errs, hits = _run_pair(body, orc, v, nh=True, frames=10)
    assert _same(body.pos, orc.pos) and _same(body.vel, orc.vel), errs
    assert hits > 0


# ---- 2. FAST: every particle-pass path against the composed oracle ---------------------------------------------------------------
# max |error| (m) over 240 substeps; each bound is 3x the largest per-frame error the MI355X showed (in the comment)
FAST_CASES = {
    # name: (constructor keywords, expected TetSimInfo.fused_particle_pass, tolerance)
    "gather-dragon": (dict(solver="polar", gather=True), 0, 6.8e-4),                # observed 2.26e-4
    "fused-lat28": (dict(solver="polar"), (1, 2), 4.5e-3),                          # observed 1.48e-3
    "frame-lean-dragon": (dict(solver="polar", lean_state=True), 2, 7.7e-4),        # observed 2.57e-4
    "quad-dragon": (dict(solver="polar"), 3, 1.03e-3),                              # observed 3.42e-4
    "nh-frame-dragon": (dict(solver="neohookean", order="original"), 4, 1.7e-4),    # observed 5.64e-5
    "call-lat45": (dict(solver="polar"), 5, 1.8e-3),                                # observed 5.91e-4
    "call-lean-lat45": (dict(solver="polar", lean_state=True), 5, 1.8e-3),          # observed 5.98e-4
    "nh-clustered-lat30": (dict(solver="neohookean", order="clustered"), 0, 7.8e-5),   # observed 2.60e-5
}


@pytest.mark.parametrize("case", list(FAST_CASES))
def test_fast_paths_follow_the_composed_oracle(case):
    kw, path, tol = FAST_CASES[case]
    name = case.split("-")[-1]
    v, t = _mesh(name)
    body = SoftBodyHIP(v, t, None, dict(PP), precision="fast", **kw)
    assert body.info.fused_particle_pass in (path if isinstance(path, tuple) else (path,)), body.info.fused_particle_pass
    nh = kw["solver"] == "neohookean"
    orc = OracleNH(v, t[body.tetOrder] if kw.get("order", "original") != "original" else t, PP) if nh else OraclePJ(v, t, PP, slot_quirk=True)
    errs, hits = _run_pair(body, orc, v, nh=nh)
    print("collider FAST", case, "max error per frame", ["%.2e" % e for e in errs])
    assert np.isfinite(body.pos).all() and max(errs) < tol, errs
    assert hits > 0


def test_fast_partitioned_gather_follows_the_composed_oracle():
    """a partitioned body (two partitions, one process: tetsim_group_step_n) -- every partition applies the list to what it advances"""
    v, t = _mesh("lat12")
    owner = (np.arange(len(v)) * 2 // len(v)).astype(np.int32)
    parts = [SoftBodyHIP(v, t, None, dict(PP), solver="polar", precision="fast", part_count=2, part_index=p, vert_owner=owner) for p in range(2)]
    orc = OraclePJ(v, t, PP, slot_quirk=True)
    errs = []
    for f in range(FRAMES):
        cols = scene(v, f)
        for b in parts:
            b.setColliders(cols)
        group_step_n(parts, SUB, DT, PP)
        for _ in range(SUB):
            pj_substep(orc, DT, PP, cols)
        got = np.empty((len(v), 3), np.float32)
        for b in parts:
            got[b.ownedIds] = b.pos
        errs.append(float(np.abs(got.astype(np.float64) - orc.pos).max()))
    print("collider FAST partitioned-lat12 max error per frame", ["%.2e" % e for e in errs])
    assert max(errs) < 8.9e-3, errs   # observed 2.96e-3


# ---- 3. cross-path bit equality with colliders -----------------------------------------------------------------------------------

@pytest.mark.parametrize("mesh,kw", [("dragon", dict(solver="polar", precision="fast")),
                                     ("dragon", dict(solver="polar", precision="fast", gather=True)),
                                     ("dragon", dict(solver="polar", precision="fast", lean_state=True)),
                                     ("lat45", dict(solver="polar", precision="fast")),
                                     ("dragon", dict(solver="neohookean", precision="fast")),
                                     ("lat30", dict(solver="neohookean", precision="fast", order="clustered")),
                                     ("dragon", dict(solver="neohookean", precision="precise", order="clustered"))])
def test_one_call_of_n_substeps_equals_n_calls(mesh, kw):
    v, t = _mesh(mesh)
    a, b, none = (SoftBodyHIP(v, t, None, dict(PP), **kw) for _ in range(3))
    for body in (a, b, none):
        body.setGrab(*_grab(v))
    for f in range(6):
        cols = scene(v, f)
        a.setColliders(cols)
        b.setColliders(cols)
        a.simulateSubsteps(SUB, DT, PP)
        none.simulateSubsteps(SUB, DT, PP)
        for _ in range(SUB):
            b.simulate(DT, PP)
    assert _same(a.pos, b.pos) and _same(a.vel, b.vel), (mesh, kw)
    assert not _same(a.pos, none.pos)   # the colliders acted


@pytest.mark.parametrize("kw", [dict(solver="polar", precision="fast"), dict(solver="polar", precision="precise"),
                                dict(solver="neohookean", precision="fast"), dict(solver="neohookean", precision="precise")])
def test_each_body_of_a_batch_equals_its_solo_run(kw):
    meshes = [_dragon(0.3), make_lattice(5, y0=0.3), _dragon(0.5)]
    cols = scene(meshes[0][0])
    batch = SoftBodyHIP.batch(meshes, dict(PP), **kw)
    solos = [SoftBodyHIP(v, t, None, dict(PP), **kw) for v, t in meshes]
    for body in [batch] + solos:
        body.setColliders(cols)
        for _ in range(6):
            body.simulateSubsteps(SUB, DT, PP)
    pos = batch.pos
    for (pr, _), solo in zip(batch.bodyRanges, solos):
        assert _same(pos[pr[0]:pr[1]], solo.pos)


@pytest.mark.parametrize("parts", [2, 4])
def test_partitions_in_one_process_equal_the_whole_body(parts):
    v, t = _mesh("lat12")
    owner = (np.arange(len(v)) * parts // len(v)).astype(np.int32)
    mono = SoftBodyHIP(v, t, None, dict(PP), solver="polar", precision="precise")
    group = [SoftBodyHIP(v, t, None, dict(PP), solver="polar", precision="precise", part_count=parts, part_index=p, vert_owner=owner) for p in range(parts)]
    for f in range(8):
        cols = scene(v, f)
        mono.setColliders(cols)
        for b in group:
            b.setColliders(cols)
        mono.simulateSubsteps(SUB, DT, PP)
        group_step_n(group, SUB, DT, PP)
    got = np.empty((len(v), 3), np.float32)
    for b in group:
        got[b.ownedIds] = b.pos
    assert _same(got, mono.pos)


@pytest.mark.parametrize("kw", [dict(solver="polar", precision="fast"), dict(solver="neohookean", precision="precise")])
def test_save_load_continue_equals_an_uninterrupted_run(kw):
    v, t = _mesh("dragon")
    a = SoftBodyHIP(v, t, None, dict(PP), **kw)
    cols = scene(v)
    a.setColliders(cols)
    for _ in range(5):
        a.simulateSubsteps(SUB, DT, PP)
    blob = a.saveState()
    for _ in range(5):
        a.simulateSubsteps(SUB, DT, PP)
    b = SoftBodyHIP(v, t, None, dict(PP), **kw)
    blank = SoftBodyHIP(v, t, None, dict(PP), **kw).saveState()
    assert len(blob) == len(blank)                       # colliders are not solver state
    b.loadState(blob)
    b.setColliders(cols)
    for _ in range(5):
        b.simulateSubsteps(SUB, DT, PP)
    assert _same(a.pos, b.pos) and _same(a.vel, b.vel)


# ---- 4. no change when unused ------------------------------------------------------------------------------------------------------

ALL_PATHS = [("dragon", dict(solver="polar", precision="precise")), ("dragon", dict(solver="polar", precision="fast")),
             ("dragon", dict(solver="polar", precision="fast", gather=True)), ("dragon", dict(solver="polar", precision="fast", lean_state=True)),
             ("lat28", dict(solver="polar", precision="fast")), ("lat45", dict(solver="polar", precision="fast")),
             ("dragon", dict(solver="neohookean", precision="precise")), ("dragon", dict(solver="neohookean", precision="fast")),
             ("lat30", dict(solver="neohookean", precision="fast", order="clustered"))]


@pytest.mark.parametrize("mesh,kw", ALL_PATHS)
def test_cleared_or_out_of_reach_colliders_change_nothing(mesh, kw):
    v, t = _mesh(mesh)
    never, cleared, far = (SoftBodyHIP(v, t, None, dict(PP), **kw) for _ in range(3))
    cleared.setColliders(scene(v))
    cleared.setColliders([])
    far.setColliders([dict(c, a=np.asarray(c["a"]) + [0.0, 50.0, 0.0], b=np.asarray(c.get("b", [0, 0, 0])) + ([0.0, 50.0, 0.0] if c["kind"] == "capsule" else 0.0))
                      if c["kind"] != "plane" else dict(c, a=[0.0, -50.0, 0.0]) for c in scene(v)])
    for body in (never, cleared, far):
        body.setGrab(*_grab(v))
        body.simulateSubsteps(SUB, DT, PP)
        for _ in range(3):
            body.simulate(DT, PP)
        body.simulateSubsteps(SUB, DT, PP)
    assert _same(never.pos, cleared.pos) and _same(never.vel, cleared.vel)
    assert _same(never.pos, far.pos) and _same(never.vel, far.vel)


@pytest.mark.parametrize("kw", [dict(solver="polar", precision="fast"), dict(solver="polar", precision="precise"), dict(solver="neohookean", precision="precise")])
def test_a_new_list_takes_effect_between_calls_with_the_same_params(kw):
    """tetsim_step skips the upload of unchanged parameters: a changed list alone must still reach the device"""
    v, t = _mesh("dragon")
    a = SoftBodyHIP(v, t, None, dict(PP), **kw)
    b = SoftBodyHIP(v, t, None, dict(PP), **kw)
    c = SoftBodyHIP(v, t, None, dict(PP), **kw)
    y = float(v[:, 1].min()) + 0.01
    wall = [dict(kind="plane", a=[0.0, y, 0.0], b=[0.0, 1.0, 0.0], friction=10.0)]   # through the body's lowest centimetre
    for body in (a, b, c):
        body.simulate(DT, PP)
        body.simulate(DT, PP)
    a.setColliders(wall)
    c.setColliders(wall)
    for body in (a, b, c):
        body.simulate(DT, PP)
    assert a.pos[:, 1].min() >= y - 1e-6 and b.pos[:, 1].min() < y and _same(a.pos, c.pos)
    a.setColliders([])                            # ... and so must a cleared one
    for body in (a, b, c):
        body.simulate(DT, PP)
    assert not _same(a.pos, c.pos)


# ---- 5. physics: a body resting on a sphere ------------------------------------------------------------------------------------------

def test_dragon_lands_on_a_sphere_and_stays_out_of_it():
    v, t = _dragon(0.6)
    lo, hi = v.min(0), v.max(0)
    c = (lo + hi) / 2
    ball = dict(kind="sphere", a=[float(c[0]), -0.6, float(c[2])], radius=1.2, friction=500.0)   # a dome wider than the Dragon, top at 0.6
    body = SoftBodyHIP(v, t, None, dict(PP), solver="polar", precision="precise")
    body.setColliders([ball])
    speeds, touched = [], 0
    for f in range(90):
        body.simulateSubsteps(SUB, DT, PP)
        p = body.pos.astype(np.float64)
        inside = ball["radius"] - np.linalg.norm(p - ball["a"], axis=1)
        assert inside.max() <= 1e-5, (f, inside.max())
        touched += int((inside > -1e-3).any())
        speeds.append(float(np.linalg.norm(body.vel, axis=1).mean()))
    assert touched > 60                              # on the sphere for most of the run
    assert max(speeds[60:]) < 2.0 * 9.81 * 0.2       # (slower than the free fall of the first 0.2 s: it is held, not falling through)


# ---- 6. validation ----------------------------------------------------------------------------------------------------------------

BAD = [
    ("too many", [dict(kind="sphere", radius=0.1)] * 9),
    ("unknown kind", [dict(kind=7)]),
    ("reserved", [dict(kind="sphere", radius=0.1, reserved=1)]),
    ("nan", [dict(kind="sphere", a=[0.0, float("nan"), 0.0], radius=0.1)]),
    ("inf in an unused field", [dict(kind="sphere", radius=0.1, axes=[[float("inf"), 0, 0], [0, 1, 0], [0, 0, 1]])]),
    ("negative radius", [dict(kind="capsule", radius=-0.1)]),
    ("negative half-extent", [dict(kind="box", b=[0.1, -0.1, 0.1])]),
    ("negative friction", [dict(kind="plane", b=[0, 1, 0], friction=-1.0)]),
    ("zero normal", [dict(kind="plane", b=[0, 0, 0])]),
    ("zero axis", [dict(kind="box", b=[0.1, 0.1, 0.1], axes=[[1, 0, 0], [0, 0, 0], [0, 0, 1]])]),
    ("skew axes", [dict(kind="box", b=[0.1, 0.1, 0.1], axes=[[1, 0, 0], [0.01, 1, 0], [0, 0, 1]])]),
]


def test_invalid_lists_are_refused_and_the_previous_one_stays():
    v, t = _mesh("dragon")
    good = scene(v)
    a, b, none = (SoftBodyHIP(v, t, None, dict(PP), solver="polar", precision="precise") for _ in range(3))
    a.setColliders(good)
    b.setColliders(good)
    for what, cols in BAD:
        with pytest.raises(TetSimError) as e:
            a.setColliders(cols)
        assert e.value.code == capi.EINVAL, what
    arr = make_colliders([dict(kind="sphere", radius=0.1)])   # a null list with a count
    assert capi.lib().tetsim_set_colliders(a._h, None, 1) == capi.EINVAL and arr is not None
    for _ in range(15):
        for body in (a, b, none):
            body.simulateSubsteps(SUB, DT, PP)
    assert _same(a.pos, b.pos) and not _same(a.pos, none.pos)
    # orthogonal within 1e-5 after normalisation passes; near-parallel axes do not
    a.setColliders([dict(kind="box", b=[0.1, 0.1, 0.1], axes=[[2, 0, 0], [0, 3, 1e-6], [0, 0, 1]])])
