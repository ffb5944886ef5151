"""Body pins (include/tetsim.h: tetsim_set_body_pins / _device): many held particles per body.

No oracle here needs a tolerance.  With one row per body a pin is a body grab, and so the handle's grab of the body alone; two pins are the
two texels a TETSIM_FLAG_REF_GRAB_TEXEL handle holds; a pin per component of a body of two disjoint components is a grab of each component
alone; a body whose every particle is pinned sits on its targets.  Equality is on the bits of pos, vel and, for polar, quats by the caller's
tet id.  Meshes, PP, DT and the path labels are those of test_gpu_colliders.py and test_gpu_body_grabs.py; a frame is one call of 20 substeps."""
import ctypes as C

import numpy as np
import pytest
import torch

from test_gpu_body_grabs import BATCH_CASES, HELD, LARGE_CASES, _bits, _code, _hip_runtime, _path, _same, _same_bodies, _state, _target, _three
from test_gpu_colliders import ALL_PATHS, DT, GRAB_ID, PP, SUB, _dragon, _mesh
from tetsim_amd import SoftBodyHIP, make_lattice, prep_pin_slots
from tetsim_amd import _capi as capi

pytestmark = pytest.mark.gpu

POLAR_FAST = dict(solver="polar", precision="fast")
POLAR_PRECISE = dict(solver="polar", precision="precise")
NH_FAST = dict(solver="neohookean", precision="fast")
NH_PRECISE = dict(solver="neohookean", precision="precise")


def _pins(meshes, held, frame, k=1):
    """the body-grab test's table as pin rows: the held particle in row 0 of k, the other rows unused"""
    p = np.full((len(meshes), k), -1, np.int32)
    x = np.zeros((len(meshes), k, 3), np.float32)
    for b, ((v, _), i) in enumerate(zip(meshes, held)):
        p[b, 0] = i
        x[b, 0] = _target(v, max(i, 0), frame, 0.15 if b == 0 else -0.05)
    return p, x


def _dev(p, x, padded=True):
    dp = torch.tensor(np.asarray(p, np.int32), device="cuda")
    dx = torch.tensor(np.asarray(x, np.float32), device="cuda")
    if padded:   # rows of 16 bytes: the [..., :3] view of a (B, K, 4) tensor
        wide = torch.full(tuple(dx.shape[:2]) + (4,), 7.0, dtype=torch.float32, device="cuda")
        wide[..., :3] = dx
        dx = wide[..., :3]
        assert dx.stride(1) == 4
    return dp, dx


def _frames(bodies, n=1):
    for _ in range(n):
        for b in bodies:
            b.simulateSubsteps(SUB, DT, PP)


# ---- 1. one row per body is the grab, every path --------------------------------------------------------------------------------------
@pytest.mark.parametrize("case", list(BATCH_CASES))
def test_one_pin_per_body_equals_the_solos_with_set_grab(case):
    kw, solo_path, batch_path = BATCH_CASES[case]
    meshes = _three()
    one, four = (SoftBodyHIP.batch(meshes, dict(PP), **kw) for _ in range(2))
    solos = [SoftBodyHIP(v, t, None, dict(PP), **kw) for v, t in meshes]
    _path(one, batch_path)
    _path(solos[0], solo_path)
    for f in range(4):
        p, x = _pins(meshes, HELD, f)
        one.setBodyPins(p, x)
        four.setBodyPins(*_pins(meshes, HELD, f, k=4))
        for solo, i, xi in zip(solos, p[:, 0], x[:, 0]):
            if i >= 0:
                solo.setGrab(int(i), xi)
        _frames([one, four] + solos)
    assert _same_bodies(one, solos) == []
    assert _same(_state(one), _state(four))
    assert np.array_equal(one.pos[GRAB_ID], _pins(meshes, HELD, 3)[1][0, 0])


@pytest.mark.parametrize("case", list(LARGE_CASES))
def test_a_single_body_with_one_pin_equals_its_twin_with_set_grab(case):
    mesh, kw, path = LARGE_CASES[case]
    v, t = _mesh(mesh)
    a, b = (SoftBodyHIP(v, t, None, dict(PP), **kw) for _ in range(2))
    _path(a, path)
    for f in range(3):
        x = _target(v, GRAB_ID, f)
        a.setBodyPins([[GRAB_ID]], [[x]])
        b.setGrab(GRAB_ID, x)
        _frames([a, b])
    assert _same(_state(a), _state(b))
    assert np.array_equal(a.pos[GRAB_ID], _target(v, GRAB_ID, 2))


def test_a_batch_on_the_one_launch_call_with_one_pin_each_equals_its_solos():
    mesh = make_lattice(36, y0=0.3)
    meshes = [mesh, mesh]
    batch = SoftBodyHIP.batch(meshes, dict(PP), **POLAR_FAST)
    _path(batch, 5)
    solos = [SoftBodyHIP(v, t, None, dict(PP), **POLAR_FAST) for v, t in meshes]
    for f in range(2):
        p, x = _pins(meshes, [GRAB_ID, 9], f)
        batch.setBodyPins(p, x)
        for solo, i, xi in zip(solos, p[:, 0], x[:, 0]):
            solo.setGrab(int(i), xi)
        _frames([batch] + solos)
    assert _same_bodies(batch, solos) == []
    assert not np.array_equal(_bits(solos[0].pos), _bits(solos[1].pos))


# ---- 2. two pins against the reference's two-texel grab ---------------------------------------------------------------------------------
def _two_texels(nt, nv):
    out = (C.c_int32 * 2)()
    for gid in range(nv):
        assert capi.lib().tetsim_prep_ref_grab_texels(gid, nt, nv, out) == 0
        if out[0] >= 0 and out[1] >= 0 and out[0] != out[1]:
            return gid, int(out[0]), int(out[1])
    raise AssertionError("no grab id of this mesh selects two texels")


@pytest.mark.parametrize("kw", [POLAR_PRECISE, POLAR_FAST])
def test_two_pins_equal_the_two_texel_grab_of_the_reference(kw):
    v, t = _mesh("dragon")
    gid, p0, p1 = _two_texels(len(t), len(v))
    assert p0 != p1 and p0 >= 0 and p1 >= 0
    pinned = SoftBodyHIP(v, t, None, dict(PP), **kw)
    texel = SoftBodyHIP(v, t, None, dict(PP), ref_grab_texel=True, **kw)
    for f in range(3):
        x = _target(v, p0, f)
        pinned.setBodyPins([[p0, p1]], [[x, x]])
        texel.setGrab(gid, x)
        _frames([pinned, texel])
    assert _same(_state(pinned), _state(texel))
    assert np.array_equal(pinned.pos[p0], _target(v, p0, 2)) and np.array_equal(pinned.pos[p1], _target(v, p0, 2))


# ---- 3. many pins against independent components ---------------------------------------------------------------------------------------
@pytest.mark.parametrize("kw", [dict(POLAR_PRECISE, ref_slot_table=False), dict(NH_PRECISE, order="original")])
def test_a_pin_per_component_equals_the_components_alone_with_set_grab(kw):
    """one mesh of two disjoint lat5 lattices; the control -- nothing held, the halves equal two solo bodies bit for bit -- is asserted first.
    Polar PRECISE runs here with ref_slot_table=False.  With the reference's slot table (the default) the control does not hold, and
    cannot: that table drops the contribution of (tet 0, corner 0) of the HANDLE's mesh (host_prep.cpp: build_incidence, SoftbodyGPU.js's
    `<= 0.0` test), so the second lattice alone loses its first tet's first corner and the same lattice as the second component of a
    concatenation keeps it -- measured on an MI355X after two calls of 20 substeps: the first half's pos, vel and quats equal the solo's
    bit for bit, all 216 particles of the second half differ; with ref_slot_table=False both halves equal their solos.  Without that one
    quirk the two are the same computation."""
    va, ta = make_lattice(5, y0=0.3)
    vb = (va.astype(np.float64) + [1.5, 0.2, 0.0]).astype(np.float32)
    v, t = np.concatenate([va, vb]), np.concatenate([ta, ta + len(va)])
    n, nt = len(va), len(ta)

    def halves_equal(both, solos):
        ok = True
        q = None
        if both.solver == "polar":
            q = np.empty_like(both.quats)
            q[both.localTets] = both.quats
        for k, solo in enumerate(solos):
            same = [np.array_equal(_bits(both.pos[k * n:(k + 1) * n]), _bits(solo.pos)), np.array_equal(_bits(both.vel[k * n:(k + 1) * n]), _bits(solo.vel))]
            print("component", k, "pos equal", same[0], "vel equal", same[1])
            ok = ok and all(same)
            if q is not None:
                qs = np.empty_like(solo.quats)
                qs[solo.localTets] = solo.quats
                print("component", k, "quats equal", np.array_equal(_bits(q[k * nt:(k + 1) * nt]), _bits(qs)))
                ok = ok and np.array_equal(_bits(q[k * nt:(k + 1) * nt]), _bits(qs))
        return ok

    def make():
        return SoftBodyHIP(v, t, None, dict(PP), **kw), [SoftBodyHIP(va, ta, None, dict(PP), **kw), SoftBodyHIP(vb, ta, None, dict(PP), **kw)]

    both, solos = make()
    _frames([both] + solos, 2)
    assert halves_equal(both, solos), "control: two disjoint components do not step as two bodies"
    both, solos = make()
    for f in range(3):
        xa, xb = _target(va, 7, f), _target(vb, 33, f, drop=-0.05)
        both.setBodyPins([[7, n + 33]], [[xa, xb]])
        solos[0].setGrab(7, xa)
        solos[1].setGrab(33, xb)
        _frames([both] + solos)
    assert halves_equal(both, solos)
    assert np.array_equal(both.pos[7], _target(va, 7, 2)) and np.array_equal(both.pos[n + 33], _target(vb, 33, 2, drop=-0.05))


# ---- 4. a fully pinned body follows its targets -----------------------------------------------------------------------------------------
@pytest.mark.parametrize("kw", [POLAR_FAST, POLAR_PRECISE, NH_FAST, NH_PRECISE])
def test_a_fully_pinned_body_sits_on_its_targets_and_its_neighbour_is_free(kw):
    v, t = make_lattice(3, y0=0.3)
    nv = len(v)
    batch = SoftBodyHIP.batch([(v, t), (v, t)], dict(PP), **kw)
    free = SoftBodyHIP(v, t, None, dict(PP), **kw)
    p = np.full((2, nv), -1, np.int32)
    p[0] = np.arange(nv)
    for f in range(3):
        x = np.zeros((2, nv, 3), np.float32)
        x[0] = (v.astype(np.float64) + [0.01 * f, 0.02 * f, -0.005 * f]).astype(np.float32)
        batch.setBodyPins(p, x)
        _frames([batch, free])
        assert np.array_equal(_bits(batch.pos[:nv]), _bits(x[0])), f
    assert _same_bodies(batch, [free, free]) == [0]


# ---- 5. boundaries ----------------------------------------------------------------------------------------------------------------------
def _boundary_meshes():
    return [make_lattice(2, y0=0.3 + 0.01 * b) for b in range(6)] + [_dragon(0.3)]


def _boundary_table(meshes, frame):
    k = 6
    p = np.full((len(meshes), k), -1, np.int32)
    x = np.zeros((len(meshes), k, 3), np.float32)
    for b, (v, t) in enumerate(meshes):
        ids = [0, len(v) - 1] if b < 6 else [0, len(v) - 1] + [int(i) for i in t[0]]
        ids = list(dict.fromkeys(ids))
        for j, i in enumerate(ids):
            p[b, j] = i
            x[b, j] = _target(v, i, frame, drop=0.02 * (j + 1))
    return p, x


@pytest.mark.parametrize("kw", [POLAR_FAST, dict(POLAR_FAST, lean_state=True), NH_FAST])
def test_pins_at_the_edges_of_bodies_waves_and_tets(kw):
    meshes = _boundary_meshes()
    assert len(meshes[0][0]) == 27
    batch = SoftBodyHIP.batch(meshes, dict(PP), **kw)
    solos = [SoftBodyHIP(v, t, None, dict(PP), **kw) for v, t in meshes]
    for f in range(2):
        p, x = _boundary_table(meshes, f)
        batch.setBodyPins(p, x)
        for b, solo in enumerate(solos):
            solo.setBodyPins(p[b:b + 1], x[b:b + 1])
        _frames([batch] + solos)
    assert _same_bodies(batch, solos) == []
    pos = batch.pos
    for b, ((p0, _), _) in enumerate(batch.bodyRanges):
        for i, xi in zip(p[b], x[b]):
            if i >= 0:
                assert np.array_equal(pos[p0 + i], xi), (b, i)


def test_one_call_of_n_substeps_equals_n_calls_with_many_pins_on_the_call_kernel():
    v, t = _mesh("lat45")
    nv = len(v)
    a, b = (SoftBodyHIP(v, t, None, dict(PP), **POLAR_FAST) for _ in range(2))
    _path(a, 5)
    ids = np.unique(np.concatenate([[0, nv - 1], np.linspace(1, nv - 2, 64).astype(np.int64)])).astype(np.int32)
    assert len(ids) == 66
    x = np.stack([_target(v, i, 0, drop=0.05) for i in ids])
    for body in (a, b):
        body.setBodyPins(ids[None], x[None])
    a.simulateSubsteps(SUB, DT, PP)
    for _ in range(SUB):
        b.simulate(DT, PP)
    assert _same(_state(a), _state(b))
    assert np.array_equal(_bits(a.pos[ids]), _bits(x))


# ---- 6. order and duplicates; device rows = host rows -----------------------------------------------------------------------------------
@pytest.mark.parametrize("kw", [POLAR_FAST, NH_PRECISE])
def test_row_order_does_not_matter_and_duplicates_go_to_the_lowest_row(kw):
    meshes = _three()
    counts = [len(v) for v, _ in meshes]
    rng = np.random.default_rng(5)
    k = 5
    p = np.stack([rng.choice(n, k, replace=False) for n in counts]).astype(np.int32)
    x = np.stack([np.stack([_target(v, i, 0, drop=0.03 * (j + 1)) for j, i in enumerate(row)]) for (v, _), row in zip(meshes, p)])
    perm = rng.permutation(k)
    plain, permuted, dup_host, dup_dev, reduced = (SoftBodyHIP.batch(meshes, dict(PP), **kw) for _ in range(5))
    plain.setBodyPins(p, x)
    permuted.setBodyPins(p[:, perm], x[:, perm])
    # duplicates: rows 3 and 4 name the particles of rows 0 and 1 again, elsewhere
    pd, xd = p.copy(), x.copy()
    pd[:, 3], pd[:, 4] = p[:, 0], p[:, 1]
    xd[:, 3:] += 0.5
    slots = prep_pin_slots(pd, xd, counts)
    won = np.zeros(pd.size, bool)
    won[slots[slots >= 0]] = True
    pr = np.where(won.reshape(pd.shape), pd, -1).astype(np.int32)
    assert (pr[:, 3:] == -1).all() and (pr[:, :3] == pd[:, :3]).all()
    dup_host.setBodyPins(pd, xd)
    dup_dev.setBodyPinsDevice(*_dev(pd, xd))
    reduced.setBodyPins(pr, xd)
    _frames([plain, permuted, dup_host, dup_dev, reduced], 2)
    assert _same(_state(plain), _state(permuted))
    assert _same(_state(dup_host), _state(reduced)) and _same(_state(dup_dev), _state(reduced))
    assert not _same(_state(plain), _state(reduced))   # (rows 3 and 4 of `plain` hold particles of their own)


@pytest.mark.parametrize("kw", [POLAR_FAST, NH_PRECISE])
def test_device_rows_equal_host_rows(kw):
    meshes = _three()
    held = [GRAB_ID, 11, 3]
    host, dev, masked, side, want = (SoftBodyHIP.batch(meshes, dict(PP), **kw) for _ in range(5))
    stream = torch.cuda.Stream()
    big = torch.randn(2048, 2048, device="cuda")
    keep = []

    def table(f):
        p, x = _pins(meshes, held, f, k=3)
        for b, (v, _) in enumerate(meshes):   # a second pin per body
            p[b, 2] = 20 + b
            x[b, 2] = _target(v, 20 + b, f, drop=0.02)
        return p, x

    for f in range(3):
        p, x = table(f)
        host.setBodyPins(p, x)
        dev.setBodyPinsDevice(*_dev(p, x))
        if f == 0:
            masked.setBodyPinsDevice(*_dev(p, x, padded=False))
        else:   # the mask: body 1 keeps the rows of frame 0
            wp, wx = p.copy(), x.copy()
            wp[1] = [2, 5, -1]
            wx[1] += 1.0
            masked.setBodyPinsDevice(*_dev(wp, wx), bodies=torch.tensor([True, False, True], device="cuda"))
        src_p, src_x = _dev(p, x, padded=False)
        torch.cuda.current_stream().synchronize()
        with torch.cuda.stream(stream):   # rows that kernels on a side stream fill, behind other work of that stream
            keep.append(big @ big)
            tp, tx = torch.empty_like(src_p), torch.empty_like(src_x)
            tp.copy_(src_p)
            tx.copy_(src_x * 1.0)
            side.setBodyPinsDevice(tp, tx, stream=stream)
        wp, wx = table(f)
        wp[1], wx[1] = table(0)[0][1], table(0)[1][1]
        want.setBodyPins(wp, wx)
        _frames([host, dev, masked, side, want])
    assert _same(_state(host), _state(dev)) and _same(_state(host), _state(side))
    assert _same(_state(masked), _state(want)) and not _same(_state(masked), _state(host))
    stream.synchronize()


# ---- 7. rows the device refuses ---------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("kw", [POLAR_FAST, NH_FAST])
def test_a_row_the_device_refuses_holds_nothing_and_disturbs_nobody(kw):
    meshes = _three()
    counts = [len(v) for v, _ in meshes]
    p, x = _pins(meshes, [GRAB_ID, 11, 3], 0, k=2)
    for b, (v, _) in enumerate(meshes):
        p[b, 1] = 30 + b
        x[b, 1] = _target(v, 30 + b, 0, drop=0.02)
    nan = x.copy()
    nan[2, 1, 1] = np.nan
    over, under = p.copy(), p.copy()
    over[0, 0] = counts[0]
    under[1, 1] = -7
    for row, particles, targets in (((0, 0), over, x), ((1, 1), under, x), ((2, 1), p, nan)):
        got, want = (SoftBodyHIP.batch(meshes, dict(PP), **kw) for _ in range(2))
        got.setBodyPinsDevice(*_dev(particles, targets))
        ok = p.copy()
        ok[row] = -1
        want.setBodyPins(ok, x)
        _frames([got, want], 2)
        assert _same(_state(got), _state(want)), row
        got.close()
        want.close()


# ---- 8. OFF is free of effects ----------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("mesh,kw", ALL_PATHS)
def test_pins_that_are_off_or_empty_change_nothing(mesh, kw):
    v, t = _mesh(mesh)
    never, empty, toggled = (SoftBodyHIP(v, t, None, dict(PP), **kw) for _ in range(3))
    x = _target(v, GRAB_ID, 0)
    empty.setBodyPins([[-1, -1]], [[x, x]])
    toggled.setBodyPins([[GRAB_ID, 7]], [[x, x]])
    toggled.setBodyPins(None, None)

    def frame(body):
        body.simulateSubsteps(SUB, DT, PP)
        for _ in range(3):
            body.simulate(DT, PP)
        body.simulateSubsteps(SUB, DT, PP)

    for body in (never, empty, toggled):
        frame(body)
    assert _same(_state(never), _state(empty)) and _same(_state(never), _state(toggled))
    empty.setBodyPins(None, None)
    for body in (never, toggled):   # ... the handle's own grab works as ever afterwards, and so do the body grabs
        body.setGrab(GRAB_ID, x)
        frame(body)
    empty.setBodyGrabs([GRAB_ID], [x])
    frame(empty)
    assert _same(_state(never), _state(toggled)) and _same(_state(never), _state(empty))
    assert np.array_equal(never.pos[GRAB_ID], x)


# ---- 9. a new table between calls with unchanged parameters ---------------------------------------------------------------------------------
@pytest.mark.parametrize("kw", [POLAR_FAST, POLAR_PRECISE, NH_PRECISE])
def test_a_new_table_takes_effect_between_calls_with_the_same_params(kw):
    """tetsim_step skips the upload of unchanged parameters: new targets, new particles or another per_body alone must still reach the kernels"""
    v, t = _mesh("dragon")
    a, twin = (SoftBodyHIP(v, t, None, dict(PP), **kw) for _ in range(2))
    x0, x1, x2 = _target(v, GRAB_ID, 0), _target(v, GRAB_ID, 5), _target(v, 7, 9)
    tables = [([[GRAB_ID, -1]], [[x0, x0]], GRAB_ID, x0),          # the first table
              ([[GRAB_ID, -1]], [[x1, x0]], GRAB_ID, x1),          # only a target
              ([[7, -1]], [[x1, x0]], 7, x1),                      # only a particle
              ([[-1, -1, 7]], [[x0, x0, x2]], 7, x2)]              # another per_body
    for p, x, gid, gx in tables:
        a.setBodyPins(p, x)
        twin.setGrab(gid, gx)
        for body in (a, twin):
            body.simulate(DT, PP)
            body.simulate(DT, PP)
        assert _same(_state(a), _state(twin)), p
        assert np.array_equal(a.pos[gid], gx)


def test_pins_switched_on_behind_calls_of_the_frame_kernel_reach_the_fused_kernels():
    """a body of the persistent 256-tet frame kernel leaves it while pins are on: frame kernel, then pins, then the frame kernel again"""
    v, t = _mesh("lat28")
    a, twin = (SoftBodyHIP(v, t, None, dict(PP), **POLAR_FAST) for _ in range(2))
    _path(a, (1, 2))
    _frames([a, twin], 2)                      # nothing held: both on their usual path
    for body in (a, twin):
        body.simulate(DT, PP)
    for f in range(2):
        x = _target(v, GRAB_ID, f)
        a.setBodyPins([[GRAB_ID, -1]], [[x, x]])
        twin.setGrab(GRAB_ID, x)
        _frames([a, twin])
        for body in (a, twin):
            body.simulate(DT, PP)
    assert _same(_state(a), _state(twin))
    assert np.array_equal(a.pos[GRAB_ID], _target(v, GRAB_ID, 1))
    a.setBodyPins(None, None)
    twin.endGrab()
    _frames([a, twin], 2)
    assert _same(_state(a), _state(twin))


# ---- 10. state --------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("kw", [POLAR_FAST, NH_PRECISE])
def test_checkpoints_and_snapshots_do_not_hold_the_table(kw):
    meshes = [_dragon(0.3), _dragon(0.5)]
    p, x = _pins(meshes, [GRAB_ID, 11], 0, k=2)
    p[:, 1] = [40, 41]
    x[0, 1], x[1, 1] = _target(meshes[0][0], 40, 0), _target(meshes[1][0], 41, 0)
    a, b, c = (SoftBodyHIP.batch(meshes, dict(PP), **kw) for _ in range(3))
    blank = len(a.saveState())

    def device_bytes(body):   # (asked afresh: body.info is the record of the handle's creation)
        info = capi.TetSimInfo()
        capi.check(capi.lib().tetsim_get_info(body._h, C.byref(info)), body._h)
        return int(info.device_bytes)

    def snapshot_bytes(body):
        before = device_bytes(body)
        snap = body.snapshot()
        grown = device_bytes(body) - before
        snap.close()
        return grown

    blank_snapshot = snapshot_bytes(a)
    assert blank_snapshot > 0
    before_table = device_bytes(a)
    a.setBodyPins(p, x)
    assert device_bytes(a) > before_table       # the table is the handle's and counts into device_bytes ...
    _frames([a], 2)
    blob = a.saveState()
    assert len(blob) == blank
    assert snapshot_bytes(a) == blank_snapshot   # ... and a snapshot holds none of it
    _frames([a], 2)
    b.loadState(blob)
    b.setBodyPins(p, x)
    _frames([b], 2)
    assert _same(_state(a), _state(b))
    # a masked restore leaves the table alone: c sets it again behind the restore, a does not
    c.loadState(a.saveState())
    c.setBodyPins(p, x)
    snap_a, snap_c = a.snapshot(), c.snapshot()
    for body, snap in ((a, snap_a), (c, snap_c)):
        body.simulateSubsteps(SUB, DT, PP)
        body.restore(snap, bodies=[True, False])
    c.setBodyPins(p, x)
    _frames([a, c])
    assert _same(_state(a), _state(c))
    assert np.array_equal(a.pos[40], x[0, 1])


# ---- 11. errors -------------------------------------------------------------------------------------------------------------------------
def test_one_kind_of_hold_at_a_time():
    v, t = _mesh("dragon")
    x = _target(v, GRAB_ID, 0)
    a = SoftBodyHIP(v, t, None, dict(PP), **POLAR_FAST)
    dp, dx = _dev([[GRAB_ID]], [[x]])
    a.setBodyPins([[GRAB_ID]], [[x]])
    assert _code(a.setGrab, GRAB_ID, x) == capi.ESTATE
    assert _code(a.startGrab, x) == capi.ESTATE
    assert _code(a.startGrabRay, [0.0, 5.0, 0.0], [0.0, -1.0, 0.0]) == capi.ESTATE
    assert _code(a.setBodyGrabs, [GRAB_ID], [x]) == capi.ESTATE
    assert _code(a.setBodyGrabsDevice, dp[0], dx[0]) == capi.ESTATE
    a.endGrab()                         # releasing the handle's grab stays legal
    a.setBodyPins(None, None)
    a.setGrab(GRAB_ID, x)               # with pins off the handle's grab is back ...
    assert _code(a.setBodyPins, [[GRAB_ID]], [[x]]) == capi.ESTATE
    assert _code(a.setBodyPinsDevice, dp, dx) == capi.ESTATE
    a.endGrab()
    a.setBodyGrabs([GRAB_ID], [x])      # ... and so are the body grabs
    assert _code(a.setBodyPins, [[GRAB_ID]], [[x]]) == capi.ESTATE
    assert _code(a.setBodyPinsDevice, dp, dx) == capi.ESTATE
    a.setBodyGrabs(None, None)
    a.setBodyPinsDevice(dp, dx)
    texel = SoftBodyHIP(v, t, None, dict(PP), ref_grab_texel=True, **POLAR_PRECISE)
    assert _code(texel.setBodyPins, [[GRAB_ID]], [[x]]) == capi.ESTATE
    assert _code(texel.setBodyPinsDevice, dp, dx) == capi.ESTATE
    lv, lt = _mesh("lat12")
    owner = (np.arange(len(lv)) * 2 // len(lv)).astype(np.int32)
    part = SoftBodyHIP(lv, lt, None, dict(PP), part_count=2, part_index=0, vert_owner=owner, **POLAR_FAST)
    assert _code(part.setBodyPins, [[GRAB_ID]], [[x]]) == capi.ESTATE
    assert _code(part.setBodyPinsDevice, dp, dx) == capi.ESTATE


def test_invalid_rows_and_pointers_are_refused_and_the_previous_table_stays():
    L = capi.lib()
    meshes = _three()
    a, b = (SoftBodyHIP.batch(meshes, dict(PP), **POLAR_FAST) for _ in range(2))
    p, x = _pins(meshes, [GRAB_ID, 11, 3], 0, k=2)
    a.setBodyPins(p, x)
    b.setBodyPins(p, x)
    nan, inf, over, under = x.copy(), x.copy(), p.copy(), p.copy()
    nan[1, 0, 2] = np.nan               # (in rows that are in use: an unused row's target is not looked at)
    inf[0, 0, 0] = np.inf
    over[0, 1] = len(meshes[0][0])
    under[1, 0] = -2
    for particles, targets in ((over, x), (under, x), (p, nan), (p, inf)):
        assert _code(a.setBodyPins, particles, targets) == capi.EINVAL
    h = a._h
    dp, dx = _dev(p, x, padded=False)
    host_p, host_x = np.ascontiguousarray(p, np.int32), np.ascontiguousarray(x, np.float32)
    hip = _hip_runtime()
    short = C.c_void_p()
    assert hip.hipMalloc(C.byref(short), C.c_size_t(6 * 12 - 4)) == 0   # an allocation of its own, one float too short for six rows
    P, X = dp.data_ptr(), dx.data_ptr()
    cases = [((P, None, 0, 2, None), "null"), ((P, X, 0, 0, None), "per_body"),
             ((P, X, 8, 2, None), "target_stride"), ((P, X, 14, 2, None), "target_stride"),
             ((P + 2, X, 0, 2, None), "aligned"), ((P, X + 1, 0, 2, None), "aligned"),
             ((host_p.ctypes.data, X, 0, 2, None), "not device memory"), ((P, host_x.ctypes.data, 0, 2, None), "not device memory"),
             ((P, X, 0, 2, host_p.ctypes.data), "not device memory"),
             ((P, short.value, 0, 2, None), "do not fit"), ((P, short.value, 16, 2, None), "do not fit")]
    for args, text in cases:
        rc = L.tetsim_set_body_pins_device(h, *args, None)
        assert rc == capi.EINVAL, (args, rc, L.tetsim_last_error(h))
        assert text.encode() in L.tetsim_last_error(h), (args, L.tetsim_last_error(h))
    assert L.tetsim_set_body_pins_device(None, P, X, 0, 2, None, None) == capi.EINVAL
    assert L.tetsim_set_body_pins(h, host_p.ctypes.data_as(C.POINTER(C.c_int32)), None, 2) == capi.EINVAL
    assert L.tetsim_set_body_pins(h, host_p.ctypes.data_as(C.POINTER(C.c_int32)), host_x.ctypes.data_as(C.POINTER(C.c_float)), 0) == capi.EINVAL
    # tensors the binding can see through
    for bad in ((dp[:2], dx[:2]), (dp.to(torch.int64), dx), (dp, dx[:, :1]), (dp, dx.to(torch.float64))):
        with pytest.raises(ValueError):
            a.setBodyPinsDevice(*bad)
    with pytest.raises(ValueError):
        a.setBodyPins(p[:2], x[:2])
    # every refusal left the table in force: a still steps like b
    _frames([a, b], 2)
    assert _same(_state(a), _state(b))
    assert np.array_equal(a.pos[GRAB_ID], x[0, 0])
    torch.cuda.synchronize()
    assert hip.hipFree(short) == 0
