"""Body grabs (include/tetsim.h: tetsim_set_body_grabs / _device) and the per-body nearest query (tetsim_nearest_particles_device).

The oracle needs no tolerance: body b of a batch with row (i, x) must give the bits that body b alone gives with setGrab(i, x) -- on
every stepping path, for both solvers and both precisions.  Equality is on the bits of pos, vel and, for polar, quats.  Meshes, PP, DT and
the path labels are those of test_gpu_colliders.py; a frame is one call of 20 substeps."""
import ctypes as C

import numpy as np
import pytest
import torch

from test_gpu_colliders import ALL_PATHS, DT, GRAB_ID, PP, SUB, _dragon, _mesh
from tetsim_amd import SoftBodyHIP, TetSimError, make_lattice
from tetsim_amd import _capi as capi

pytestmark = pytest.mark.gpu


def _bits(a):
    return np.ascontiguousarray(a).view(np.uint32)


def _state(body):
    s = [body.pos, body.vel]
    if body.solver == "polar":
        s.append(body.quats)
    return s


def _same(a, b):
    return all(np.array_equal(_bits(x), _bits(y)) for x, y in zip(a, b))


def _same_bodies(batch, solos):
    """every body of the batch against its solo run: pos, vel and (polar) quats, bit for bit; returns the bodies that differ"""
    pos, vel = batch.pos, batch.vel
    quats = None
    if batch.solver == "polar":   # quats come in each handle's own tet order: compare them by the caller's tet id
        quats = np.empty_like(batch.quats)
        quats[batch.localTets] = batch.quats
    bad = []
    for b, (((p0, p1), (e0, e1)), solo) in enumerate(zip(batch.bodyRanges, solos)):
        ok = np.array_equal(_bits(pos[p0:p1]), _bits(solo.pos)) and np.array_equal(_bits(vel[p0:p1]), _bits(solo.vel))
        if quats is not None:
            qs = np.empty_like(solo.quats)
            qs[solo.localTets] = solo.quats
            ok = ok and np.array_equal(_bits(quats[e0:e1]), _bits(qs))
        if not ok:
            bad.append(b)
    return bad


def _path(body, want):
    got = body.info.fused_particle_pass
    assert got in (want if isinstance(want, tuple) else (want,)), (got, want)


def _target(v, particle, frame, drop=0.15):
    """`drop` below where the particle starts, moved 1 cm per frame"""
    return (v[particle].astype(np.float64) - [0.0, drop, 0.0] + [0.01 * frame, 0.0, 0.0]).astype(np.float32)


def _three():
    return [_dragon(0.3), make_lattice(5, y0=0.3), _dragon(0.5)]


HELD = [GRAB_ID, 11, -1]   # body 0 by particle 5, body 1 by another one, body 2 not at all


def _table(meshes, held, frame):
    return (np.asarray(held, np.int32),
            np.stack([_target(v, max(p, 0), frame, 0.15 if b == 0 else -0.05) for b, ((v, _), p) in enumerate(zip(meshes, held))]))


def _step_against_solos(batch, solos, meshes, held, frames, set_rows=None):
    for f in range(frames):
        p, x = _table(meshes, held, f)
        (set_rows or batch.setBodyGrabs)(p, x)
        batch.simulateSubsteps(SUB, DT, PP)
        for solo, i, xi in zip(solos, p, x):
            if i >= 0:
                solo.setGrab(int(i), xi)
            solo.simulateSubsteps(SUB, DT, PP)


# ---- 1. batch = solos, every path -----------------------------------------------------------------------------------------------------
# (constructor keywords, path of the Dragon alone, path of the batch)
BATCH_CASES = {
    "polar-precise": (dict(solver="polar", precision="precise"), 0, 0),
    "polar-fast": (dict(solver="polar", precision="fast"), 3, 3),
    "polar-fast-gather": (dict(solver="polar", precision="fast", gather=True), 0, 0),
    "polar-fast-lean": (dict(solver="polar", precision="fast", lean_state=True), 2, 2),
    "nh-precise-original": (dict(solver="neohookean", precision="precise", order="original"), 4, 4),
    "nh-precise-clustered": (dict(solver="neohookean", precision="precise", order="clustered"), 0, 0),
    "nh-fast": (dict(solver="neohookean", precision="fast"), 4, 4),
    "nh-fast-clustered": (dict(solver="neohookean", precision="fast", order="clustered"), 0, 0),
}


@pytest.mark.parametrize("case", list(BATCH_CASES))
def test_each_body_of_a_batch_equals_its_solo_run_with_set_grab(case):
    kw, solo_path, batch_path = BATCH_CASES[case]
    meshes = _three()
    batch, free = (SoftBodyHIP.batch(meshes, dict(PP), **kw) for _ in range(2))
    solos = [SoftBodyHIP(v, t, None, dict(PP), **kw) for v, t in meshes]
    print("body grabs", case, "paths: batch", batch.info.fused_particle_pass, "solos", [s.info.fused_particle_pass for s in solos])
    _path(batch, batch_path)
    _path(solos[0], solo_path)
    _step_against_solos(batch, solos, meshes, HELD, 6)
    for _ in range(6):
        free.simulateSubsteps(SUB, DT, PP)
    assert _same_bodies(batch, solos) == []
    assert _same_bodies(free, solos) == [0, 1]   # the held bodies differ from an unheld run, the third one does not


# ---- 2. the large paths on a single body ------------------------------------------------------------------------------------------------
LARGE_CASES = {
    "fused-lat28": ("lat28", dict(solver="polar", precision="fast"), (1, 2)),
    "call-lat45": ("lat45", dict(solver="polar", precision="fast"), 5),
    "call-lean-lat45": ("lat45", dict(solver="polar", precision="fast", lean_state=True), 5),
    "nh-levels-lat16": ("lat16", dict(solver="neohookean", precision="precise"), 0),
    "nh-clustered-lat30": ("lat30", dict(solver="neohookean", precision="fast", order="clustered"), 0),
}


@pytest.mark.parametrize("case", list(LARGE_CASES))
def test_a_single_body_with_its_row_equals_its_twin_with_set_grab(case):
    mesh, kw, path = LARGE_CASES[case]
    v, t = _mesh(mesh)
    a, b = (SoftBodyHIP(v, t, None, dict(PP), **kw) for _ in range(2))
    _path(a, path)
    assert a.info.num_bodies == 1
    if mesh == "lat16":
        assert a.numParticles > 4096   # level launches, not the single-workgroup call
    for f in range(3):
        x = _target(v, GRAB_ID, f)
        a.setBodyGrabs([GRAB_ID], [x])
        b.setGrab(GRAB_ID, x)
        a.simulateSubsteps(SUB, DT, PP)
        b.simulateSubsteps(SUB, DT, PP)
    assert _same(_state(a), _state(b))
    assert np.array_equal(a.pos[GRAB_ID], _target(v, GRAB_ID, 2))


def test_a_batch_on_the_one_launch_call_equals_its_solos():
    """two equal lattices: 36 cells is the smallest for which the batch has the 2,048 tiles of the one-launch call (35: 2,010; 36: 2,188)"""
    mesh = make_lattice(36, y0=0.3)
    meshes = [mesh, mesh]
    kw = dict(solver="polar", precision="fast")
    batch = SoftBodyHIP.batch(meshes, dict(PP), **kw)
    _path(batch, 5)
    solos = [SoftBodyHIP(v, t, None, dict(PP), **kw) for v, t in meshes]
    _step_against_solos(batch, solos, meshes, [GRAB_ID, 9], 3)
    assert _same_bodies(batch, solos) == []
    assert not np.array_equal(_bits(solos[0].pos), _bits(solos[1].pos))


# ---- 3. one call of n = n calls ---------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("mesh,kw,path,frames", [("dragon", dict(solver="polar", precision="fast"), 3, 6),
                                                 ("dragon", dict(solver="polar", precision="fast", lean_state=True), 2, 6),
                                                 ("lat45", dict(solver="polar", precision="fast"), 5, 3),
                                                 ("dragon", dict(solver="neohookean", precision="fast"), 4, 6),
                                                 ("dragon", dict(solver="neohookean", precision="precise", order="clustered"), 0, 6)])
def test_one_call_of_n_substeps_equals_n_calls(mesh, kw, path, frames):
    v, t = _mesh(mesh)
    a, b = (SoftBodyHIP(v, t, None, dict(PP), **kw) for _ in range(2))
    _path(a, path)
    for f in range(frames):
        x = _target(v, GRAB_ID, f)
        a.setBodyGrabs([GRAB_ID], [x])
        b.setBodyGrabs([GRAB_ID], [x])
        a.simulateSubsteps(SUB, DT, PP)
        for _ in range(SUB):
            b.simulate(DT, PP)
    assert _same(_state(a), _state(b))
    assert np.array_equal(a.pos[GRAB_ID], _target(v, GRAB_ID, frames - 1))


# ---- 4. device variant = host variant ---------------------------------------------------------------------------------------------------
def _dev(particles, targets, padded=True):
    p = torch.tensor(np.asarray(particles, np.int32), device="cuda")
    x = torch.tensor(np.asarray(targets, np.float32), device="cuda")
    if padded:   # rows of 16 bytes: the [:, :3] view of a (B, 4) tensor
        wide = torch.full((len(particles), 4), 7.0, dtype=torch.float32, device="cuda")
        wide[:, :3] = x
        x = wide[:, :3]
        assert x.stride(0) == 4
    return p, x


@pytest.mark.parametrize("kw", [dict(solver="polar", precision="fast"), dict(solver="neohookean", precision="precise")])
def test_device_rows_equal_host_rows(kw):
    meshes = _three()
    host, dev, masked, side = (SoftBodyHIP.batch(meshes, dict(PP), **kw) for _ in range(4))
    held = [GRAB_ID, 11, 3]
    stream = torch.cuda.Stream()
    big = torch.randn(2048, 2048, device="cuda")
    keep = []
    for f in range(3):
        p, x = _table(meshes, held, f)
        host.setBodyGrabs(p, x)
        dev.setBodyGrabsDevice(*_dev(p, x))
        # the mask: body 1 keeps the row of frame 0
        if f == 0:
            masked.setBodyGrabsDevice(*_dev(p, x, padded=False))
        else:
            wrong = x.copy()
            wrong[1] += 1.0
            masked.setBodyGrabsDevice(*_dev([p[0], 2, p[2]], wrong), bodies=torch.tensor([True, False, True], device="cuda"))
        # rows that a kernel on a side stream fills, behind other work of that stream
        src_p, src_x = _dev(p, x, padded=False)
        torch.cuda.current_stream().synchronize()
        with torch.cuda.stream(stream):
            keep.append(big @ big)
            tp, tx = torch.empty_like(src_p), torch.empty_like(src_x)
            tp.copy_(src_p)
            tx.copy_(src_x * 1.0)
            side.setBodyGrabsDevice(tp, tx, stream=stream)
        for body in (host, dev, masked, side):
            body.simulateSubsteps(SUB, DT, PP)
    assert _same(_state(host), _state(dev))
    assert _same(_state(host), _state(side))
    # the masked handle: bodies 0 and 2 follow the frames, body 1 hangs from its first row
    want = SoftBodyHIP.batch(meshes, dict(PP), **kw)
    for f in range(3):
        p, x = _table(meshes, held, f)
        x[1] = _table(meshes, held, 0)[1][1]
        want.setBodyGrabs(p, x)
        want.simulateSubsteps(SUB, DT, PP)
    assert _same(_state(masked), _state(want))
    assert not _same(_state(masked), _state(host))
    stream.synchronize()


# ---- 5. rows the device refuses ---------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("kw", [dict(solver="polar", precision="fast"), dict(solver="neohookean", precision="fast")])
def test_a_row_the_device_refuses_means_not_held_and_disturbs_nobody(kw):
    meshes = _three()
    counts = [len(v) for v, _ in meshes]
    held = [GRAB_ID, 11, 3]
    p, x = _table(meshes, held, 0)
    nan = x.copy()
    nan[2, 1] = np.nan
    bad = [(0, [counts[0], p[1], p[2]], x), (1, [p[0], -7, p[2]], x), (2, list(p), nan)]
    for body, particles, targets in bad:
        got, want = (SoftBodyHIP.batch(meshes, dict(PP), **kw) for _ in range(2))
        got.setBodyGrabsDevice(*_dev(particles, targets))
        ok = p.copy()
        ok[body] = -1
        want.setBodyGrabs(ok, x)
        for b in (got, want):
            b.simulateSubsteps(SUB, DT, PP)
            b.simulateSubsteps(SUB, DT, PP)
        assert _same(_state(got), _state(want)), body
        got.close()
        want.close()


# ---- 6. OFF is free of effects ----------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("mesh,kw", ALL_PATHS)
def test_body_grabs_that_are_off_or_empty_change_nothing(mesh, kw):
    v, t = _mesh(mesh)
    never, empty, toggled = (SoftBodyHIP(v, t, None, dict(PP), **kw) for _ in range(3))
    x = _target(v, GRAB_ID, 0)
    empty.setBodyGrabs([-1], [x])
    toggled.setBodyGrabs([GRAB_ID], [x])
    toggled.setBodyGrabs(None, None)

    def frame(body):
        body.simulateSubsteps(SUB, DT, PP)
        for _ in range(3):
            body.simulate(DT, PP)
        body.simulateSubsteps(SUB, DT, PP)

    for body in (never, empty, toggled):
        frame(body)
    assert _same(_state(never), _state(empty)) and _same(_state(never), _state(toggled))
    for body in (never, toggled):   # ... and the handle's own grab works as ever afterwards
        body.setGrab(GRAB_ID, x)
        frame(body)
    assert _same(_state(never), _state(toggled))
    assert np.array_equal(never.pos[GRAB_ID], x)


# ---- 7. a new table between calls with unchanged parameters --------------------------------------------------------------------------------
@pytest.mark.parametrize("kw", [dict(solver="polar", precision="fast"), dict(solver="polar", precision="precise"), dict(solver="neohookean", precision="precise")])
def test_a_new_table_takes_effect_between_calls_with_the_same_params(kw):
    """tetsim_step skips the upload of unchanged parameters: a changed table alone must still reach the kernels"""
    v, t = _mesh("dragon")
    a, stale, twin = (SoftBodyHIP(v, t, None, dict(PP), **kw) for _ in range(3))
    x0, x1 = _target(v, GRAB_ID, 0), _target(v, GRAB_ID, 5)
    for body in (a, stale):
        body.setBodyGrabs([GRAB_ID], [x0])
    twin.setGrab(GRAB_ID, x0)
    for body in (a, stale, twin):
        body.simulate(DT, PP)
        body.simulate(DT, PP)
    a.setBodyGrabs([7], [x1])          # another particle, another place: same DevParams
    twin.setGrab(7, x1)
    for body in (a, stale, twin):
        body.simulate(DT, PP)
        body.simulate(DT, PP)
    assert _same(_state(a), _state(twin)) and not _same(_state(a), _state(stale))
    assert np.array_equal(a.pos[7], x1) and np.array_equal(stale.pos[GRAB_ID], x0)


# ---- 8. state -----------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("kw", [dict(solver="polar", precision="fast"), dict(solver="neohookean", precision="precise")])
def test_checkpoints_and_snapshots_do_not_hold_the_table(kw):
    meshes = [_dragon(0.3), _dragon(0.5)]
    held = [GRAB_ID, 11]
    a, b, c = (SoftBodyHIP.batch(meshes, dict(PP), **kw) for _ in range(3))
    blank = len(a.saveState())
    a.setBodyGrabs(*_table(meshes, held, 0))
    for _ in range(3):
        a.simulateSubsteps(SUB, DT, PP)
    blob = a.saveState()
    assert len(blob) == blank
    for _ in range(3):
        a.simulateSubsteps(SUB, DT, PP)
    b.loadState(blob)
    b.setBodyGrabs(*_table(meshes, held, 0))
    for _ in range(3):
        b.simulateSubsteps(SUB, DT, PP)
    assert _same(_state(a), _state(b))
    # a masked restore leaves the table alone: c sets it again behind the restore, a does not
    c.loadState(a.saveState())
    c.setBodyGrabs(*_table(meshes, held, 0))
    snap_a, snap_c = a.snapshot(), c.snapshot()
    for body, snap in ((a, snap_a), (c, snap_c)):
        body.simulateSubsteps(SUB, DT, PP)
        body.restore(snap, bodies=[True, False])
    c.setBodyGrabs(*_table(meshes, held, 0))
    for body in (a, c):
        body.simulateSubsteps(SUB, DT, PP)
    assert _same(_state(a), _state(c))
    assert np.array_equal(a.pos[GRAB_ID], _table(meshes, held, 0)[1][0])


# ---- 9. errors ------------------------------------------------------------------------------------------------------------------------------
def _hip_runtime():
    """The HIP runtime this process already has loaded (torch's)."""
    for line in open("/proc/self/maps"):
        if "libamdhip64" in line:
            return C.CDLL(line.split()[-1])
    raise RuntimeError("no libamdhip64 in this process")


def _code(fn, *args):
    with pytest.raises(TetSimError) as e:
        fn(*args)
    return e.value.code


def test_one_kind_of_grab_at_a_time():
    v, t = _mesh("dragon")
    x = _target(v, GRAB_ID, 0)
    a = SoftBodyHIP(v, t, None, dict(PP), solver="polar", precision="fast")
    a.setBodyGrabs([GRAB_ID], [x])
    assert _code(a.setGrab, GRAB_ID, x) == capi.ESTATE
    assert _code(a.startGrab, x) == capi.ESTATE
    assert _code(a.startGrabRay, [0.0, 5.0, 0.0], [0.0, -1.0, 0.0]) == capi.ESTATE
    a.endGrab()                         # releasing the handle's grab stays legal
    a.setBodyGrabs(None, None)
    a.setGrab(GRAB_ID, x)               # ... and with body grabs off the handle's grab is back
    assert _code(a.setBodyGrabs, [GRAB_ID], [x]) == capi.ESTATE
    p, tx = _dev([GRAB_ID], [x])
    assert _code(a.setBodyGrabsDevice, p, tx) == capi.ESTATE
    a.endGrab()
    a.setBodyGrabs([GRAB_ID], [x])
    texel = SoftBodyHIP(v, t, None, dict(PP), solver="polar", precision="precise", ref_grab_texel=True)
    assert _code(texel.setBodyGrabs, [GRAB_ID], [x]) == capi.ESTATE
    assert _code(texel.setBodyGrabsDevice, p, tx) == capi.ESTATE
    lv, lt = _mesh("lat12")
    owner = (np.arange(len(lv)) * 2 // len(lv)).astype(np.int32)
    part = SoftBodyHIP(lv, lt, None, dict(PP), solver="polar", precision="fast", part_count=2, part_index=0, vert_owner=owner)
    assert _code(part.setBodyGrabs, [GRAB_ID], [x]) == capi.ESTATE
    assert _code(part.setBodyGrabsDevice, p, tx) == capi.ESTATE
    pts = torch.zeros((1, 3), dtype=torch.float32, device="cuda")
    assert _code(part.nearestParticlesDevice, pts) == capi.ESTATE


def test_invalid_rows_and_pointers_are_refused_and_the_previous_table_stays():
    L = capi.lib()
    meshes = _three()
    kw = dict(solver="polar", precision="fast")
    a, b = (SoftBodyHIP.batch(meshes, dict(PP), **kw) for _ in range(2))
    held = [GRAB_ID, 11, 3]
    p, x = _table(meshes, held, 0)
    a.setBodyGrabs(p, x)
    b.setBodyGrabs(p, x)
    nan = x.copy()
    nan[1, 2] = np.nan
    inf = x.copy()
    inf[0, 0] = np.inf
    for particles, targets in (([len(meshes[0][0]), 11, 3], x), ([GRAB_ID, -2, 3], x), (p, nan), (p, inf)):
        assert _code(a.setBodyGrabs, particles, targets) == capi.EINVAL
    h = a._h
    dp, dx = _dev(p, x, padded=False)
    host_p, host_x = np.asarray(p, np.int32), np.ascontiguousarray(x, np.float32)
    hip = _hip_runtime()
    short = C.c_void_p()
    assert hip.hipMalloc(C.byref(short), C.c_size_t(3 * 12 - 4)) == 0   # an allocation of its own, one float too short for three rows
    cases = [((None, dx.data_ptr(), 0, None), None),   # particles == NULL is OFF, not an error: checked below
             ((dp.data_ptr(), None, 0, None), "null"),
             ((dp.data_ptr(), dx.data_ptr(), 8, None), "target_stride"), ((dp.data_ptr(), dx.data_ptr(), 14, None), "target_stride"),
             ((dp.data_ptr() + 2, dx.data_ptr(), 0, None), "aligned"), ((dp.data_ptr(), dx.data_ptr() + 1, 0, None), "aligned"),
             ((host_p.ctypes.data, dx.data_ptr(), 0, None), "not device memory"), ((dp.data_ptr(), host_x.ctypes.data, 0, None), "not device memory"),
             ((dp.data_ptr(), dx.data_ptr(), 0, host_p.ctypes.data), "not device memory"),
             ((dp.data_ptr(), short.value, 0, None), "do not fit"), ((short.value, dx.data_ptr(), 0, None), None),   # (32 bytes hold three indices)
             ((dp.data_ptr(), short.value, 16, None), "do not fit")]
    for args, text in cases[1:]:
        if text is None:
            continue
        rc = L.tetsim_set_body_grabs_device(h, *args, None)
        assert rc == capi.EINVAL, (args, rc, L.tetsim_last_error(h))
        assert text.encode() in L.tetsim_last_error(h), (args, L.tetsim_last_error(h))
    assert L.tetsim_set_body_grabs_device(None, dp.data_ptr(), dx.data_ptr(), 0, None, None) == capi.EINVAL
    assert L.tetsim_set_body_grabs(h, host_p.ctypes.data_as(C.POINTER(C.c_int32)), None) == capi.EINVAL
    pts, ids, d2 = dx, torch.empty(3, dtype=torch.int32, device="cuda"), torch.empty(3, dtype=torch.float64, device="cuda")
    for args, text in (((None, 0, ids.data_ptr(), None), "null"), ((pts.data_ptr(), 0, None, None), "null"), ((pts.data_ptr(), 8, ids.data_ptr(), None), "point_stride"),
                       ((host_x.ctypes.data, 0, ids.data_ptr(), None), "not device memory"), ((pts.data_ptr(), 0, host_p.ctypes.data, None), "not device memory"),
                       ((pts.data_ptr(), 0, ids.data_ptr(), d2.data_ptr() + 4), "aligned"), ((short.value, 0, ids.data_ptr(), None), "do not fit")):
        rc = L.tetsim_nearest_particles_device(h, *args, None)
        assert rc == capi.EINVAL and text.encode() in L.tetsim_last_error(h), (args, rc, L.tetsim_last_error(h))
    # a tensor the binding can see through
    with pytest.raises(ValueError):
        a.setBodyGrabsDevice(dp[:2], dx[:2])
    with pytest.raises(ValueError):
        a.setBodyGrabsDevice(dp.to(torch.int64), dx)
    # every refusal left the table in force: a still steps like b
    for body in (a, b):
        body.simulateSubsteps(SUB, DT, PP)
        body.simulateSubsteps(SUB, DT, PP)
    assert _same(_state(a), _state(b))
    assert np.array_equal(a.pos[GRAB_ID], x[0])
    torch.cuda.synchronize()
    assert hip.hipFree(short) == 0


# ---- 10. the nearest particle of every body ----------------------------------------------------------------------------------------------
def _points(meshes):
    """a point near each body, off its surface"""
    return np.stack([v.mean(0) + [0.07, 0.11, -0.05] for v, _ in meshes]).astype(np.float32)


@pytest.mark.parametrize("kw", [dict(solver="polar", precision="fast"), dict(solver="neohookean", precision="precise")])
def test_nearest_per_body_equals_the_solos_nearest_particle(kw):
    meshes = _three()
    batch = SoftBodyHIP.batch(meshes, dict(PP), **kw)
    solos = [SoftBodyHIP(v, t, None, dict(PP), **kw) for v, t in meshes]
    for body in [batch] + solos:
        body.simulateSubsteps(SUB, DT, PP)
        body.simulateSubsteps(SUB, DT, PP)
    pts = _points(meshes)
    dev_pts = torch.tensor(pts, device="cuda")
    ids, d2 = batch.nearestParticlesDevice(dev_pts)
    first = (ids.cpu().numpy().copy(), d2.cpu().numpy().copy())
    want = [solo.nearestParticle(q) for solo, q in zip(solos, pts)]
    assert first[0].tolist() == [w[0] for w in want]
    assert np.array_equal(first[1].view(np.uint64), np.asarray([w[1] for w in want], np.float64).view(np.uint64))
    # two calls give the same bits; caller-owned outputs and padded points give them too
    wide = torch.zeros((3, 4), dtype=torch.float32, device="cuda")
    wide[:, :3] = dev_pts
    oi, od = torch.full((3,), -5, dtype=torch.int32, device="cuda"), torch.zeros(3, dtype=torch.float64, device="cuda")
    batch.nearestParticlesDevice(wide[:, :3], out_ids=oi, out_dist2=od)
    assert np.array_equal(oi.cpu().numpy(), first[0]) and np.array_equal(od.cpu().numpy().view(np.uint64), first[1].view(np.uint64))


def test_nearest_ties_go_to_the_lowest_index_and_nan_particles_are_never_picked():
    n = 4
    v, t = make_lattice(n, y0=0.3)
    meshes = [(v, t), (v.copy(), t)]
    batch = SoftBodyHIP.batch(meshes, dict(PP), solver="polar", precision="fast")
    # the centre of a cell of the unstepped lattice: its 8 corners are equidistant in f64 when the spacing is a power of two apart ...
    xs = np.unique(v[:, 0]); ys = np.unique(v[:, 1]); zs = np.unique(v[:, 2])
    centre = np.array([(float(xs[1]) + float(xs[2])) / 2, (float(ys[1]) + float(ys[2])) / 2, (float(zs[1]) + float(zs[2])) / 2])
    q = centre.astype(np.float32)
    d = ((q.astype(np.float64) - v.astype(np.float64)) ** 2)
    d2 = d[:, 0] + d[:, 1] + d[:, 2]
    tied = np.nonzero(d2 == d2.min())[0]
    assert len(tied) == 8, tied      # ... which this lattice's coordinates are: the tie is real
    pts = torch.tensor(np.stack([q, q]), device="cuda")
    ids, dist = batch.nearestParticlesDevice(pts)
    assert ids.cpu().numpy().tolist() == [int(tied.min())] * 2
    assert dist.cpu().numpy().tolist() == [float(d2.min())] * 2
    # body 1's particle 0 becomes NaN; the query sits on top of where it was
    pos, vel = batch.pos, batch.vel
    pos[len(v)] = np.nan
    batch.writeState(pos, vel)
    at0 = torch.tensor(np.stack([v[0], v[0]]), device="cuda")
    ids, dist = batch.nearestParticlesDevice(at0)
    got = ids.cpu().numpy().tolist()
    assert got[0] == 0 and got[1] > 0 and dist.cpu().numpy()[0] == 0.0 and dist.cpu().numpy()[1] > 0.0
    solo = SoftBodyHIP(v, t, None, dict(PP), solver="polar", precision="fast")
    spos = solo.pos
    spos[0] = np.nan
    solo.writeState(spos, solo.vel)
    assert solo.nearestParticle(v[0]) == (got[1], float(dist.cpu().numpy()[1]))


@pytest.mark.parametrize("kw", [dict(solver="polar", precision="fast"), dict(solver="neohookean", precision="fast")])
def test_nearest_then_grab_on_the_device_equals_start_grab_on_each_solo(kw):
    meshes = _three()
    batch = SoftBodyHIP.batch(meshes, dict(PP), **kw)
    solos = [SoftBodyHIP(v, t, None, dict(PP), **kw) for v, t in meshes]
    for body in [batch] + solos:
        body.simulateSubsteps(SUB, DT, PP)
    pts = _points(meshes)
    dev_pts = torch.tensor(pts, device="cuda")
    ids, _ = batch.nearestParticlesDevice(dev_pts)
    batch.setBodyGrabsDevice(ids, dev_pts)          # no host in between
    picked = [solo.startGrab(q) for solo, q in zip(solos, pts)]
    for body in [batch] + solos:
        body.simulateSubsteps(SUB, DT, PP)
        body.simulateSubsteps(SUB, DT, PP)
    assert ids.cpu().numpy().tolist() == picked
    assert _same_bodies(batch, solos) == []
    for ((p0, _), _), i, q in zip(batch.bodyRanges, picked, pts):
        assert np.array_equal(batch.pos[p0 + i], q)
