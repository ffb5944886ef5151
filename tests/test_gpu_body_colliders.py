"""Body colliders (include/tetsim.h: tetsim_set_body_colliders / _device).

The oracle needs no tolerance: body b of a batch with rows r0 .. rk must give the bits that body b alone gives with setColliders of the
same rows widened to double -- on every stepping path, for both solvers and both precisions, tetsim_step and tetsim_step_n.  Equality is
on the bits of pos, vel and, for polar, quats, with the helpers of test_gpu_body_grabs.py; meshes, PP, DT and path labels are
test_gpu_colliders.py's; a frame is one call of 20 substeps."""
import ctypes as C

import numpy as np
import pytest
import torch

import body_collider_ref as ref
import crowd
from test_gpu_body_grabs import BATCH_CASES, LARGE_CASES, _code, _hip_runtime, _path, _same, _same_bodies, _state, _target, _three
from test_gpu_colliders import DT, GRAB_ID, PP, SUB, _mesh
from test_gpu_crowd import Sampled
from tetsim_amd import SoftBodyHIP, TetSimError, body_collider_rows, make_lattice
from tetsim_amd import _capi as capi

pytestmark = pytest.mark.gpu



def _scene(v, frame=0, lift=0.06):
    """f32_scene lifted into the body's lowest centimetres, so that a body in free fall meets it within the first frame"""
    return ref.f32_scene(v + np.float32([0.0, lift, 0.0]), frame)


def _lists(meshes, frame):
    """body 0: the four-collider scene with the moving sphere; body 1: a box and a tilted plane; body 2: nothing"""
    two = _scene(meshes[1][0], 0, 0.2)
    return [_scene(meshes[0][0], frame), [two[2], two[3]], []]


def _rows(meshes, frame):
    """... as rows of per_body = 4: body 1's two colliders sit in slots 0 and 3, empty slots between them"""
    lists = _lists(meshes, frame)
    rows = ref.rows(lists, 4)
    rows[1, 3], rows[1, 1] = rows[1, 1].copy(), ref.rows([[]], 1)[0, 0]
    return rows, lists


def _step(batch, solos, meshes, frames, set_rows=None):
    for f in range(frames):
        rows, lists = _rows(meshes, f)
        (set_rows or batch.setBodyColliders)(rows)
        batch.simulateSubsteps(SUB, DT, PP)
        for solo, cs in zip(solos, lists):
            solo.setColliders(cs)
            solo.simulateSubsteps(SUB, DT, PP)


# ---- 1. batch = solos, every path ---------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("case", list(BATCH_CASES))
def test_each_body_of_a_batch_equals_its_solo_run_with_set_colliders(case):
    kw, solo_path, batch_path = BATCH_CASES[case]
    meshes = _three()
    batch, free = (SoftBodyHIP.batch(meshes, dict(PP), **kw) for _ in range(2))
    solos = [SoftBodyHIP(v, t, None, dict(PP), **kw) for v, t in meshes]
    _path(batch, batch_path)
    _path(solos[0], solo_path)
    _step(batch, solos, meshes, 6)
    for _ in range(6):
        free.simulateSubsteps(SUB, DT, PP)
    assert _same_bodies(batch, solos) == []
    assert _same_bodies(free, solos) == [0, 1]   # the colliders were met; the body without rows steps as ever


# ---- 2. the large paths on a single body ----------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("case", list(LARGE_CASES))
def test_a_single_body_with_its_rows_equals_its_twin_with_set_colliders(case):
    mesh, kw, path = LARGE_CASES[case]
    v, t = _mesh(mesh)
    a, b, none = (SoftBodyHIP(v, t, None, dict(PP), **kw) for _ in range(3))
    _path(a, path)
    for f in range(3):
        cs = _scene(v, f)
        a.setBodyColliders(ref.rows([cs], 8))
        b.setColliders(cs)
        for body in (a, b, none):
            body.simulateSubsteps(SUB, DT, PP)
    assert _same(_state(a), _state(b)) and not _same(_state(a), _state(none))


# ---- 3. one call of n = n calls -------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("kw,path", [(dict(solver="polar", precision="fast"), 3), (dict(solver="polar", precision="fast", lean_state=True), 2),
                                     (dict(solver="neohookean", precision="fast"), 4)])
def test_one_call_of_n_substeps_equals_n_calls(kw, path):
    v, t = _mesh("dragon")
    a, b = (SoftBodyHIP(v, t, None, dict(PP), **kw) for _ in range(2))
    _path(a, path)
    for f in range(4):
        rows = ref.rows([_scene(v, f)], 4)
        a.setBodyColliders(rows)
        b.setBodyColliders(rows)
        a.simulateSubsteps(SUB, DT, PP)
        for _ in range(SUB):
            b.simulate(DT, PP)
    assert _same(_state(a), _state(b))


# ---- 3b. switching ON and OFF in mid-run: the bodies whose one-launch calls leave the table to their stepwise kernels ------------------------
@pytest.mark.parametrize("mesh,kw,path", [("dragon", dict(solver="polar", precision="fast"), 3), ("dragon", dict(solver="neohookean", precision="fast"), 4),
                                          ("dragon", dict(solver="neohookean", precision="precise"), 4),
                                          ("lat30", dict(solver="neohookean", precision="fast", order="clustered"), 0)])
def test_switching_on_and_off_between_calls_equals_the_twin(mesh, kw, path):
    """step, ON, step, OFF, step, ON again: the persistent / one-launch kernels and the stepwise ones hand the state to each other"""
    v, t = _mesh(mesh)
    a, b = (SoftBodyHIP(v, t, None, dict(PP), **kw) for _ in range(2))
    _path(a, path)
    cs = _scene(v)
    rows = ref.rows([cs], 4)
    for f, on in enumerate([False, True, True, False, True, False]):
        a.setBodyColliders(rows if on else None)
        b.setColliders(cs if on else [])
        for body in (a, b):
            body.simulateSubsteps(SUB, DT, PP)
            if f % 2:
                body.simulate(DT, PP)
    assert _same(_state(a), _state(b))


def test_a_stride_of_100_bytes_is_served():
    v, t = _mesh("dragon")
    a, b = (SoftBodyHIP(v, t, None, dict(PP), solver="polar", precision="fast") for _ in range(2))
    cs = _scene(v)
    wide = torch.full((1, 4, 25), float("nan"), dtype=torch.float32, device="cuda")
    wide[:, :, :24] = torch.tensor(ref.rows([cs], 4), device="cuda")
    assert wide.stride(1) * 4 == 100
    a.setBodyCollidersDevice(wide[:, :, :24])
    b.setColliders(cs)
    for body in (a, b):
        body.simulateSubsteps(SUB, DT, PP)
    assert _same(_state(a), _state(b))


# ---- 4. device variant = host variant ---------------------------------------------------------------------------------------------------------
def _wide(rows, width=32):
    """the rows as the [..., :24] view of a wider tensor whose other floats are NaN"""
    w = torch.full(rows.shape[:2] + (width,), float("nan"), dtype=torch.float32, device="cuda")
    w[:, :, :24] = torch.tensor(rows, device="cuda")
    return w[:, :, :24]


@pytest.mark.parametrize("kw", [dict(solver="polar", precision="fast"), dict(solver="neohookean", precision="precise")])
def test_device_rows_equal_host_rows(kw):
    meshes = _three()
    host, dev, masked, want = (SoftBodyHIP.batch(meshes, dict(PP), **kw) for _ in range(4))
    stream = torch.cuda.Stream()
    big = torch.randn(2048, 2048, device="cuda")
    keep = []
    for f in range(3):
        rows, _ = _rows(meshes, f)
        host.setBodyColliders(rows)
        src = _wide(rows)
        assert src.stride(1) == 32 and src.stride(0) == 4 * 32
        torch.cuda.current_stream().synchronize()
        with torch.cuda.stream(stream):   # rows that a kernel on a side stream fills, behind other work of that stream
            keep.append(big @ big)
            t = torch.full((3, 4, 32), float("nan"), device="cuda")
            t[:, :, :24].copy_(src * 1.0)
            dev.setBodyCollidersDevice(t[:, :, :24], stream=stream)
        # the mask: body 1 keeps the rows of frame 0
        stale = rows.copy()
        stale[1] = _rows(meshes, 0)[0][1]
        want.setBodyColliders(stale)
        if f == 0:
            masked.setBodyCollidersDevice(_wide(rows))
        else:
            wrong = rows.copy()
            wrong[1, :, 2] += 1.0
            masked.setBodyCollidersDevice(_wide(wrong), bodies=torch.tensor([True, False, True], device="cuda"))
        for body in (host, dev, masked, want):
            body.simulateSubsteps(SUB, DT, PP)
    assert _same(_state(host), _state(dev))
    assert _same(_state(masked), _state(want))
    stream.synchronize()


def test_the_device_call_does_not_wait_for_the_host():
    """behind a long kernel on the caller's stream the call returns while that kernel still runs"""
    meshes = _three()
    a = SoftBodyHIP.batch(meshes, dict(PP), solver="polar", precision="fast")
    rows = torch.tensor(_rows(meshes, 0)[0], device="cuda")
    a.setBodyCollidersDevice(rows)   # (the first call allocates and may block)
    big = torch.randn(4096, 4096, device="cuda")
    torch.cuda.synchronize()
    done = torch.cuda.Event()
    for _ in range(20):
        big = big @ big * 1e-4
    done.record()
    a.setBodyCollidersDevice(rows)
    assert not done.query()
    torch.cuda.synchronize()


# ---- 5. the crowd -------------------------------------------------------------------------------------------------------------------------
def _crowd_lists(cr, seed):
    out = []
    for b, (v, _) in enumerate(cr.bodies):
        rng = np.random.default_rng([seed, b])
        lo, hi = v.min(0).astype(np.float64), v.max(0).astype(np.float64)
        c = (lo + hi) / 2
        plane = dict(kind="plane", a=[c[0], lo[1] - 0.002, c[2]], b=[rng.uniform(-0.2, 0.2), 1.0, rng.uniform(-0.2, 0.2)], friction=rng.uniform(1.0, 50.0))
        ball = dict(kind="sphere", a=[c[0], lo[1] - 0.05, c[2]], radius=0.06 + rng.uniform(0.0, 0.01), friction=20.0, velocity=[0.1, 0.0, 0.0])
        box = dict(kind="box", a=[c[0], lo[1] - 0.1, c[2]], b=[1.0, 0.099, 1.0], friction=100.0)
        out.append([[], [plane], [ball, box]][b % 3])
    return out


@pytest.mark.parametrize("kw", [dict(solver="polar", precision="fast"), dict(solver="neohookean", precision="fast")])
def test_the_crowd_equals_its_solos(kw):
    cr = crowd.build()
    pos, vel = cr.state(3)
    batch = SoftBodyHIP.batch(cr.bodies, dict(crowd.PP), **kw)
    batch.writeState(pos, vel)
    solos = []
    for b in crowd.SAMPLE:
        s = SoftBodyHIP(*cr.bodies[b], None, dict(crowd.PP), **kw)
        s.writeState(cr.body(b, pos), cr.body(b, vel))
        solos.append(s)
    first = ref.lists_from_rows(ref.rows(_crowd_lists(cr, 1), 2))
    second = ref.lists_from_rows(ref.rows(_crowd_lists(cr, 2), 2))
    chosen = cr.mask(5)
    assert chosen[list(crowd.SAMPLE)].any() and not chosen[list(crowd.SAMPLE)].all()
    batch.setBodyColliders(ref.rows(first, 2))
    for frame in range(2):
        if frame == 1:   # a second set call, from the device, for the chosen bodies only: the others keep their lists
            batch.setBodyCollidersDevice(torch.tensor(ref.rows(second, 2), device="cuda"), bodies=torch.tensor(chosen, device="cuda"))
        batch.simulateSubsteps(SUB, DT, crowd.PP)
        for s, b in zip(solos, crowd.SAMPLE):
            s.setColliders(second[b] if frame == 1 and chosen[b] else first[b])
            s.simulateSubsteps(SUB, DT, crowd.PP)
    assert _same_bodies(Sampled(batch), solos) == []


# ---- 6. rows the host cannot see ----------------------------------------------------------------------------------------------------------
def _bad_rows(meshes):
    """body 0's scene in per_body = 8 with seeded bad rows between the good ones"""
    good = ref.rows([_scene(meshes[0][0], 0)], 4)[0]
    rows = ref.rows([[], _scene(meshes[1][0], 0, 0.2)[2:], []], 8)
    bad = [good[0].copy() for _ in range(5)]
    bad[0][9] = np.nan                                  # a NaN in a field a sphere does not use
    bad[1][0] = 1.5                                     # no such kind
    bad[2][16] = -0.1                                   # negative radius
    bad[3] = good[3].copy(); bad[3][4:7] = 0.0          # a plane with a zero normal
    bad[4] = good[2].copy(); bad[4][10] = 0.01          # a box with skewed axes
    rows[0] = np.stack([bad[0], good[0], bad[1], good[1], bad[2], good[2], bad[3], good[3]])
    rows[2, 0] = bad[4]
    return rows, bad


def test_rows_the_device_refuses_are_empty_slots_and_disturb_nobody():
    meshes = _three()
    kw = dict(solver="polar", precision="fast")
    rows, bad = _bad_rows(meshes)
    assert [ref.row_ok(r) for r in rows[0]] == [False, True] * 4 and not any(ref.row_ok(r) for r in bad)
    lists = ref.lists_from_rows(rows)
    assert [len(c) for c in lists] == [4, 2, 0]
    batch = SoftBodyHIP.batch(meshes, dict(PP), **kw)
    solos = [SoftBodyHIP(v, t, None, dict(PP), **kw) for v, t in meshes]
    for r in bad:   # the solo's setColliders refuses exactly what row_ok refuses
        one = ref.rows([[]], 1)
        one[0, 0] = r
        with np.errstate(invalid="ignore"):
            d = r.astype(np.float64)
        cs = [dict(kind=int(d[0]) if d[0] == int(d[0]) else 7, a=d[1:4].tolist(), b=d[4:7].tolist(), axes=d[7:16].reshape(3, 3).tolist(), radius=float(d[16]),
                   friction=float(d[17]), velocity=d[18:21].tolist())]
        assert _code(solos[0].setColliders, cs) == capi.EINVAL
    batch.setBodyCollidersDevice(torch.tensor(rows, device="cuda"))
    for solo, cs in zip(solos, lists):
        solo.setColliders(cs)
    for body in [batch] + solos:
        for _ in range(3):
            body.simulateSubsteps(SUB, DT, PP)
    assert _same_bodies(batch, solos) == []
    # the host variant refuses each of them, names body and slot, and the table stays in force
    for k, r in enumerate(bad):
        wrong = rows.copy()
        wrong[:] = ref.rows(lists, 8)
        wrong[1, 5] = r
        with pytest.raises(TetSimError) as e:
            batch.setBodyColliders(wrong)
        assert e.value.code == capi.EINVAL and "body 1, slot 5" in str(e.value), (k, str(e.value))
    for body in [batch] + solos:
        body.simulateSubsteps(SUB, DT, PP)
    assert _same_bodies(batch, solos) == []


# ---- 7. with body grabs -------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("kw", [dict(solver="polar", precision="fast"), dict(solver="polar", precision="precise"), dict(solver="neohookean", precision="fast"),
                                dict(solver="neohookean", precision="precise")])
def test_a_held_body_with_colliders_equals_its_solo(kw):
    meshes = _three()
    batch = SoftBodyHIP.batch(meshes, dict(PP), **kw)
    solos = [SoftBodyHIP(v, t, None, dict(PP), **kw) for v, t in meshes]
    held = [GRAB_ID, 11, -1]
    for f in range(4):
        x = np.stack([_target(v, max(p, 0), f) for (v, _), p in zip(meshes, held)])
        rows, lists = _rows(meshes, f)
        batch.setBodyGrabs(held, x)
        batch.setBodyColliders(rows)
        batch.simulateSubsteps(SUB, DT, PP)
        for solo, p, xi, cs in zip(solos, held, x, lists):
            if p >= 0:
                solo.setGrab(p, xi)
            solo.setColliders(cs)
            solo.simulateSubsteps(SUB, DT, PP)
    assert _same_bodies(batch, solos) == []
    assert np.array_equal(batch.pos[GRAB_ID], _target(meshes[0][0], GRAB_ID, 3))   # the held particle is where it is held, not pushed


# ---- 8. states and errors -----------------------------------------------------------------------------------------------------------------
def test_states_and_errors():
    L = capi.lib()
    v, t = _mesh("dragon")
    kw = dict(solver="polar", precision="fast")
    a, twin = (SoftBodyHIP(v, t, None, dict(PP), **kw) for _ in range(2))
    cs = ref.f32_scene(v)
    rows = ref.rows([cs], 4)
    size = C.c_uint64()
    assert L.tetsim_state_size(a._h, C.byref(size)) == 0
    blank = size.value
    a.setColliders(cs[:1])
    assert _code(a.setBodyColliders, rows) == capi.ESTATE                       # ON while the handle's list is set
    assert _code(a.setBodyCollidersDevice, torch.tensor(rows, device="cuda")) == capi.ESTATE
    a.setColliders([])
    a.setBodyColliders(rows)
    assert _code(a.setColliders, cs[:1]) == capi.ESTATE                         # the handle's list while ON
    a.setColliders([])                                                          # ... clearing it stays legal
    lv, lt = _mesh("lat12")
    owner = (np.arange(len(lv)) * 2 // len(lv)).astype(np.int32)
    part = SoftBodyHIP(lv, lt, None, dict(PP), solver="polar", precision="fast", part_count=2, part_index=0, vert_owner=owner)
    assert _code(part.setBodyColliders, rows) == capi.ESTATE
    assert _code(part.setBodyCollidersDevice, torch.tensor(rows, device="cuda")) == capi.ESTATE
    fp = rows.ctypes.data_as(C.POINTER(C.c_float))
    dev = torch.tensor(rows, device="cuda")
    for per_body in (0, 9):
        assert L.tetsim_set_body_colliders(a._h, fp, per_body) == capi.EINVAL
        assert L.tetsim_set_body_colliders_device(a._h, dev.data_ptr(), 0, per_body, None, None) == capi.EINVAL
    # (100 is a multiple of 4 of at least 96: by the header's rule a LEGAL stride -- test_a_stride_of_100_bytes_is_served; refused are:)
    for stride in (98, 92, 48):   # not a multiple of 4; below 96
        assert L.tetsim_set_body_colliders_device(a._h, dev.data_ptr(), stride, 4, None, None) == capi.EINVAL and b"row_stride" in L.tetsim_last_error(a._h)
    assert L.tetsim_set_body_colliders_device(a._h, rows.ctypes.data, 0, 4, None, None) == capi.EINVAL and b"not device memory" in L.tetsim_last_error(a._h)
    hip = _hip_runtime()
    short = C.c_void_p()
    assert hip.hipMalloc(C.byref(short), C.c_size_t(4 * 96 - 96)) == 0   # an allocation of its own, one row short
    assert L.tetsim_set_body_colliders_device(a._h, short.value, 0, 4, None, None) == capi.EINVAL and b"do not fit" in L.tetsim_last_error(a._h)
    with pytest.raises(ValueError):
        a.setBodyCollidersDevice(dev[:, :, :20])
    # the table is not solver state
    for _ in range(2):
        a.simulateSubsteps(SUB, DT, PP)
    assert L.tetsim_state_size(a._h, C.byref(size)) == 0 and size.value == blank
    blob = a.saveState()
    assert len(blob) == blank
    snap = a.snapshot()
    free = SoftBodyHIP(v, t, None, dict(PP), **kw)
    assert len(a.saveState()) == len(free.saveState())
    del snap
    # OFF, then stepping, equals a twin that loaded the same state and steps with no colliders
    a.setBodyColliders(None)
    twin.loadState(blob)
    for body in (a, twin):
        body.simulateSubsteps(SUB, DT, PP)
        body.simulate(DT, PP)
    assert _same(_state(a), _state(twin))
    torch.cuda.synchronize()
    assert hip.hipFree(short) == 0


# ---- 9. the seven refusals, from both set calls ------------------------------------------------------------------------------------------------
# (what is wrong with the collider, tetsim_set_colliders' text, tetsim_set_body_colliders' text) in the order the library checks
_REFUSALS = [
    (dict(kind=7), "unknown kind", "unknown kind (0, 1, 2, 3, or -1 for an empty slot)"),
    (dict(kind="sphere", axes=[[1.0, 0.0, 0.0], [0.0, float("inf"), 0.0], [0.0, 0.0, 1.0]]), "non-finite value", "non-finite value"),
    (dict(kind="capsule", radius=-0.1), "negative radius or friction", "negative radius or friction"),
    (dict(kind="plane", b=[0.0, 0.0, 0.0]), "zero-length plane normal", "zero-length plane normal"),
    (dict(kind="box", b=[0.1, -0.1, 0.1]), "negative half-extent", "negative half-extent"),
    (dict(kind="box", b=[0.1, 0.1, 0.1], axes=[[1.0, 0.0, 0.0], [0.0, 1.0, 0.0], [0.0, 0.0, 0.0]]), "zero-length box axis", "zero-length box axis"),
    (dict(kind="box", b=[0.1, 0.1, 0.1], axes=[[1.0, 0.0, 0.0], [0.01, 1.0, 0.0], [0.0, 0.0, 1.0]]), "box axes are not orthogonal", "box axes are not orthogonal"),
]


def test_both_set_calls_refuse_the_seven_reasons_in_their_own_words_and_keep_what_was_set():
    """For each of the seven reasons a collider is refused, setColliders on a solo handle and setBodyColliders on a batch raise EINVAL with
    the text commit 50eac02 gives -- recorded there, not derived from the routine the two calls now share -- and the list / the table set
    before stays in force: after every refusal one substep equals, on bits, the twin's that never saw the refused call."""
    v, t = make_lattice(5, y0=0.3)
    kw = dict(solver="polar", precision="fast")
    lo = float(v[:, 1].min())
    good = ref.lists_from_rows(ref.rows([[dict(kind="plane", a=[0.0, lo + 0.02, 0.0], b=[0.1, 1.0, 0.05], friction=5.0)]]))[0]   # cuts the body's lowest layer: met at once
    solo, solo_twin, free = (SoftBodyHIP(v, t, None, dict(PP), **kw) for _ in range(3))
    batch, batch_twin = (SoftBodyHIP.batch([(v, t)] * 2, dict(PP), **kw) for _ in range(2))
    rows = ref.rows([good, good], 2)
    for body in (solo, solo_twin):
        body.setColliders(good)
    for body in (batch, batch_twin):
        body.setBodyColliders(rows)
    for k, (bad, solo_text, row_text) in enumerate(_REFUSALS):
        assert ref.refusal(ref.row(bad)) == k + 1
        with pytest.raises(TetSimError) as e:
            solo.setColliders(good + [bad])
        assert e.value.code == capi.EINVAL and str(e.value) == "tetsim error 1: collider 1: " + solo_text
        wrong = rows.copy()
        wrong[1, 1] = ref.row(bad)
        with pytest.raises(TetSimError) as e:
            batch.setBodyColliders(wrong)
        assert e.value.code == capi.EINVAL and str(e.value) == "tetsim error 1: body 1, slot 1: " + row_text
        for body in (solo, solo_twin, batch, batch_twin, free):
            body.simulate(DT, PP)
        assert _same(_state(solo), _state(solo_twin)) and _same(_state(batch), _state(batch_twin)), k
    assert _same_bodies(batch, [solo, solo]) == [] and not _same(_state(solo), _state(free))   # ... and the list was met
