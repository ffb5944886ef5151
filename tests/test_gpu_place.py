"""Placement (include/tetsim.h: tetsim_place_bodies / _device; SoftBodyHIP.placeBodies / placeBodiesDevice): one rigid motion per chosen
body, applied to the complete state.  The definition is tests/place_ref.py; the yardsticks are that file, the CPU oracle (a placed
trajectory is a valid trajectory of the same body), tetsim_write_state for the Neo-Hookean solver, and the library's guarantee that a body
in a batch equals its solo run bit for bit.  Kinds and meshes are those of test_gpu_snapshot.py.  Every test prints the
fused_particle_pass of its bodies.

FAST paths against the oracle (test 3): the allowance is tests/golden/place_tolerances.json -- per label the error observed on an MI355X
and min(3 x observed, cap), the cap being what tests/golden/tolerances.json gives the same path against the oracle at the nearest larger
substep count (the row names that label).  TETSIM_RECORD_ERRORS=<file> records instead of asserting, as conftest.within does."""
import ctypes as C
import json
import os

import numpy as np
import pytest
import torch

import place_ref
from conftest import GOLDEN, allowed_error
from oracle import OraclePJ
from tetsim_amd import SoftBodyHIP, TetSimError, place_rows
from tetsim_amd import _capi as capi
from test_gpu_body_grabs import _hip_runtime
from test_gpu_device_io import DT, PP, WIDE
from test_gpu_snapshot import BATCH, KINDS, POLAR_FAST, SHIFTS, batch, bits, cuda_mask, mesh, reads, same, show, solo, split, twins

pytestmark = pytest.mark.gpu
POLAR = [k for k in KINDS if k.startswith("polar")]
NH = [k for k in KINDS if k.startswith("nh")]


def seeded_row(seed, centre, offset=(0.3, 1.5, -0.2)):
    """An unnormalised quaternion, a pivot near `centre`, and a non-zero offset, linear and angular velocity."""
    rng = np.random.default_rng(seed)
    q = rng.standard_normal(4) * 1.7
    pivot = np.asarray(centre, np.float64) + rng.uniform(-0.1, 0.1, 3)
    return place_rows(q, pivot, offset, rng.uniform(-1.0, 1.0, 3), rng.uniform(-2.0, 2.0, 3))


def rows_tensor(rows):
    return torch.from_numpy(np.ascontiguousarray(rows, np.float32)).to("cuda")


def values(body):
    """What the host can read of the state, as floats."""
    if body.solver == "polar":
        return {"pos": body.pos, "vel": body.vel, "quats": body.quats}
    return {"pos": body.pos, "vel": body.vel, "prevPos": body.prevPos}


def placed(row, r, keep):
    """place_ref of values()."""
    pos, vel = place_ref.place_particles(row, r["pos"], r["vel"], keep)
    out = {"pos": pos, "vel": vel}
    if "quats" in r:
        out["quats"] = place_ref.place_quats(row, r["quats"])
    else:
        out["prevPos"] = place_ref.place_points(row, r["prevPos"])
    return out


def drag(v, *bodies, substeps=15):
    """Hold corner 0 where it is and move it 2 mm per substep, as a mouse drag does (test_gpu_polar.py: test_floor_grab_and_bounds): fifteen
    substeps of that deform the body and give it velocities.  `bodies`: SoftBodyHIP or oracle objects, stepped one substep at a time."""
    start = v[0].astype(np.float64)
    for s in range(substeps):
        p = [start[0] + 0.002 * (s + 1), start[1] + 0.001 * (s + 1), start[2] - 0.0015 * (s + 1)]
        for b in bodies:
            b.setGrab(0, p)
            b.simulate(DT, PP)


def release(*bodies):
    for b in bodies:
        b.setGrab(-1, [0.0, 0.0, 0.0])


# ---- 1. the placed state itself -------------------------------------------------------------------------------------------------------
STATE_CASES = [(k, "lat4") for k in KINDS] + [(k, "loose") for k in POLAR_FAST]


@pytest.mark.parametrize("keep", [False, True])
@pytest.mark.parametrize("kind,name", STATE_CASES)
def test_the_placed_state_is_place_ref_of_the_state_before(kind, name, keep):
    v, _ = mesh(name)
    body = solo(name, kind)
    show("%s %s" % (kind, name), body)
    if kind == "polar-fast" and name == "loose":
        assert body.info.fused_particle_pass == 5
    drag(v, body)
    before = values(body)                   # (a lean-state body: the quaternions recovered from its shape)
    row = seeded_row(11, v.mean(axis=0))
    body.placeBodiesDevice(rows_tensor(row), keep_velocity=keep)
    after, want = values(body), placed(row[0], before, keep)
    assert np.abs(after["pos"] - before["pos"]).max() > 0.5
    for n in want:
        assert np.array_equal(after[n], want[n], equal_nan=True), n
    body.close()


# ---- 2. / 3. against the oracle -------------------------------------------------------------------------------------------------------
_oracle = {}
ORACLE_KEEP = True


def oracle_run(name):
    """Per mesh, computed once: the oracle dragged for 15 substeps, released, placed by place_ref (positions, velocities, quaternions and the
    world-space corners of its textureElem), and stepped 25 more.  Poses stay inside the box the oracle hard-codes."""
    if name not in _oracle:
        v, t = mesh(name)
        orc = OraclePJ(v, t, PP, slot_quirk=True)
        drag(v, orc)
        orc.endGrab()
        row = seeded_row(23, v.mean(axis=0), offset=(0.3, 1.5, -0.2))
        idx_p, idx_t = np.arange(len(v)), np.arange(len(t))
        pos, vel = place_ref.place_particles(row[0], orc.pos, orc.vel, ORACLE_KEEP)
        q, el = orc.tetState(idx_t)
        el = el.copy()
        el[..., :3] = place_ref.place_shape_absolute(row[0], el[..., :3])
        orc.writeParticles(idx_p, pos, vel)
        orc.writeTets(idx_t, place_ref.place_quats(row[0], q), el)
        for _ in range(25):
            orc.simulate(DT, PP)
        inside = orc.pos[:-1] if name == "loose" else orc.pos   # (the particle no tet references is no evidence)
        lo, hi = inside.min(axis=0), inside.max(axis=0)
        assert lo[0] > -2.5 and hi[0] < 2.5 and lo[2] > -2.5 and hi[2] < 2.5 and lo[1] > -1.0 and hi[1] < 10.0
        _oracle[name] = (row, orc.pos, orc.vel, orc.quats)
    return _oracle[name]


def device_run(name, kind):
    v, _ = mesh(name)
    row = oracle_run(name)[0]
    body = solo(name, kind)
    show("%s %s" % (kind, name), body)
    drag(v, body)
    release(body)
    body.placeBodiesDevice(rows_tensor(row), keep_velocity=ORACLE_KEEP)
    body.simulateSubsteps(25, DT, PP)
    q = np.empty_like(body.quats)
    q[body.localTets] = body.quats
    return body, body.pos, body.vel, q


@pytest.mark.parametrize("name", ["lat4", "dragon"])
def test_precise_polar_continues_as_the_placed_oracle_does(name):
    """A shape or a prediction left unrotated shows at the first substep."""
    _, pos, vel, quats = oracle_run(name)
    body, p, u, q = device_run(name, "polar-precise")
    print("max |dx| %.3g, |dv| %.3g, |dq| %.3g" % (np.abs(p - pos).max(), np.abs(u - vel).max(), np.abs(q - quats).max()))
    assert np.array_equal(p, pos) and np.array_equal(u, vel) and np.array_equal(q, quats)
    body.close()


# (kind, mesh, the label of tests/golden/tolerances.json whose allowance caps this check)
FAST_CASES = [("polar-fast", "dragon", "polar fast blocked vs oracle dragon @200"),
              ("polar-fast-lean", "dragon", "polar fast lean vs oracle dragon @200"),
              ("polar-fast-constant-rest", "dragon", "polar fast constant-rest vs oracle dragon @200"),
              ("polar-fast", "loose", "polar fast one-launch call loose-particle delaunay vs oracle @60")]
_place_tol = None


def place_allowed(label, cap_label):
    global _place_tol
    if _place_tol is None:
        with open(os.path.join(GOLDEN, "place_tolerances.json")) as f:
            _place_tol = json.load(f)["checks"]
    row = _place_tol[label]
    cap = allowed_error(cap_label, np.inf)[0]
    assert row["cap_label"] == cap_label and np.isfinite(cap)
    assert row["allowed"] <= 3.0 * row["observed"] * (1 + 1e-9) and row["allowed"] <= cap, (label, row, cap)
    return row["allowed"]


@pytest.mark.parametrize("kind,name,cap_label", FAST_CASES)
def test_fast_paths_continue_next_to_the_placed_oracle(kind, name, cap_label):
    _, pos, _, _ = oracle_run(name)
    body, p, _, _ = device_run(name, kind)
    if name == "loose":
        assert body.info.fused_particle_pass == 5
        p, pos = p[:-1], pos[:-1]            # (the particle no tet references is no evidence: test_gpu_call_kernel_irregular.py)
    err = float(np.abs(p - pos).max())
    label = "placed %s %s vs oracle @15+25" % (kind, name)
    print("%s: max |dx| %.3g (cap: %s)" % (label, err, cap_label))
    rec = os.environ.get("TETSIM_RECORD_ERRORS")
    if rec:
        with open(rec, "a") as f:
            f.write(json.dumps({"label": label, "observed": err, "cap_label": cap_label}) + "\n")
    else:
        allowed = place_allowed(label, cap_label)
        assert err <= allowed, "%s: observed %.3g, allowed %.3g" % (label, err, allowed)
    body.close()


# ---- 4. Neo-Hookean: the twin that was told positions and velocities -------------------------------------------------------------------
@pytest.mark.parametrize("keep", [False, True])
@pytest.mark.parametrize("name", ["lat4", "dragon"])
@pytest.mark.parametrize("kind", NH)
def test_neohookean_equals_its_twin_through_write_state(kind, name, keep):
    v, _ = mesh(name)
    a, b = solo(name, kind), solo(name, kind)
    show("%s %s" % (kind, name), a, b)
    drag(v, a, b)
    release(a, b)
    row = seeded_row(31, v.mean(axis=0))
    a.placeBodiesDevice(rows_tensor(row), keep_velocity=keep)
    b.writeState(*place_ref.place_particles(row[0], b.pos, b.vel, keep))
    for body in (a, b):
        body.simulateSubsteps(20, DT, PP)
    assert same(reads(a), reads(b))
    assert np.abs(a.pos - v).max() > 0.5
    a.close()
    b.close()


# ---- 5. the batch contract --------------------------------------------------------------------------------------------------------------
def body_row(seed, b):
    v, _ = mesh(BATCH[b])
    return seeded_row(seed, v.mean(axis=0) + np.array([SHIFTS[b], 0.0, 0.0]), offset=(0.2, 0.8, -0.3))[0]


@pytest.mark.parametrize("kind", list(KINDS))
def test_a_placed_body_of_a_batch_equals_its_solo_twin_and_the_others_are_untouched(kind):
    rows = np.stack([body_row(41, 0), body_row(42, 1), body_row(43, 2)])
    never = twins(kind)[20]
    solos = {}
    for b in (0, 2):                         # the solo twins, placed through the host variant
        s = solo(BATCH[b], kind, SHIFTS[b])
        s.simulateSubsteps(10, DT, WIDE)
        s.placeBodies(rows[b:b + 1], keep_velocity=True)
        s.simulateSubsteps(10, DT, WIDE)
        solos[b] = reads(s)
        show("solo %s %s" % (kind, BATCH[b]), s)
        s.close()
    a = batch(kind)
    show("batch %s" % kind, a)
    a.simulateSubsteps(10, DT, WIDE)
    a.placeBodiesDevice(rows_tensor(rows), bodies=cuda_mask([1, 0, 1]), keep_velocity=True)   # (no sync() around it)
    a.simulateSubsteps(10, DT, WIDE)
    got = split(a, reads(a))
    assert same(got[0], solos[0]) and same(got[2], solos[2])
    assert same(got[1], never[1]) and not same(got[0], never[0]) and not same(got[2], never[2])
    a.close()
    # rows the host cannot see: a NaN, a zero quaternion -- their bodies continue untouched while the third is placed
    bad = rows.copy()
    bad[0, capi.PLACE_LINEAR + 1] = np.nan
    bad[1, capi.PLACE_Q:capi.PLACE_Q + 4] = 0.0
    c = batch(kind)
    c.simulateSubsteps(10, DT, WIDE)
    c.placeBodiesDevice(rows_tensor(bad), keep_velocity=True)
    c.simulateSubsteps(10, DT, WIDE)
    got = split(c, reads(c))
    assert same(got[0], never[0]) and same(got[1], never[1]) and same(got[2], solos[2])
    c.close()


# ---- 6. the exact permutation ----------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("kind", POLAR)
def test_the_half_quaternion_permutes_a_fresh_body_exactly(kind):
    """q = (0.5, 0.5, 0.5, 0.5) is the rotation by 120 degrees that takes (x, y, z) to (z, x, y), in exact arithmetic and in the definition's."""
    v, t = mesh("lat4")
    v = (v + np.array([1.0, 0.0, 0.0], np.float32)).astype(np.float32)   # (the permuted body stays above the floor)
    pp = dict(PP, gravity=0.0)
    body = SoftBodyHIP(v, t, None, dict(pp), **KINDS[kind])
    show(kind, body)
    body.placeBodies(place_rows([0.5, 0.5, 0.5, 0.5]))
    assert np.array_equal(body.pos, v[:, [2, 0, 1]]) and not body.vel.any()
    assert np.array_equal(body.quats, np.full((len(t), 4), 0.5, np.float32))
    body.simulateSubsteps(1, DT, pp)
    assert np.abs(body.quats - 0.5).max() < 1e-5      # (an unrotated shape gives the rotation by 120 degrees back: a quaternion near identity)
    assert np.abs(body.pos - v[:, [2, 0, 1]]).max() < 1e-5
    body.close()


# ---- 7. no synchronisation, and the stream contract ------------------------------------------------------------------------------------
@pytest.mark.parametrize("kind", ["polar-precise", "polar-fast", "polar-fast-lean", "nh-fast"])
def test_step_place_step_export_needs_one_synchronisation(kind):
    v, _ = mesh("dragon")
    row = rows_tensor(seeded_row(51, v.mean(axis=0), offset=(0.1, 0.5, 0.2)))
    names = ("pos", "vel", "quats") if kind.startswith("polar") else ("pos", "vel", "prevPos")
    out = []
    for synced in (False, True):
        body = solo("dragon", kind)
        show(kind, body)
        wait = body.sync if synced else (lambda: None)
        if synced:
            torch.cuda.synchronize()
        body.simulateSubsteps(8, DT, PP)
        wait()
        rows = row * 2.0                      # produced on torch's stream right in front of the call that reads it
        if synced:
            torch.cuda.synchronize()
        body.placeBodiesDevice(rows, keep_velocity=True)
        rows.fill_(float("nan"))              # ... and reused right behind it
        wait()
        body.simulateSubsteps(8, DT, PP)
        wait()
        got = body.exportTensors(names)
        torch.cuda.synchronize()
        out.append({n: bits(got[n].cpu().numpy()) for n in names})
        assert np.isfinite(got["pos"].cpu().numpy()).all()
        body.close()
    assert same(out[0], out[1])


# ---- 8. refusals ------------------------------------------------------------------------------------------------------------------------
def test_every_refusal_names_its_code_and_leaves_the_state_alone():
    a = batch("polar-fast")
    show("batch polar-fast", a)
    a.simulateSubsteps(5, DT, WIDE)
    L, h = a._L, a._h
    rows = np.stack([body_row(61, b) for b in range(3)])
    dr, dm = rows_tensor(rows), cuda_mask([1, 1, 1])
    host_rows, host_mask = np.ascontiguousarray(rows), np.ones(3, np.uint8)
    hip = _hip_runtime()
    short, short_mask = C.c_void_p(), C.c_void_p()
    assert hip.hipMalloc(C.byref(short), C.c_size_t(3 * 64 - 4)) == 0      # an allocation of its own, one float too short for three rows
    assert hip.hipMalloc(C.byref(short_mask), C.c_size_t(2)) == 0          # ... and a mask of two bytes for three bodies
    state = a.saveState()
    cases = [((None, 0, None, 0), capi.EINVAL, "null"),
             ((dr.data_ptr(), 60, None, 0), capi.EINVAL, "row_stride"), ((dr.data_ptr(), 66, None, 0), capi.EINVAL, "row_stride"),
             ((dr.data_ptr() + 2, 0, None, 0), capi.EINVAL, "aligned"),
             ((host_rows.ctypes.data, 0, None, 0), capi.EINVAL, "not device memory"),
             ((short.value, 0, None, 0), capi.EINVAL, "do not fit"), ((short.value, 96, None, 0), capi.EINVAL, "do not fit"),
             ((dr.data_ptr(), 0, None, 2), capi.EINVAL, "flag"), ((dr.data_ptr(), 0, None, 0x80000001), capi.EINVAL, "flag"),
             ((dr.data_ptr(), 0, host_mask.ctypes.data, 0), capi.EINVAL, "not device memory"),
             ((dr.data_ptr(), 0, short_mask.value, 0), capi.EINVAL, "do not fit")]
    for args, code, text in cases:
        rc = L.tetsim_place_bodies_device(h, *args, None)
        assert rc == code and text.encode() in L.tetsim_last_error(h), (args, rc, L.tetsim_last_error(h))
        assert a.saveState() == state, args
    assert L.tetsim_place_bodies_device(None, dr.data_ptr(), 0, None, 0, None) == capi.EINVAL
    # the host variant: rows it can see
    for k, value in ((capi.PLACE_PIVOT, np.nan), (capi.PLACE_ANGULAR + 2, np.inf), (capi.PLACE_Q, None)):
        bad = rows.copy()
        if value is None:
            bad[1, capi.PLACE_Q:capi.PLACE_Q + 4] = 0.0
        else:
            bad[1, k] = value
        with pytest.raises(TetSimError) as e:
            a.placeBodies(bad)
        assert e.value.code == capi.EINVAL and a.saveState() == state
    assert L.tetsim_place_bodies(h, host_rows.ctypes.data_as(C.POINTER(C.c_float)), None, 4) == capi.EINVAL and a.saveState() == state
    # what the binding can see through: a mask of the wrong size, rows of the wrong shape
    with pytest.raises(ValueError):
        a.placeBodiesDevice(dr, bodies=cuda_mask([1, 1]))
    with pytest.raises(ValueError):
        a.placeBodiesDevice(dr[:2])
    with pytest.raises(ValueError):
        a.placeBodies(rows, bodies=[1, 0])
    assert a.saveState() == state
    # ... and the call itself still works on this handle: a masked-out body of the bad row is no error for the host variant
    bad = rows.copy()
    bad[1, 0] = np.nan
    a.placeBodies(bad, bodies=[1, 0, 1])
    assert a.saveState() != state
    for p in (short, short_mask):
        hip.hipFree(p)
    a.close()
