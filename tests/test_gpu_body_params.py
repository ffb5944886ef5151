"""Body parameters (include/tetsim.h: tetsim_set_body_params / _device).

The oracle needs no tolerance: body b of a batch with row r must give the bits that body b alone gives stepped with TetSimParams r -- on
every stepping path, for both solvers and both precisions, tetsim_step and tetsim_step_n.  Equality is on the bits of pos, vel and, for
polar, quats, with the helpers of test_gpu_body_grabs.py; meshes, PP, DT and path labels are test_gpu_colliders.py's; a frame is one call
of SUB substeps."""
import ctypes as C

import numpy as np
import pytest
import torch

import body_collider_ref as cref
import crowd
from test_gpu_body_grabs import BATCH_CASES, LARGE_CASES, _code, _hip_runtime, _path, _same, _same_bodies, _state, _target, _three
from test_gpu_colliders import DT, GRAB_ID, PP, SUB, _mesh
from test_gpu_crowd import Sampled
from tetsim_amd import SoftBodyHIP, TetSimError, body_param_rows, make_lattice
from tetsim_amd import _capi as capi

pytestmark = pytest.mark.gpu

CASES = dict(BATCH_CASES)
CASES["polar-fast-own-bounds"] = (dict(solver="polar", precision="fast", ref_fixed_bounds=False), 3, 3)
CASES["polar-precise-own-bounds"] = (dict(solver="polar", precision="precise", ref_fixed_bounds=False), 0, 0)


def _dicts(meshes):
    """body 0: PP itself; body 1: weak gravity, no friction, softer, a floor 2 cm under it; body 2: gravity upwards, a ceiling 2 cm above
    it and side walls 1 cm inside its box"""
    v1, v2 = meshes[1][0].astype(np.float64), meshes[2][0].astype(np.float64)
    one = dict(PP, gravity=-3.0, friction=0.0, devCompliance=1e-4, volCompliance=1e-6)
    one["worldBounds"] = [-2.5, v1[:, 1].min() - 0.02, -2.5, 2.5, 10.0, 2.5]
    lo, hi = v2.min(0), v2.max(0)
    two = dict(PP, gravity=2.0, friction=50.0)
    two["worldBounds"] = [lo[0] + 0.01, -1.0, lo[2] + 0.01, hi[0] - 0.01, hi[1] + 0.02, hi[2] - 0.01]
    return [dict(PP), one, two]


def _fixed(kw):
    return kw["solver"] == "polar" and kw.get("ref_fixed_bounds", True)


# ---- 1. batch = solos, every path ---------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("case", list(CASES))
def test_each_body_of_a_batch_equals_its_solo_run_with_its_own_params(case):
    kw, solo_path, batch_path = CASES[case]
    meshes = _three()
    dicts = _dicts(meshes)
    batch, shared = (SoftBodyHIP.batch(meshes, dict(PP), **kw) for _ in range(2))
    solos = [SoftBodyHIP(v, t, None, dict(PP), **kw) for v, t in meshes]
    _path(batch, batch_path)
    _path(solos[0], solo_path)
    batch.setBodyParams(dicts)
    for _ in range(6):
        batch.simulateSubsteps(SUB, DT, PP)
        shared.simulateSubsteps(SUB, DT, PP)
        for solo, d in zip(solos, dicts):
            solo.simulateSubsteps(SUB, DT, d)
    assert _same_bodies(batch, solos) == []
    assert _same_bodies(shared, solos) == [1, 2]   # the rows made a difference; the body whose row is PP steps as ever
    if _fixed(kw):   # the reference's constant box for every body: body 1's bounds made no difference
        plain = SoftBodyHIP(*meshes[1], None, dict(PP), **kw)
        for _ in range(6):
            plain.simulateSubsteps(SUB, DT, dict(dicts[1], worldBounds=PP["worldBounds"]))
        assert _same(_state(plain), _state(solos[1]))


# ---- 2. every field is read ---------------------------------------------------------------------------------------------------------------
def _low_lattice():
    return make_lattice(5, y0=0.0005)   # touches the floor y = 0 within the first frame, so that floor friction acts


@pytest.mark.parametrize("kw", [dict(solver="polar", precision="fast", ref_fixed_bounds=False), dict(solver="polar", precision="precise"),
                                dict(solver="neohookean", precision="fast"), dict(solver="neohookean", precision="precise"),
                                dict(solver="neohookean", precision="fast", order="clustered")])
def test_every_field_of_a_row_is_read(kw):
    """A solo that differs from the body's row in exactly ONE value ends in other bits, wherever that value acts; a silently ignored field
    would pass the test above with rows that happen not to matter.

    The body is a lattice resting on the floor, with a wall 1 mm inside it: floor friction acts only below y = 0, which a body that starts
    30 cm up does not reach in six frames.  The CPU oracle (oracle/orc.py) meets the same condition on this body with these rows: within
    six frames OracleNH ends in other bits for each of gravity, friction, devCompliance, volCompliance and worldBounds, OraclePJ for gravity
    and friction.  OraclePJ is the reference's polar solver, which has the constant box and no compliances, so bounds without the
    fixed-bounds flag have no oracle; there the twins themselves must differ."""
    v, t = _low_lattice()
    meshes = [_mesh("dragon"), (v, t)]
    hi = v.astype(np.float64).max(0)
    row = dict(PP, gravity=-3.0, friction=0.5, devCompliance=1e-4, volCompliance=1e-6, worldBounds=[-2.5, -1.0, -2.5, float(hi[0]) - 0.001, 10.0, 2.5])   # (a wall 1 mm inside the body: the clamp acts at once)
    batch = SoftBodyHIP.batch(meshes, dict(PP), **kw)
    batch.setBodyParams([None, row])
    changes = dict(gravity=-3.5, friction=0.25)
    if kw["solver"] == "neohookean":
        changes.update(devCompliance=2e-4, volCompliance=2e-6)
    if not _fixed(kw):
        changes["worldBounds"] = [-2.5, -1.0, -2.5, float(hi[0]) - 0.002, 10.0, 2.5]
    twins = {k: SoftBodyHIP(v, t, None, dict(PP), **kw) for k in ["same"] + list(changes)}
    for _ in range(6):
        batch.simulateSubsteps(SUB, DT, PP)
        for k, twin in twins.items():
            twin.simulateSubsteps(SUB, DT, row if k == "same" else dict(row, **{k: changes[k]}))
    (p0, p1), _ = batch.bodyRanges[1]
    mine = [batch.pos[p0:p1], batch.vel[p0:p1]]
    assert _same(mine, [twins["same"].pos, twins["same"].vel])
    ignored = [k for k in changes if _same(mine, [twins[k].pos, twins[k].vel])]
    assert ignored == []


# ---- 3. the large paths on a single body ----------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("case", list(LARGE_CASES))
def test_a_single_body_with_its_row_equals_its_twin_stepped_with_the_same_values(case):
    mesh, kw, path = LARGE_CASES[case]
    v, t = _mesh(mesh)
    a, b, none = (SoftBodyHIP(v, t, None, dict(PP), **kw) for _ in range(3))
    _path(a, path)
    row = dict(PP, gravity=-3.0, friction=0.0, devCompliance=1e-4, volCompliance=1e-6)
    row["worldBounds"] = [-2.5, float(v[:, 1].min()) - 0.02, -2.5, 2.5, 10.0, 2.5]
    a.setBodyParams([row])
    for _ in range(3):
        a.simulateSubsteps(SUB, DT, PP)
        b.simulateSubsteps(SUB, DT, row)
        none.simulateSubsteps(SUB, DT, PP)
    assert _same(_state(a), _state(b)) and not _same(_state(a), _state(none))


# ---- 4. one call of n = n calls -------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("kw,path", [(dict(solver="polar", precision="fast"), 3), (dict(solver="polar", precision="fast", lean_state=True), 2),
                                     (dict(solver="neohookean", precision="fast"), 4)])
def test_one_call_of_n_substeps_equals_n_calls(kw, path):
    v, t = _mesh("dragon")
    a, b = (SoftBodyHIP(v, t, None, dict(PP), **kw) for _ in range(2))
    _path(a, path)
    for f in range(4):
        row = dict(PP, gravity=-3.0 - f, friction=0.5 * f, devCompliance=1e-4)
        a.setBodyParams([row])
        b.setBodyParams([row])
        a.simulateSubsteps(SUB, DT, PP)
        for _ in range(SUB):
            b.simulate(DT, PP)
    assert _same(_state(a), _state(b))


# ---- 5. ON, other rows, OFF, ON again between calls ------------------------------------------------------------------------------------------
@pytest.mark.parametrize("mesh,kw,path", [("dragon", dict(solver="polar", precision="fast"), 3), ("dragon", dict(solver="neohookean", precision="fast"), 4),
                                          ("dragon", dict(solver="neohookean", precision="precise"), 4),
                                          ("lat30", dict(solver="neohookean", precision="fast", order="clustered"), 0)])
def test_switching_on_and_off_between_calls_equals_the_twin(mesh, kw, path):
    """step, ON, other rows (nothing else changes: the host's parameter block compares equal, the rows must still be fresh), OFF, ON again"""
    v, t = _mesh(mesh)
    a, b = (SoftBodyHIP(v, t, None, dict(PP), **kw) for _ in range(2))
    _path(a, path)
    first = dict(PP, gravity=-3.0, friction=0.0, devCompliance=1e-4, volCompliance=1e-6)
    second = dict(PP, gravity=4.0, friction=2.0, devCompliance=3e-5)
    for f, row in enumerate([None, first, second, second, None, first]):
        a.setBodyParams(None if row is None else [row])
        for body in (a, b):
            body.simulateSubsteps(SUB, DT, PP if body is a or row is None else row)
            if f % 2:
                body.simulate(DT, PP if body is a or row is None else row)
    assert _same(_state(a), _state(b))


# ---- 6. the device variant --------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("kw", [dict(solver="polar", precision="fast"), dict(solver="neohookean", precision="precise")])
def test_device_rows_equal_host_rows(kw):
    meshes = _three()
    dicts = _dicts(meshes)
    rows = body_param_rows(dicts, PP)
    later = rows.copy()
    later[:, capi.BP_GRAVITY] += 1.0
    host, dev = (SoftBodyHIP.batch(meshes, dict(PP), **kw) for _ in range(2))
    stream = torch.cuda.Stream()
    dev.setBodyParamsDevice(torch.tensor(rows, device="cuda"))   # (the first call allocates)
    torch.cuda.current_stream().synchronize()
    with torch.cuda.stream(stream):   # rows that a kernel on a side stream fills, in a [:, :10] view of a wider tensor
        wide = torch.full((3, 13), float("nan"), dtype=torch.float64, device="cuda")
        wide[:, :10].copy_(torch.tensor(later, device="cuda"))
        wide[2, capi.BP_FRICTION] = float("nan")   # a row the table cannot hold: body 2 keeps its row
        dev.setBodyParamsDevice(wide[:, :10], bodies=torch.tensor([True, False, True], device="cuda"), stream=stream)
        wide.fill_(float("inf"))   # harmless: the set kernel is ahead of it on this stream
    effective = rows.copy()
    effective[0] = later[0]   # body 1: left out by the mask; body 2: its NaN row was left alone
    host.setBodyParams(effective)
    for body in (host, dev):
        for _ in range(3):
            body.simulateSubsteps(SUB, DT, PP)
    assert _same(_state(host), _state(dev))
    stream.synchronize()


# ---- 7. together with the other tables -------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("kw", [dict(solver="polar", precision="fast"), dict(solver="neohookean", precision="fast")])
def test_grabs_colliders_and_params_together_equal_the_solos(kw):
    meshes = _three()
    dicts = _dicts(meshes)
    batch = SoftBodyHIP.batch(meshes, dict(PP), **kw)
    solos = [SoftBodyHIP(v, t, None, dict(PP), **kw) for v, t in meshes]
    held = [GRAB_ID, 11, -1]
    lists = [cref.f32_scene(meshes[0][0] + np.float32([0.0, 0.06, 0.0]), 0), cref.f32_scene(meshes[1][0] + np.float32([0.0, 0.2, 0.0]), 0)[2:], []]
    batch.setBodyParams(dicts)
    batch.setBodyColliders(lists)
    for f in range(4):
        x = np.stack([_target(v, max(p, 0), f) for (v, _), p in zip(meshes, held)])
        batch.setBodyGrabs(held, x)
        batch.simulateSubsteps(SUB, DT, PP)
        for solo, p, xi, cs, d in zip(solos, held, x, lists, dicts):
            if p >= 0:
                solo.setGrab(p, xi)
            solo.setColliders(cs)
            solo.simulateSubsteps(SUB, DT, d)
    assert _same_bodies(batch, solos) == []


# ---- 8. the crowd -------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("kw", [dict(solver="polar", precision="fast"), dict(solver="neohookean", precision="fast")])
def test_the_crowd_equals_its_solos(kw):
    cr = crowd.build()
    pos, vel = cr.state(3)
    batch = SoftBodyHIP.batch(cr.bodies, dict(crowd.PP), **kw)
    batch.writeState(pos, vel)
    rng = np.random.default_rng(20)
    dicts = []
    for v, _ in cr.bodies:
        lo = v.astype(np.float64).min(0)
        dicts.append(dict(crowd.PP, gravity=rng.uniform(-12.0, 3.0), friction=rng.uniform(0.0, 100.0), devCompliance=10.0 ** rng.uniform(-6, -3),
                          volCompliance=rng.uniform(0.0, 1e-6), worldBounds=[-20.0, lo[1] - rng.uniform(0.0, 0.01), -20.0, 20.0, 10.0, 20.0]))
    batch.setBodyParams(dicts)
    solos = []
    for b in crowd.SAMPLE:
        s = SoftBodyHIP(*cr.bodies[b], None, dict(crowd.PP), **kw)
        s.writeState(cr.body(b, pos), cr.body(b, vel))
        solos.append(s)
    for _ in range(2):
        batch.simulateSubsteps(SUB, DT, crowd.PP)
        for s, b in zip(solos, crowd.SAMPLE):
            s.simulateSubsteps(SUB, DT, dicts[b])
    assert _same_bodies(Sampled(batch), solos) == []


# ---- 9. errors, each leaving the state and the table as they were ------------------------------------------------------------------------
def test_errors_leave_state_and_table_alone():
    L = capi.lib()
    meshes = _three()
    kw = dict(solver="polar", precision="fast")
    dicts = _dicts(meshes)
    a, twin = (SoftBodyHIP.batch(meshes, dict(PP), **kw) for _ in range(2))
    size = C.c_uint64()
    assert L.tetsim_state_size(a._h, C.byref(size)) == 0
    blank = size.value
    rows = body_param_rows(dicts, PP)
    twin.setBodyParams(rows)

    def step_and_compare():
        for body in (a, twin):
            body.simulateSubsteps(SUB, DT, PP)
            body.simulate(DT, PP)
        assert _same(_state(a), _state(twin))

    # strides of 80 and 88 bytes are served, and rows as nested lists; what they leave is the twin's table
    a.setBodyParams(rows.tolist())
    a.setBodyParamsDevice(torch.tensor(rows, device="cuda"))
    wide88 = torch.zeros((3, 11), dtype=torch.float64, device="cuda")
    wide88[:, :10] = torch.tensor(rows, device="cuda")
    assert wide88.stride(0) * 8 == 88
    a.setBodyParamsDevice(wide88[:, :10])
    assert L.tetsim_state_size(a._h, C.byref(size)) == 0 and size.value == blank   # the table is not solver state
    step_and_compare()
    # the refused device calls: every one brings rows that WOULD change every body (gravity 5 upwards) ...
    other = rows.copy()
    other[:, capi.BP_GRAVITY] = 5.0
    dev = torch.tensor(other, device="cuda")
    for stride in (8, 72, 84):
        assert L.tetsim_set_body_params_device(a._h, dev.data_ptr(), stride, None, None) == capi.EINVAL and b"row_stride" in L.tetsim_last_error(a._h)
    assert L.tetsim_set_body_params_device(a._h, dev.data_ptr() + 4, 0, None, None) == capi.EINVAL           # misaligned
    assert L.tetsim_set_body_params_device(a._h, other.ctypes.data, 0, None, None) == capi.EINVAL and b"not device memory" in L.tetsim_last_error(a._h)
    hip = _hip_runtime()
    short = C.c_void_p()
    assert hip.hipMalloc(C.byref(short), C.c_size_t(3 * 80 - 8)) == 0   # an allocation of its own, one double short
    assert L.tetsim_set_body_params_device(a._h, short.value, 0, None, None) == capi.EINVAL and b"do not fit" in L.tetsim_last_error(a._h)
    host_mask = np.ones(3, np.uint8)
    assert L.tetsim_set_body_params_device(a._h, dev.data_ptr(), 0, host_mask.ctypes.data, None) == capi.EINVAL     # a mask in host memory; below: a mask of which only two bytes fit
    assert L.tetsim_set_body_params_device(a._h, dev.data_ptr(), 0, short.value + (3 * 80 - 8) - 2, None) == capi.EINVAL and b"do not fit" in L.tetsim_last_error(a._h)
    with pytest.raises(ValueError):
        a.setBodyParamsDevice(dev[:, :9])
    # ... and with no set call in between, the bodies step as the twin's do: nothing was enqueued, the table is as it was
    step_and_compare()
    # the refused host row names its body; bodies 0 and 2 of that call carry good rows that would change them, and do not
    bad = other.copy()
    bad[1, capi.BP_BOUNDS_HI + 1] = np.inf
    with pytest.raises(TetSimError) as e:
        a.setBodyParams(bad)
    assert e.value.code == capi.EINVAL and "body 1" in str(e.value)
    with pytest.raises(ValueError):
        a.setBodyParams([[1.0, 2.0]] * 3)
    step_and_compare()
    # a partitioned body
    lv, lt = _mesh("lat12")
    owner = (np.arange(len(lv)) * 2 // len(lv)).astype(np.int32)
    part = SoftBodyHIP(lv, lt, None, dict(PP), solver="polar", precision="fast", part_count=2, part_index=0, vert_owner=owner)
    assert _code(part.setBodyParams, rows[:1]) == capi.ESTATE
    assert _code(part.setBodyParamsDevice, dev[:1]) == capi.ESTATE
    torch.cuda.synchronize()
    assert hip.hipFree(short) == 0
