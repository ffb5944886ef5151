"""Per-body pose on the device (include/tetsim.h: tetsim_body_poses_device / tetsim_read_body_poses; SoftBodyHIP.observePoses /
bodyPoses) against tests/pose_ref.py.

THE BOUNDS.  The raw moments [0..25] are f64 sums of products of the f64 table and the f32 state, every operation rounded once, added in a
fixed tree.  pose_ref.raw evaluates the same sums over Fractions of the same table (tetsim_prep_pose_table: the records the device reads)
and the read-back state, and returns S, the sum of the absolute values of the terms: a value is within c * 2^-53 * S of the exact one, c =
the roundings on a term's path + the body's particle count (pose_ref.raw_bounds).  The derived values [26..47] are a fixed procedure of
+ - * / sqrt on the stored raw values and must equal pose_ref.derived(row[0:26]) BIT FOR BIT.  A placed rest body is held to the bounds
tests/test_pose_cpu.py derives (angle, OMEGA, VCOM), and its RESIDUAL to
    sqrt((2 * rms delta)^2 + e),   e = what the rounding of the raw sums and of lambda_max can add to ((T + Q0) - 2 lambda_max) / MASS
(pose_ref.residual_floor: the best fit is no worse than the true motion, whose rms distance is at most the rms of the f32 store
roundings delta_i; twice that covers the second-order terms; RESIDUAL^2 is a difference of sums about the origin, hence e).
Nothing here was measured on a GPU first; nothing is in tolerances.json.

Bodies and meshes: those of tests/test_gpu_observe.py (its Case)."""
import ctypes as C
from fractions import Fraction

import numpy as np
import pytest
import torch

from conftest import load_mesh
import place_ref
import pose_ref as R
from test_gpu_device_io import DT, KINDS, PP
from test_gpu_observe import Case, bits, f32bits, is_sentinel, sentinel_rows
from test_gpu_snapshot import _hip_runtime, device_bytes
from test_pose_cpu import check_placed, prep_table
from tetsim_amd import SoftBodyHIP, TetSimError, make_lattice, place_rows
from tetsim_amd import _capi as capi

pytestmark = pytest.mark.gpu
MESHES = ["dragon", "lat4", "dragon3", "mixed", "hub"]
W = capi.POSE_WIDTH


def table_of(c):
    """The records the device reads: tetsim_prep_pose_table of the Case's concatenation."""
    batch = len(c.parts) > 1
    return prep_table(c.rest, c.tets, c.first_vert if batch else None, c.first_tet if batch else None, PP["density"])[0]


def rows_of(t):
    return t.detach().cpu().numpy().astype(np.float64).reshape(-1, W).copy()


def check_rows(label, rows, tbl, pos, vel, first_vert=None, nan_bodies=()):
    """Every body's row: [0..25] within pose_ref.raw_bounds of the exact sums, [26..47] = pose_ref.derived of its own [0..25] bit for bit."""
    ref = R.raw(tbl, pos, vel, first_vert)
    assert rows.shape == (len(ref), W)
    want = R.derived(rows)
    for b, (row, o) in enumerate(zip(rows, ref)):
        bound, worst = R.raw_bounds(o), 0.0
        for k in range(R.RAW):
            if isinstance(o["value"][k], float):
                assert np.isnan(row[k]), (label, b, k, row[k])
                continue
            err = abs(Fraction(float(row[k])) - o["value"][k])
            assert np.isfinite(row[k]) and err <= bound[k], (label, b, k, row[k], float(o["value"][k]), float(err), float(bound[k]))
            worst = max(worst, float(err / bound[k]) if bound[k] else 0.0)
        print("%s body %d: worst |error| / bound of the raw moments = %.3g; Q %s RESIDUAL %.3g GAP %.3g" % (label, b, worst, row[R.Q:R.Q + 4], row[R.RESIDUAL], row[R.GAP]))
        if b in nan_bodies:                                          # (a NaN's payload is nobody's promise: which values are NaN is)
            assert np.array_equal(row[R.RAW:], want[b], equal_nan=True) and np.isnan(row[R.Q:R.Q + 4]).all() and np.isnan(row[R.COM:R.COM + 3]).all()
        else:
            assert np.array_equal(bits(row[R.RAW:]), bits(want[b])), (label, b, row[R.RAW:], want[b])
        assert not bits(row[R.RESERVED:]).any()
    return ref


# ---- 1. against the reference, behind 20 substeps and without a synchronisation in between ---------------------------------------------
@pytest.mark.parametrize("kind", list(KINDS))
@pytest.mark.parametrize("mesh", MESHES)
def test_pose_follows_the_step_and_equals_the_reference(mesh, kind):
    c = Case(mesh, kind)
    c.body.simulateSubsteps(20, DT, c.pp)
    poses = c.body.observePoses()
    torch.cuda.synchronize()
    assert poses.dtype == torch.float64 and poses.is_cuda and tuple(poses.shape) == (len(c.parts), W)
    pos, vel = c.body.pos, c.body.vel
    assert np.isfinite(pos).all() and np.isfinite(vel).all() and np.abs(vel).max() > 0
    rows = rows_of(poses)
    check_rows("%s/%s" % (mesh, kind), rows, table_of(c), pos, vel, c.first_vert)
    q = rows[:, R.Q:R.Q + 4]
    assert np.allclose(np.linalg.norm(q, axis=1), 1.0, rtol=0, atol=2.0 ** -50) and (q[:, 3] > 0.9).all()   # 20 substeps of free fall: barely turned
    obs = c.body.bodyObservations()                                  # the other half of the rigid state: the same mass centre by another sum
    assert np.allclose(rows[:, R.COM:R.COM + 3], obs[:, capi.OBS_COM:capi.OBS_COM + 3], rtol=0, atol=1e-9)
    assert np.allclose(rows[:, R.MASS], obs[:, capi.OBS_MASS], rtol=1e-12)


# ---- 2. a constructed state: the inverse of a placement, and INTEGRATION.md 4j's snippet -----------------------------------------------
def stand_up_rows(poses):
    """rows that undo every body's rotation about its mass centre, built on the device from the pose rows."""
    rows = torch.zeros((poses.shape[0], capi.PLACE_WIDTH), dtype=torch.float32, device=poses.device)
    q = poses[:, capi.POSE_Q:capi.POSE_Q + 4]
    rows[:, capi.PLACE_Q:capi.PLACE_Q + 3] = -q[:, :3]               # the conjugate: the rotation back
    rows[:, capi.PLACE_Q + 3] = q[:, 3]
    rows[:, capi.PLACE_PIVOT:capi.PLACE_PIVOT + 3] = poses[:, capi.POSE_COM:capi.POSE_COM + 3]
    return rows


@pytest.mark.parametrize("kind", list(KINDS))
def test_a_placed_rest_body_reports_its_placement_and_stands_up_again(kind):
    c = Case("mixed", kind)
    tbl = table_of(c)
    rng = np.random.default_rng(5)
    q = rng.standard_normal((3, 4))
    q[0, 3], q[2] = -abs(q[0, 3]), [0.0, 0.0, 1.0, 0.0]              # one with w < 0, one half turn
    centres = np.stack([c.rest[int(c.first_vert[b]):int(c.first_vert[b + 1])].mean(axis=0) for b in range(3)])
    rows = place_rows(q, centres + rng.uniform(-0.1, 0.1, (3, 3)), rng.uniform(-0.5, 0.5, (3, 3)) + [0.0, 1.0, 0.0], rng.uniform(-1, 1, (3, 3)), rng.uniform(-2, 2, (3, 3)))
    c.body.placeBodies(rows, bodies=[True, False, True])
    poses = c.body.observePoses()
    got = rows_of(poses)
    pos, vel = c.body.pos, c.body.vel
    ref = check_rows("placed/" + kind, got, tbl, pos, vel, c.first_vert)
    for b in range(3):
        lo, hi = int(c.first_vert[b]), int(c.first_vert[b + 1])
        row = rows[b] if b != 1 else place_rows([0.0, 0.0, 0.0, 1.0])[0]
        if b != 1:                                                   # (what place_ref says the state is, bit for bit: tests/test_gpu_place.py)
            want_pos, want_vel = place_ref.place_particles(row, c.rest[lo:hi], np.zeros((hi - lo, 3), np.float32))
            assert np.array_equal(f32bits(pos[lo:hi]), f32bits(want_pos)) and np.array_equal(f32bits(vel[lo:hi]), f32bits(want_vel))
        rms = check_placed("placed/%s body %d" % (kind, b), row, tbl[lo:hi], pos[lo:hi], vel[lo:hi], got[b])
        floor = R.residual_floor(ref[b], got[b])
        print("  RESIDUAL %.3g, allowed %.3g (rms delta %.3g, rounding floor %.3g)" % (got[b, R.RESIDUAL], np.sqrt(4 * rms * rms + floor), rms, np.sqrt(floor)))
        assert got[b, R.RESIDUAL] <= np.sqrt(4 * rms * rms + floor)
    assert not got[1, R.OMEGA:R.OMEGA + 3].any() and not got[1, R.L:R.L + 3].any()
    # ... and back on their feet, without a host copy: the snippet of INTEGRATION.md 4j
    c.body.placeBodiesDevice(stand_up_rows(poses), bodies=[True, False, True])
    again = rows_of(c.body.observePoses())
    pos2, vel2 = c.body.pos, c.body.vel
    for b in (0, 2):
        lo, hi = int(c.first_vert[b]), int(c.first_vert[b + 1])
        angle_b = R.placement_bounds(tbl[lo:hi], pos2[lo:hi], vel2[lo:hi], np.zeros(3))[0]
        angle = R.quat_angle(again[b, R.Q:R.Q + 4], [0.0, 0.0, 0.0, 1.0])
        # the row's quaternion is the pose's rounded to f32 (each component within 2^-25: a 4-vector error below 2^-24, an angle below
        # 2^-23) of a rotation that was itself within the first placement's angle bound; then the new state's own bound
        allow = angle_b + 2.0 ** -23 + R.placement_bounds(tbl[lo:hi], pos[lo:hi], vel[lo:hi], place_ref.Motion(rows[b]).angular)[0]
        print("stood up/%s body %d: angle to the identity %.3g, allowed %.3g" % (kind, b, angle, allow))
        assert angle <= allow
        assert np.allclose(again[b, R.COM:R.COM + 3], got[b, R.COM:R.COM + 3], rtol=0, atol=1e-5)   # turned about its mass centre
    assert np.array_equal(bits(again[1]), bits(got[1]))


# ---- 3. a mirrored body, a NaN ------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("kind", ["polar-fast", "nh-fast"])
def test_a_mirrored_dragon_gets_a_proper_rotation_and_a_nan_stays_in_its_body(kind):
    c = Case("dragon3", kind)
    tbl = table_of(c)
    zero = np.zeros_like(c.rest)
    c.body.writeState(c.rest, zero)
    before = rows_of(c.body.observePoses())
    ref = check_rows("rest/" + kind, before, tbl, c.rest, zero, c.first_vert)
    for b in range(3):                                               # at rest: the identity, and no residual but the rounding floor
        assert before[b, R.RESIDUAL] <= np.sqrt(R.residual_floor(ref[b], before[b])) and R.quat_angle(before[b, R.Q:R.Q + 4], [0, 0, 0, 1]) < 1e-6
    v0, v1 = int(c.first_vert[1]), int(c.first_vert[2])
    pos = c.rest.copy()
    pos[v0:v1, 0] = (np.float32(2.0) * pos[v0:v1, 0].mean(dtype=np.float64).astype(np.float32) - pos[v0:v1, 0]).astype(np.float32)   # mirrored in x about its own centroid
    c.body.writeState(pos, zero)
    rows = rows_of(c.body.observePoses())
    check_rows("mirrored/" + kind, rows, tbl, pos, zero, c.first_vert)
    q = rows[1, R.Q:R.Q + 4]
    size = np.sqrt(rows[1, R.Q0] / rows[1, R.MASS])                 # the body's rms radius
    print("mirrored: Q %s, RESIDUAL %.3g of an rms radius of %.3g, GAP %.3g" % (q, rows[1, R.RESIDUAL], size, rows[1, R.GAP]))
    assert abs(np.linalg.norm(q) - 1.0) <= 2.0 ** -50
    # Kabsch: the best proper rotation onto a mirror image P q has S m |R q - P q|^2 = 4 mu_1, mu_1 the smallest eigenvalue of
    # B = S m q q^T (the singular values of P B are B's eigenvalues, and the determinant fix gives up the smallest one twice):
    # RESIDUAL = 2 sqrt(mu_1 / MASS) up to the f32 store of the mirrored positions -- large, of the order of the body's thickness
    B = np.einsum("i,ia,ib->ab", tbl["m"][v0:v1], tbl["q"][v0:v1], tbl["q"][v0:v1])
    thick = np.sqrt(np.linalg.eigvalsh(B)[0] / rows[1, R.MASS])
    assert 1.999 * thick <= rows[1, R.RESIDUAL] <= 2.001 * thick and rows[1, R.RESIDUAL] > 0.01 * size
    assert np.array_equal(bits(rows[[0, 2]]), bits(before[[0, 2]]))
    pos = c.rest.copy()
    pos[v0 + 7] = np.nan                                             # one particle of body 1
    c.body.writeState(pos, zero)
    rows = rows_of(c.body.observePoses())
    check_rows("nan/" + kind, rows, tbl, pos, zero, c.first_vert, nan_bodies=(1,))
    assert np.isnan(rows[1, R.MX:R.MX + 3]).all() and np.isnan(rows[1, R.A:R.A + 9]).all() and np.isnan(rows[1, R.G:R.G + 6]).all()
    assert rows[1, R.MASS] == before[1, R.MASS] and rows[1, R.Q0] == before[1, R.Q0]
    assert np.array_equal(bits(rows[[0, 2]]), bits(before[[0, 2]]))


# ---- 4. reproducible and position independent ---------------------------------------------------------------------------------------------
@pytest.mark.parametrize("kind", list(KINDS))
@pytest.mark.parametrize("mesh", ["dragon3", "mixed"])
def test_same_bits_again_and_same_bits_alone(mesh, kind):
    c = Case(mesh, kind)
    c.body.simulateSubsteps(20, DT, c.pp)
    first = rows_of(c.body.observePoses())
    again = rows_of(c.body.observePoses())
    assert np.array_equal(bits(first), bits(again))
    pos, vel = c.body.pos, c.body.vel
    for b in range(len(c.parts)):
        solo = c.solo(b)
        lo, hi = int(c.first_vert[b]), int(c.first_vert[b + 1])
        solo.writeState(pos[lo:hi], vel[lo:hi])                      # the same state, whatever path the solo body would step through
        assert np.array_equal(f32bits(solo.pos), f32bits(pos[lo:hi])) and np.array_equal(f32bits(solo.vel), f32bits(vel[lo:hi]))
        alone = rows_of(solo.observePoses())
        assert alone.shape == (1, W) and np.array_equal(bits(alone[0]), bits(first[b])), (mesh, kind, b, alone[0], first[b])


# ---- 5. the contract ------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("kind", ["polar-fast", "nh-precise-coloured"])
def test_strided_rows_leave_padding_and_guard_rows_alone(kind):
    c = Case("dragon3", kind)
    c.body.simulateSubsteps(20, DT, c.pp)
    buf = sentinel_rows(3 + 2, 64)                                   # rows 512 bytes apart, one guard row in front, one behind
    view = buf[1:-1, :W]
    assert view.stride(0) * 8 == 512 and view.data_ptr() == buf.data_ptr() + 512
    packed = c.body.observePoses()
    assert c.body.observePoses(out=view) is view
    torch.cuda.synchronize()
    assert np.array_equal(bits(view), bits(packed)) and not is_sentinel(view[:, :1])
    assert is_sentinel(buf[0]) and is_sentinel(buf[-1]) and is_sentinel(buf[1:-1, W:])
    assert np.array_equal(bits(c.body.bodyPoses()), bits(packed))
    assert c.body.observePoses() is packed                           # allocated once, reused


@pytest.mark.parametrize("side_stream", [False, True], ids=["default-stream", "side-stream"])
@pytest.mark.parametrize("kind", ["polar-fast", "nh-fast"])
def test_a_reused_tensor_is_ordered_on_its_stream(kind, side_stream):
    """observe, clone, step, observe into the same tensor -- one synchronisation at the end.  The references come from a twin body."""
    c, twin = Case("dragon", kind), Case("dragon", kind)
    twin.body.simulateSubsteps(20, DT, c.pp)
    first = twin.body.bodyPoses()
    twin.body.simulateSubsteps(20, DT, c.pp)
    second = twin.body.bodyPoses()
    assert not np.array_equal(bits(first), bits(second))
    stream = torch.cuda.Stream() if side_stream else torch.cuda.current_stream()
    with torch.cuda.stream(stream):
        c.body.simulateSubsteps(20, DT, c.pp)
        t = c.body.observePoses()
        kept = t.clone()
        c.body.simulateSubsteps(20, DT, c.pp)
        t2 = c.body.observePoses(stream=stream if side_stream else None)
    torch.cuda.synchronize()
    assert t2 is t
    assert np.array_equal(bits(kept), bits(first))
    assert np.array_equal(bits(t), bits(second))


@pytest.mark.parametrize("kind", ["polar-fast", "nh-fast"])
def test_refusals_leave_dst_and_the_next_step_alone(kind):
    L = capi.lib()
    c, twin = Case("dragon3", kind), Case("dragon3", kind)
    for x in (c, twin):
        x.body.simulateSubsteps(20, DT, x.pp)
    h, nb = c.body._h, 3
    dst = sentinel_rows(nb + 1, W)
    p = dst.data_ptr()
    host = np.full(nb * W, np.nan)
    hip = _hip_runtime()
    short = C.c_void_p()
    assert hip.hipMalloc(C.byref(short), C.c_size_t(nb * 8 * W - 8)) == 0        # an allocation of its own, one double too short
    assert hip.hipMemset(short, 0xA5, C.c_size_t(nb * 8 * W - 8)) == 0
    d0 = device_bytes(c.body)
    for args, text in (((None, 0), "null"), ((p + 4, 0), "aligned"), ((p + 2, 384), "aligned"), ((p, 8), "row_stride"), ((p, 376), "row_stride"),
                       ((p, 388), "row_stride"), ((p, 160), "row_stride"), ((host.ctypes.data, 0), "not device memory"), ((short.value, 0), "do not fit")):
        rc = L.tetsim_body_poses_device(h, args[0], args[1], None)
        assert rc == capi.EINVAL, (args, rc, L.tetsim_last_error(h))
        assert text.encode() in L.tetsim_last_error(h), (args, L.tetsim_last_error(h))
    assert L.tetsim_read_body_poses(h, None) == capi.EINVAL
    torch.cuda.synchronize()
    assert is_sentinel(dst) and np.isnan(host).all() and device_bytes(c.body) == d0   # (not even the tables were made)
    back = np.zeros(nb * 8 * W - 8, np.uint8)
    assert hip.hipMemcpy(C.c_void_p(back.ctypes.data), short, C.c_size_t(back.size), 2) == 0 and (back == 0xA5).all()
    assert hip.hipFree(short) == 0
    for bad in (dst[:nb].float(), dst[:nb - 1], dst[:nb, :W - 1], torch.zeros((nb, W), dtype=torch.float64)):
        with pytest.raises(ValueError):
            c.body.observePoses(out=bad)
    assert is_sentinel(dst)
    # ... and the next step and the next good call are right, in step with a twin that was never refused anything
    for x in (c, twin):
        x.body.simulateSubsteps(5, DT, x.pp)
    got = c.body.observePoses(out=dst[:nb])
    torch.cuda.synchronize()
    assert np.array_equal(f32bits(c.body.pos), f32bits(twin.body.pos)) and np.array_equal(f32bits(c.body.vel), f32bits(twin.body.vel))
    assert np.array_equal(bits(got), bits(twin.body.bodyPoses())) and is_sentinel(dst[nb:])


@pytest.mark.parametrize("kind", list(KINDS))
def test_device_bytes_grow_with_the_first_call_only(kind):
    c = Case("mixed", kind)
    c.body.simulateSubsteps(3, DT, c.pp)
    d0 = device_bytes(c.body)
    first = rows_of(c.body.observePoses())
    d1 = device_bytes(c.body)
    nv, chunks = len(c.rest), sum(-(-len(v) // 256) for v, _ in c.parts)
    assert d1 >= d0 + 32 * nv + 208 * chunks + 384 * len(c.parts)    # the table (32 bytes per particle), the chunk rows (26 doubles), the host read's rows
    assert d1 <= d0 + 32 * nv + 224 * chunks + 400 * len(c.parts) + 4 * nv   # ... the chunk and body tables (8 bytes each); a polar body's index map
    host = c.body.bodyPoses()
    c.body.observePoses(out=sentinel_rows(3, 64)[:, :W])
    c.body.simulateSubsteps(3, DT, c.pp)
    c.body.observePoses()
    assert device_bytes(c.body) == d1
    assert np.array_equal(bits(host), bits(first))


def test_a_partitioned_body_is_refused():
    v, t = load_mesh("lat4")
    parts = [SoftBodyHIP(v, t, None, dict(PP), solver="polar", precision="fast", part_count=2, part_index=i) for i in range(2)]
    for part in parts:
        dst = sentinel_rows(1, W)
        with pytest.raises(TetSimError) as e:
            part.observePoses(out=dst)
        assert e.value.code == capi.ESTATE and "partitioned" in str(e.value)
        with pytest.raises(TetSimError) as e:
            part.bodyPoses()
        assert e.value.code == capi.ESTATE and "partitioned" in str(e.value)
        torch.cuda.synchronize()
        assert is_sentinel(dst)


def test_a_body_without_tets_gives_the_massless_row():
    v, _ = load_mesh("notets")
    t = np.zeros((0, 4), dtype=np.int32)
    body = SoftBodyHIP(v, t, None, dict(PP), solver="neohookean")
    for _ in range(10):
        body.simulate(DT * 2, PP)
    rows = body.bodyPoses()
    want = np.zeros(W)
    want[R.Q + 3] = 1.0
    assert rows.shape == (1, W) and np.array_equal(bits(rows[0]), bits(want))
    assert np.abs(body.vel).max() > 0


# ---- 6. more than 256 chunks in one body ------------------------------------------------------------------------------------------------------
def test_a_body_of_more_than_256_chunks():
    """The finish kernel's thread t folds the chunk rows t, t + 256, ..: the smallest lattice with more than 65,536 particles."""
    v, t = make_lattice(40)
    assert 256 * 256 < len(v) <= 41 ** 3
    body = SoftBodyHIP(v, t, None, dict(PP), solver="polar", precision="fast")
    vel = np.random.default_rng(3).normal(0.0, 1.5, v.shape).astype(np.float32)
    body.writeState(v, vel)
    rows = body.bodyPoses()
    tbl = prep_table(v, t, None, None, PP["density"])[0]
    check_rows("lat40", rows, tbl, v, vel)
    assert abs(rows[0, R.MASS] - 1000.0) < 1e-2 and R.quat_angle(rows[0, R.Q:R.Q + 4], [0, 0, 0, 1]) < 1e-6
    assert np.array_equal(bits(rows_of(body.observePoses())), bits(rows))
