"""Device snapshots (include/tetsim.h: tetsim_snapshot_*; SoftBodyHIP.snapshot / capture / restore): the complete solver state kept in
device memory, restored for the bodies a device-side mask names, with no host copy and no synchronisation.

Every comparison is on bits.  The yardsticks are the library's host path (saveState / loadState) and its guarantee that a body in a batch
equals its solo run bit for bit.  Kinds: those of test_gpu_device_io.py plus the constant-rest-shape polar body (no shape sections).
Meshes, all from tests/golden: lat4, the Dragon, lat12; and lat4 without its last three tets plus one particle no tet references, which
takes the one-launch call (fused_particle_pass == 5) at any size and whose 381 tets leave every section a short last 16-byte unit.
Every test prints the fused_particle_pass of its bodies."""
import ctypes as C

import numpy as np
import pytest
import torch

from conftest import load_mesh
from tetsim_amd import SoftBodyHIP, TetSimError
from tetsim_amd import _capi as capi
from test_gpu_device_io import DT, KINDS as IO_KINDS, PP, WIDE

pytestmark = pytest.mark.gpu
KINDS = dict(IO_KINDS)
KINDS["polar-fast-constant-rest"] = dict(solver="polar", precision="fast", constant_rest_shape=True)
POLAR_FAST = [k for k in KINDS if k.startswith("polar-fast")]
HEADER = 64   # sizeof(StateHeader), tetsim_state.hip: what a blob holds in front of the payload
SHIFTS = (-3.0, 0.0, 3.0)
BATCH = ("lat4", "dragon", "lat12")


def mesh(name):
    if name == "loose":
        v, t = load_mesh("lat4")
        return np.concatenate([v, [[0.25, 1.5, 0.25]]]).astype(np.float32), t[:-3]
    return load_mesh(name)


def solo(name, kind, shift=None):
    v, t = mesh(name)
    if shift is None:
        return SoftBodyHIP(v, t, None, dict(PP), **KINDS[kind])
    return SoftBodyHIP((v + np.array([shift, 0, 0], np.float32)).astype(np.float32), t, None, dict(WIDE), ref_fixed_bounds=False, **KINDS[kind])


def batch(kind):
    """lat4, the Dragon and lat12 side by side: 125 / 1234 / 2197 particles, so every body boundary falls inside a workgroup's chunk."""
    bodies = []
    for name, s in zip(BATCH, SHIFTS):
        v, t = mesh(name)
        bodies.append(((v + np.array([s, 0, 0], np.float32)).astype(np.float32), t))
    return SoftBodyHIP.batch(bodies, dict(WIDE), ref_fixed_bounds=False, **KINDS[kind])


def show(what, *bodies):
    print("%s: fused_particle_pass %s" % (what, [b.info.fused_particle_pass for b in bodies]))


def bits(a):
    return np.ascontiguousarray(a, dtype=np.float32).view(np.uint32)


def reads(body):
    """{name: bits} of everything the host can read of the state."""
    if body.solver == "polar":
        return {"pos": bits(body.pos), "vel": bits(body.vel), "quats": bits(body.quats)}
    return {"pos": bits(body.pos), "vel": bits(body.vel), "prevPos": bits(body.prevPos)}


def split(body, r):
    """reads() of a batch, body by body."""
    out = []
    for (p0, p1), (e0, e1) in body.bodyRanges:
        out.append({n: a[e0:e1] if n == "quats" else a[p0:p1] for n, a in r.items()})
    return out


def same(a, b):
    return list(a) == list(b) and all(np.array_equal(a[n], b[n]) for n in a)


def cuda_mask(values):
    return torch.tensor(values, dtype=torch.bool, device="cuda")


def device_bytes(body):
    info = capi.TetSimInfo()
    capi.check(body._L.tetsim_get_info(body._h, C.byref(info)), body._h)
    return info.device_bytes


# ---- 1. the whole handle ------------------------------------------------------------------------------------------------------------
ROUND_TRIP = [(k, m) for k in KINDS for m in ("lat4", "dragon")] + [(k, "loose") for k in POLAR_FAST]


@pytest.mark.parametrize("kind,name", ROUND_TRIP)
def test_restore_of_the_whole_handle_equals_load_state(kind, name):
    body = solo(name, kind)
    show("%s %s" % (kind, name), body)
    if kind == "polar-fast" and name == "loose":
        assert body.info.fused_particle_pass == 5
    body.simulateSubsteps(7, DT, PP)
    snap = body.snapshot()
    b0 = body.saveState()
    body.simulateSubsteps(13, DT, PP)
    r1 = reads(body)
    ve1 = body.volError if body.solver == "neohookean" else None
    body.simulateSubsteps(4, DT, PP)
    body.restore(snap)                       # (no sync() between the step call and the restore)
    assert body.saveState() == b0
    body.simulateSubsteps(13, DT, PP)
    assert same(reads(body), r1)
    if ve1 is not None:
        assert body.volError == ve1
    # ... and a one-byte mask on a single body is the same restore
    body.restore(snap, bodies=cuda_mask([1]))
    assert body.saveState() == b0
    body.restore(snap, bodies=cuda_mask([0]))
    body.simulateSubsteps(13, DT, PP)
    assert same(reads(body), r1)
    snap.close()
    body.close()


# ---- 2. / 3. / 5. masks in a batch --------------------------------------------------------------------------------------------------
_twins = {}


def twins(kind):
    """Per kind, computed once: the batch stepped 5, 10 and 20 substeps from creation, body by body."""
    if kind not in _twins:
        b = batch(kind)
        show("twin batch %s" % kind, b)
        out = {}
        done = 0
        for upto in (5, 10, 20):
            b.simulateSubsteps(upto - done, DT, WIDE)
            done = upto
            out[upto] = split(b, reads(b))
        b.close()
        assert not any(same(out[10][i], out[20][i]) or same(out[5][i], out[10][i]) for i in range(3))   # (a restore that did nothing would show)
        _twins[kind] = out
    return _twins[kind]


@pytest.mark.parametrize("kind", list(KINDS))
def test_masked_restore_in_a_batch(kind):
    tw = twins(kind)
    for mask in ([0, 1, 0], [1, 0, 1], [0, 0, 0], [1, 1, 1]):
        a = batch(kind)
        show("%s mask %s" % (kind, mask), a)
        snap = a.snapshot()
        a.simulateSubsteps(10, DT, WIDE)
        a.restore(snap, bodies=cuda_mask(mask))
        a.simulateSubsteps(10, DT, WIDE)
        got = split(a, reads(a))
        for b in range(3):   # a chosen body started again from the snapshot: 10 substeps from creation; the others never noticed
            assert same(got[b], tw[10 if mask[b] else 20][b]), (mask, b)
        a.close()


@pytest.mark.parametrize("kind", list(KINDS))
def test_masked_capture(kind):
    tw = twins(kind)
    a = batch(kind)
    show(kind, a)
    snap = a.snapshot()
    a.simulateSubsteps(5, DT, WIDE)
    a.capture(snap, bodies=[0, 0, 1])         # (a host sequence)
    a.simulateSubsteps(5, DT, WIDE)
    a.restore(snap)
    a.simulateSubsteps(5, DT, WIDE)
    got = split(a, reads(a))
    assert same(got[0], tw[5][0]) and same(got[1], tw[5][1])   # from the creation-time part of the snapshot
    assert same(got[2], tw[10][2])                              # captured at 5, restored, 5 more
    a.close()


@pytest.mark.parametrize("kind", ["polar-fast", "nh-fast"])
def test_the_mask_is_read_in_stream_order(kind):
    """The mask comes out of work enqueued on a side stream right before the call, and is overwritten on that stream right after it."""
    tw = twins(kind)
    a = batch(kind)
    show(kind, a)
    snap = a.snapshot()
    a.simulateSubsteps(10, DT, WIDE)
    side = torch.cuda.Stream()
    ones = torch.ones((4096, 4096), device="cuda")
    keep = torch.tensor([0.0, 1.0, 0.0], device="cuda")
    torch.cuda.synchronize()
    with torch.cuda.stream(side):
        x = ones @ ones                        # 4096 everywhere, after a while
        mask = (x[0, :3] * keep) > 1.0         # [0, 1, 0]
        a.restore(snap, bodies=mask, stream=side)
        mask.logical_not_()
    a.simulateSubsteps(10, DT, WIDE)
    got = split(a, reads(a))
    assert mask.cpu().tolist() == [True, False, True]
    for b, chosen in enumerate([0, 1, 0]):
        assert same(got[b], tw[10 if chosen else 20][b]), b
    a.close()


# ---- 4. a dt the snapshot was not taken with ----------------------------------------------------------------------------------------
@pytest.mark.parametrize("kind", ["polar-fast", "polar-precise"])
@pytest.mark.parametrize("masked", [False, True])
def test_dt_mismatch_single_dragon(kind, masked):
    a, y = solo("dragon", kind), solo("dragon", kind)
    show(kind, a, y)
    a.simulateSubsteps(7, DT, PP)
    snap = a.snapshot()
    blob = a.saveState()
    a.simulateSubsteps(6, 2 * DT, PP)
    a.restore(snap, bodies=cuda_mask([1]) if masked else None)
    a.simulateSubsteps(5, 2 * DT, PP)
    y.loadState(blob)
    y.simulateSubsteps(5, 2 * DT, PP)
    assert same(reads(a), reads(y))
    a.close(), y.close()


@pytest.mark.parametrize("kind", ["polar-fast", "polar-precise"])
def test_dt_mismatch_in_a_batch(kind):
    a, t = batch(kind), batch(kind)
    s = solo("dragon", kind, shift=SHIFTS[1])
    show(kind, a, t, s)
    for x in (a, t, s):
        x.simulateSubsteps(7, DT, WIDE)
    snap = a.snapshot()
    blob = s.saveState()                      # the chosen body's state of the same moment (a body in a batch equals its solo run)
    for x in (a, t):
        x.simulateSubsteps(6, 2 * DT, WIDE)
    a.restore(snap, bodies=cuda_mask([0, 1, 0]))
    moved = t.exportTensors(("pos", "vel"))   # the twin forces the same re-prediction on itself
    t.importTensors(moved["pos"], moved["vel"])
    s.loadState(blob)
    for x in (a, t, s):
        x.simulateSubsteps(5, 2 * DT, WIDE)
    got, twin = split(a, reads(a)), split(t, reads(t))
    assert same(got[1], reads(s))
    assert same(got[0], twin[0]) and same(got[2], twin[2])
    for x in (a, t, s):
        x.close()


# ---- 6. refusals --------------------------------------------------------------------------------------------------------------------
def _hip_runtime():
    """The HIP runtime this process already has loaded (torch's)."""
    for line in open("/proc/self/maps"):
        if "libamdhip64" in line:
            return C.CDLL(line.split()[-1])
    raise RuntimeError("no libamdhip64 in this process")


@pytest.mark.parametrize("kind", ["polar-fast", "nh-fast"])
def test_refusals_leave_everything_alone(kind):
    L = capi.lib()
    a, other = batch(kind), batch(kind)
    show(kind, a, other)
    a.simulateSubsteps(6, DT, WIDE)
    snap, foreign = a.snapshot(), other.snapshot()
    old = a.saveState()
    a.simulateSubsteps(6, DT, WIDE)
    before = a.saveState()
    good = cuda_mask([1, 1, 1])
    hip = _hip_runtime()
    short = C.c_void_p()
    assert hip.hipMalloc(C.byref(short), C.c_size_t(a.info.num_bodies - 1)) == 0   # an allocation of its own, one byte too short
    host = np.ones(3, dtype=np.uint8)
    for fn in (L.tetsim_snapshot_capture, L.tetsim_snapshot_restore):
        for args, text in (((foreign._s, good.data_ptr()), "another handle"), ((None, good.data_ptr()), "null"),
                           ((snap._s, host.ctypes.data), "not device memory"), ((snap._s, short.value), "do not fit")):
            rc = fn(a._h, args[0], args[1], None)
            assert rc == capi.EINVAL, (rc, L.tetsim_last_error(a._h))
            assert text.encode() in L.tetsim_last_error(a._h), L.tetsim_last_error(a._h)
    assert L.tetsim_snapshot_create(a._h, None) == capi.EINVAL
    with pytest.raises(ValueError):
        a.restore(snap, bodies=cuda_mask([1, 1]))
    with pytest.raises(ValueError):
        a.restore(snap, bodies=[1, 0])
    assert a.saveState() == before
    a.restore(snap)
    assert a.saveState() == old
    assert hip.hipFree(short) == 0
    a.close(), other.close()


def test_a_partitioned_body_is_refused():
    L = capi.lib()
    v, t = load_mesh("lat4")
    parts = [SoftBodyHIP(v, t, None, dict(PP), solver="polar", precision="fast", part_count=2, part_index=i) for i in range(2)]
    whole = solo("lat4", "polar-fast")
    show("partitions, whole", *parts, whole)
    snap = whole.snapshot()
    for part in parts:
        before = part.saveState()
        with pytest.raises(TetSimError) as e:
            part.snapshot()
        assert e.value.code == capi.ESTATE and "partitioned" in str(e.value)
        for fn in (L.tetsim_snapshot_capture, L.tetsim_snapshot_restore):
            assert fn(part._h, snap._s, None, None) == capi.ESTATE
            assert b"partitioned" in L.tetsim_last_error(part._h)
        assert part.saveState() == before
    for x in parts + [whole]:
        x.close()


# ---- 7. lifetime --------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("kind", list(KINDS))
def test_lifetime_and_device_bytes(kind):
    body = batch(kind)
    show(kind, body)
    body.simulateSubsteps(3, DT, WIDE)
    payload = len(body.saveState()) - HEADER
    d0 = device_bytes(body)
    s1 = body.snapshot()
    assert device_bytes(body) == d0 + payload
    s2 = body.snapshot()
    assert device_bytes(body) == d0 + 2 * payload
    s1.close()
    assert device_bytes(body) == d0 + payload and s1._s is None
    s1.close()                                # (twice is harmless)
    body.restore(s2)
    with pytest.raises(ValueError):
        body.restore(s1)
    body.close()                              # with s2 alive: the handle frees it
    assert s2._s is None
    s2.close()
    other = batch(kind)
    s3 = other.snapshot()
    s3.close()
    other.close()
