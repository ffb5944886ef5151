"""Touch sensing on the device (include/tetsim.h: tetsim_touch_bodies_device / tetsim_read_body_touch / tetsim_touch_particles_device;
SoftBodyHIP.touchBodies / bodyTouch / touchParticlesDevice) against tests/touch_ref.py.

NO TOLERANCE ANYWHERE: the header defines every value as a sequence of f64 operations, each rounded on its own, and a fixed reduction
tree; touch_ref restates both in numpy, and every comparison below is bit for bit (NaNs compare as NaN, whatever their payload).

Bodies: the five kinds of tests/test_gpu_device_io.py.  Meshes: lat4 (one partial chunk of particles), the Dragon (1,234 particles = 5
chunks, 3,840 tets, internal particle order), dragon3 and lat4 + Dragon + lat4 (body boundaries that are no multiple of 256)."""
import ctypes as C

import numpy as np
import pytest
import torch

import body_collider_ref
import touch_ref
from conftest import load_mesh
from test_gpu_device_io import DT, KINDS, PP
from test_gpu_observe import Case, f32bits
from test_gpu_snapshot import _hip_runtime, device_bytes
from tetsim_amd import SoftBodyHIP, TetSimError
from tetsim_amd import _capi as capi

pytestmark = pytest.mark.gpu
W, SW, PW, S0 = capi.TOUCH_WIDTH, capi.TOUCH_SLOT_WIDTH, capi.TOUCH_PARTICLE_WIDTH, capi.TOUCH_SLOT0
MARGINS = (0.0, 1e-3, -1e-3)
SENT64, SENT32 = 0x7FF8DEADDEADDEAD, 0x7FC0DEAD   # NaN payloads no kernel produces
AXES = ((0.6, 0.8, 0.0), (-0.8, 0.6, 0.0), (0.0, 0.0, 1.0))


def f32_lists(lists):
    """collider dicts with every value rounded to f32: what a row of the body-collider table can hold, so batch and solo get the same numbers"""
    return body_collider_ref.lists_from_rows(body_collider_ref.rows(lists))


def scene8(v):
    """All four kinds in one list of eight around the body with rest vertices v: a tilted plane it rests on, a sphere, a box and a capsule
    that overlap it, a capsule beside it, and a sphere, a box and a plane far away."""
    lo, hi = v.min(axis=0).astype(np.float64), v.max(axis=0).astype(np.float64)
    c, s = (lo + hi) / 2, hi - lo
    return f32_lists([[
        dict(kind="plane", a=(0.0, lo[1] + 0.02 * s[1], 0.0), b=(0.05, 1.0, -0.03), friction=0.3),
        dict(kind="sphere", a=(hi[0], c[1], c[2]), radius=0.25 * s[0], friction=0.2, velocity=(0.1, 0.0, 0.0)),
        dict(kind="box", a=(lo[0], c[1], c[2]), b=tuple(0.2 * s), axes=AXES, velocity=(0.0, 0.05, 0.0)),
        dict(kind="capsule", a=(c[0], hi[1] + 0.3, lo[2]), b=(c[0], hi[1] + 0.3, hi[2]), radius=0.1),
        dict(kind="sphere", a=(c[0], c[1] + 5.0, c[2]), radius=0.5),
        dict(kind="capsule", a=(lo[0], hi[1], c[2]), b=(hi[0], hi[1], c[2]), radius=0.05 * s[1], friction=0.1, velocity=(0.0, 0.0, 0.2)),
        dict(kind="box", a=(c[0] + 3.0, c[1] + 0.5, c[2] - 0.25), b=(0.25, 0.5, 0.125), axes=AXES),
        dict(kind="plane", a=(0.0, -5.0, 0.0), b=(0.0, 1.0, 0.0)),
    ]])[0]


def bits64(a):
    a = np.ascontiguousarray(a.detach().cpu().numpy() if isinstance(a, torch.Tensor) else a, dtype=np.float64).copy()
    a[np.isnan(a)] = np.nan
    return a.view(np.uint64)


def bits32(a):
    a = np.ascontiguousarray(a.detach().cpu().numpy() if isinstance(a, torch.Tensor) else a, dtype=np.float32).copy()
    a[np.isnan(a)] = np.nan
    return a.view(np.uint32)


def same(label, got, want, bits):
    got, want = (a.detach().cpu().numpy() if isinstance(a, torch.Tensor) else np.asarray(a) for a in (got, want))
    g, w = bits(got), bits(want)
    assert g.shape == w.shape, (label, g.shape, w.shape)
    if not np.array_equal(g, w):
        at = tuple(int(i[0]) for i in np.nonzero(g != w))
        raise AssertionError("%s: %d values differ, first at %s: got %r, reference %r" % (label, int((g != w).sum()), at, np.asarray(got)[at], np.asarray(want)[at]))


def f64_view(kind):
    return kind == "nh-precise-coloured"


def query(body, margin):
    """(body rows, particle rows) as numpy copies"""
    rows, prt = body.touchBodies(margin), body.touchParticlesDevice(margin)
    torch.cuda.synchronize()
    assert rows.dtype == torch.float64 and tuple(rows.shape) == (body.info.num_bodies, W)
    assert prt.dtype == torch.float32 and tuple(prt.shape) == (body.info.owned_particles, PW)
    return rows.cpu().numpy().copy(), prt.cpu().numpy().copy()


def check_reference(label, body, lists, first_vert, margin, rows, prt):
    pos, vel = body.pos, body.vel
    same(label + " body rows", rows, touch_ref.body_rows(pos, vel, lists, margin, first_vert), bits64)
    same(label + " particle rows", prt, touch_ref.all_particle_rows(pos, lists, margin, first_vert), bits32)


def slot_counts(rows):
    return rows[:, S0 + capi.TOUCH_SLOT_COUNT::SW]


# ---- 1. bit for bit, solo ----------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("kind", list(KINDS))
@pytest.mark.parametrize("mesh", ["lat4", "dragon"])
def test_solo_rows_equal_the_reference_bit_for_bit(mesh, kind):
    c = Case(mesh, kind)
    cols = scene8(c.rest)
    c.body.setColliders(cols)
    c.body.simulateSubsteps(40, DT, c.pp)
    assert np.isfinite(c.body.pos).all() and np.isfinite(c.body.vel).all()
    lists = [touch_ref.view(cols, f64_view(kind))]
    for margin in MARGINS:
        rows, prt = query(c.body, margin)
        check_reference("%s/%s margin %g" % (mesh, kind, margin), c.body, lists, None, margin, rows, prt)
        same("host twin", c.body.bodyTouch(margin), rows, bits64)
        counts = slot_counts(rows)[0]
        print("%s/%s margin %g: touching %d, counts %s, min sd %.3g in slot %d" % (mesh, kind, margin, rows[0, 0], counts.tolist(), rows[0, 1], rows[0, 2]))
        assert rows[0, capi.TOUCH_SLOTS] == 8
        assert [int(k) for k in rows[0, S0::SW]] == [3, 0, 2, 1, 0, 1, 2, 3]
        if margin == 1e-3:                                       # the test cannot pass on empty rows
            assert (counts > 0).any() and (counts == 0).any() and rows[0, 0] > 0
            assert counts[4] == 0 and counts[6] == 0 and counts[7] == 0
            assert (prt[:, capi.TOUCH_P_TOUCHES] > 0).sum() == rows[0, 0] and (prt[:, capi.TOUCH_P_SLOT] >= 0).all()


# ---- 2. batch and independence -----------------------------------------------------------------------------------------------------------
def batch_rows(c):
    """float32 [bodies, 8, 24]: body 0 no collider at all, body 1 eight rows of which two in the middle are empty, body 2 its scene with one
    row the table cannot hold (a negative radius)."""
    rows = body_collider_ref.rows([[], scene8(c.parts[1][0]), scene8(c.parts[2][0])], per_body=8)
    rows[1, 2, :] = 0.0
    rows[1, 2, 0] = -1.0
    rows[1, 5, 0] = -1.0
    rows[2, 1, 16] = -1.0
    return rows


@pytest.mark.parametrize("kind", list(KINDS))
@pytest.mark.parametrize("mesh", ["dragon3", "mixed"])
def test_a_body_of_a_batch_gives_the_bits_it_gives_alone(mesh, kind):
    c = Case(mesh, kind)
    rws = batch_rows(c)
    c.body.setBodyCollidersDevice(torch.from_numpy(rws).cuda())
    c.body.simulateSubsteps(10, DT, c.pp)
    cols = body_collider_ref.lists_from_rows(rws)
    assert [len(x) for x in cols] == [0, 6, 7]
    lists = [touch_ref.view(x, f64_view(kind)) for x in cols]
    margin = 1e-3
    rows, prt = query(c.body, margin)
    check_reference("%s/%s" % (mesh, kind), c.body, lists, c.first_vert, margin, rows, prt)
    assert rows[:, capi.TOUCH_SLOTS].tolist() == [0, 6, 7] and rows[0, capi.TOUCH_MIN_SLOT] == -1 and rows[0, capi.TOUCH_MIN_SD] == np.inf
    assert [int(k) for k in rows[1, S0::SW]] == [3, 0, 1, 0, 2, 3, -1, -1] and [int(k) for k in rows[2, S0::SW]] == [3, 2, 1, 0, 1, 2, 3, -1]
    assert (slot_counts(rows)[1:] > 0).any()
    pos, vel = c.body.pos, c.body.vel
    for b in range(3):
        solo = c.solo(b)
        lo, hi = int(c.first_vert[b]), int(c.first_vert[b + 1])
        solo.setColliders(cols[b])
        solo.writeState(pos[lo:hi], vel[lo:hi])
        assert np.array_equal(f32bits(solo.pos), f32bits(pos[lo:hi])) and np.array_equal(f32bits(solo.vel), f32bits(vel[lo:hi]))
        alone, alone_prt = query(solo, margin)
        same("body %d alone" % b, alone[0], rows[b], bits64)
        same("body %d alone, particles" % b, alone_prt, prt[lo:hi], bits32)


# ---- 3. physics sanity -------------------------------------------------------------------------------------------------------------------
def test_a_dropped_lattice_touches_the_plane_it_comes_to_rest_on():
    v, t = load_mesh("lat4")
    body = SoftBodyHIP(v, t, None, dict(PP), solver="polar", precision="fast")
    height = float(np.float32(v[:, 1].min() - np.float32(0.03125)))   # (above the solver's own floor at y = 0)
    assert height > 0.01
    body.setColliders([dict(kind="plane", a=(0.0, height, 0.0), b=(0.0, 1.0, 0.0), friction=0.5)])
    margin = 1e-3
    before = body.bodyTouch(margin)[0]
    assert before[capi.TOUCH_TOUCHING] == 0 and before[S0 + capi.TOUCH_SLOT_COUNT] == 0 and before[capi.TOUCH_MIN_SLOT] == 0
    assert before[capi.TOUCH_MIN_SD] == float(v[:, 1].min()) - height and not before[S0 + 3:S0 + SW].any()   # (one exact f64 subtraction)
    body.simulateSubsteps(1500, DT, PP)
    row = body.bodyTouch(margin)[0]
    slot = row[S0:S0 + SW]
    print("at rest: touching %d, min sd %.3g, centroid %s, rel vel %s" % (row[0], row[1], slot[3:6], slot[9:12]))
    assert row[capi.TOUCH_TOUCHING] > 0 and slot[capi.TOUCH_SLOT_COUNT] == row[capi.TOUCH_TOUCHING] and slot[capi.TOUCH_SLOT_KIND] == 3
    assert np.array_equal(bits64(slot[6:9]), bits64(np.array([0.0, 1.0, 0.0])))
    assert abs(slot[capi.TOUCH_SLOT_CENTROID + 1] - height) < margin
    assert np.abs(slot[9:12]).max() < 0.5                        # at rest, not in free fall (1.25 s of which is 12 m/s)


# ---- 4. edge rows ------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("kind", ["polar-fast", "nh-precise-coloured"])
def test_a_nan_particle_touches_nothing_and_disturbs_no_other_body(kind):
    c = Case("mixed", kind)
    cols = scene8(c.parts[1][0])
    c.body.setColliders(cols)
    c.body.simulateSubsteps(5, DT, c.pp)
    margin = 1e-3
    before, before_prt = query(c.body, margin)
    t = c.body.exportTensors(("pos", "vel"))
    pos, vel = t["pos"].clone(), t["vel"].clone()
    at = int(c.first_vert[1]) + 77
    pos[at, 1] = float("nan")
    c.body.importTensors(pos, vel)
    rows, prt = query(c.body, margin)
    assert prt[at].tolist() == [np.inf, 0.0, 0.0, 0.0, -1.0, 0.0, 0.0, 0.0]
    same("the other bodies", rows[[0, 2]], before[[0, 2]], bits64)
    keep = np.arange(len(prt)) != at
    same("the other particles", prt[keep], before_prt[keep], bits32)
    assert rows[1, 0] == before[1, 0] - (before_prt[at, capi.TOUCH_P_TOUCHES] > 0) and np.isfinite(rows[1, :4]).all()
    check_reference("nan/" + kind, c.body, [touch_ref.view(cols, f64_view(kind))] * 3, c.first_vert, margin, rows, prt)


@pytest.mark.parametrize("kind", ["polar-precise", "nh-precise-coloured"])
def test_a_particle_at_a_spheres_centre_and_a_handle_without_colliders(kind):
    c = Case("lat4", kind)
    rows, prt = query(c.body, 0.5)                               # no colliders at all
    assert rows[0, :4].tolist() == [0.0, np.inf, -1.0, 0.0] and (rows[0, S0::SW] == -1).all() and (rows[0, S0 + 2::SW] == np.inf).all()
    assert not np.delete(rows[0], np.concatenate([[1, 2], np.arange(S0, W, SW), np.arange(S0 + 2, W, SW)])).any()
    assert (prt[:, 0] == np.inf).all() and (prt[:, 4] == -1).all() and not prt[:, [1, 2, 3, 5, 6, 7]].any()
    check_reference("none/" + kind, c.body, [[]], None, 0.5, rows, prt)
    centre = np.array([0.3125, 0.5625, -0.1875], np.float32)
    cols = [dict(kind="sphere", a=centre.astype(np.float64).tolist(), radius=0.25)]
    pos = c.rest.copy()
    pos[60] = centre
    c.body.writeState(pos, np.zeros_like(pos))
    c.body.setColliders(cols)
    rows, prt = query(c.body, 0.0)
    assert prt[60].tolist() == [-0.25, 0.0, 0.0, 0.0, 0.0, 1.0, 0.0, 0.0] and rows[0, capi.TOUCH_MIN_SD] == -0.25 and rows[0, capi.TOUCH_MIN_SLOT] == 0
    assert rows[0, capi.TOUCH_TOUCHING] >= 1
    check_reference("centre/" + kind, c.body, [touch_ref.view(cols, f64_view(kind))], None, 0.0, rows, prt)


# ---- 5. surroundings ---------------------------------------------------------------------------------------------------------------------
def sentinel64(rows, width):
    return torch.full((rows, width), SENT64, dtype=torch.int64, device="cuda").view(torch.float64)


def sentinel32(rows, width):
    return torch.full((rows, width), SENT32, dtype=torch.int32, device="cuda").view(torch.float32)


def is_sentinel(t):
    if t.dtype == torch.float64:
        return bool((t.contiguous().view(torch.int64) == SENT64).all())
    return bool((t.contiguous().view(torch.int32) == SENT32).all())


@pytest.mark.parametrize("kind", ["polar-fast", "nh-precise-coloured"])
def test_strided_rows_two_calls_a_side_stream_and_an_untouched_state(kind):
    c = Case("dragon3", kind)
    c.body.setColliders(scene8(c.parts[1][0]))
    c.body.simulateSubsteps(10, DT, c.pp)
    blob = c.body.saveState()
    d0 = device_bytes(c.body)
    margin = 1e-3
    rows, prt = query(c.body, margin)
    d1 = device_bytes(c.body)
    chunks = sum(-(-len(v) // 256) for v, _ in c.parts)
    assert d1 >= d0 + 8 * 90 * chunks + 8 * W * 3                # the chunk rows and the rows of the host read
    again, again_prt = query(c.body, margin)
    same("again", again, rows, bits64)
    same("again, particles", again_prt, prt, bits32)
    n = c.body.info.owned_particles
    side = torch.cuda.Stream()
    with torch.cuda.stream(side):                                # enqueued and consumed on a side stream, no host wait in between
        buf = sentinel64(3 + 2, 128)
        view = buf[1:-1, :W]
        pbuf = sentinel32(n + 2, 12)
        pview = pbuf[1:-1, :PW]
        assert c.body.touchBodies(margin, out=view, stream=side) is view
        assert c.body.touchParticlesDevice(margin, out=pview, stream=side) is pview
        total, ptotal = view.clone(), pview.clone()
    torch.cuda.synchronize()
    same("strided", total, rows, bits64)
    same("strided, particles", ptotal, prt, bits32)
    assert is_sentinel(buf[0]) and is_sentinel(buf[-1]) and is_sentinel(buf[1:-1, W:])
    assert is_sentinel(pbuf[0]) and is_sentinel(pbuf[-1]) and is_sentinel(pbuf[1:-1, PW:])
    same("host twin", c.body.bodyTouch(margin), rows, bits64)
    assert c.body.touchBodies(margin) is c.body.touchBodies(margin)   # allocated once, reused
    assert device_bytes(c.body) == d1
    assert c.body.saveState() == blob                            # read-only


# ---- 6. errors ---------------------------------------------------------------------------------------------------------------------------
def test_refusals_leave_dst_alone():
    L = capi.lib()
    c = Case("dragon3", "polar-fast")
    c.body.setColliders(scene8(c.parts[1][0]))
    h, nb, n = c.body._h, 3, c.body.info.owned_particles
    dst, pdst = sentinel64(nb + 1, W), sentinel32(n + 1, PW)
    p, pp = dst.data_ptr(), pdst.data_ptr()
    host = np.full(nb * W, np.nan)
    hip = _hip_runtime()
    short = C.c_void_p()
    assert hip.hipMalloc(C.byref(short), C.c_size_t(nb * 8 * W - 8)) == 0          # an allocation of its own, one double too short
    assert hip.hipMemset(short, 0xA5, C.c_size_t(nb * 8 * W - 8)) == 0
    d0 = device_bytes(c.body)
    for margin, ptr, stride, text in ((np.nan, p, 0, "margin"), (np.inf, p, 0, "margin"), (-np.inf, p, 0, "margin"), (0.0, None, 0, "null"),
                                      (0.0, p + 4, 0, "aligned"), (0.0, p, 8, "row_stride"), (0.0, p, 792, "row_stride"), (0.0, p, 804, "row_stride"),
                                      (0.0, host.ctypes.data, 0, "not device memory"), (0.0, short.value, 0, "do not fit")):
        rc = L.tetsim_touch_bodies_device(h, margin, ptr, stride, None)
        assert rc == capi.EINVAL and text.encode() in L.tetsim_last_error(h), (margin, ptr, stride, rc, L.tetsim_last_error(h))
    for margin, ptr, stride, text in ((np.nan, pp, 0, "margin"), (0.0, None, 0, "null"), (0.0, pp + 2, 0, "aligned"), (0.0, pp, 16, "row_stride"),
                                      (0.0, pp, 34, "row_stride"), (0.0, host.ctypes.data, 0, "not device memory"), (0.0, short.value, 0, "do not fit")):
        rc = L.tetsim_touch_particles_device(h, margin, ptr, stride, None)
        assert rc == capi.EINVAL and text.encode() in L.tetsim_last_error(h), (margin, ptr, stride, rc, L.tetsim_last_error(h))
    assert L.tetsim_read_body_touch(h, 0.0, None) == capi.EINVAL
    assert L.tetsim_read_body_touch(h, np.nan, host.ctypes.data_as(C.POINTER(C.c_double))) == capi.EINVAL
    assert L.tetsim_touch_bodies_device(None, 0.0, p, 0, None) == capi.EINVAL
    torch.cuda.synchronize()
    assert is_sentinel(dst) and is_sentinel(pdst) and np.isnan(host).all() and device_bytes(c.body) == d0   # (not even the scratch was made)
    back = np.zeros(nb * 8 * W - 8, np.uint8)
    assert hip.hipMemcpy(C.c_void_p(back.ctypes.data), short, C.c_size_t(back.size), 2) == 0 and (back == 0xA5).all()
    assert hip.hipFree(short) == 0
    for bad in (dst[:nb].float(), dst[:nb - 1], dst[:nb, :W - 1], torch.zeros((nb, W), dtype=torch.float64)):
        with pytest.raises(ValueError):
            c.body.touchBodies(0.0, out=bad)
    for bad in (pdst[:n].double(), pdst[:n - 1], pdst[:n, :PW - 1], torch.zeros((n, PW), dtype=torch.float32)):
        with pytest.raises(ValueError):
            c.body.touchParticlesDevice(0.0, out=bad)
    assert is_sentinel(dst) and is_sentinel(pdst)
    got = c.body.touchBodies(1e-3, out=dst[:nb])                 # ... and the next good call is right
    torch.cuda.synchronize()
    same("after the refusals", got, c.body.bodyTouch(1e-3), bits64)
    assert is_sentinel(dst[nb:])


def test_a_partitioned_body_is_refused():
    v, t = load_mesh("lat4")
    parts = [SoftBodyHIP(v, t, None, dict(PP), solver="polar", precision="fast", part_count=2, part_index=i) for i in range(2)]
    for part in parts:
        dst, pdst = sentinel64(1, W), sentinel32(part.info.owned_particles, PW)
        for call in (lambda: part.touchBodies(0.0, out=dst), lambda: part.bodyTouch(0.0), lambda: part.touchParticlesDevice(0.0, out=pdst)):
            with pytest.raises(TetSimError) as e:
                call()
            assert e.value.code == capi.ESTATE and "partitioned" in str(e.value)
        torch.cuda.synchronize()
        assert is_sentinel(dst) and is_sentinel(pdst)
