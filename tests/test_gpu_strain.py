"""Per-tet strain on the device (include/tetsim.h: tetsim_tet_strain_device / tetsim_read_tet_strain / tetsim_body_strain_device /
tetsim_visual_strain_device; SoftBodyHIP.tetStrainDevice / tetStrain / bodyStrainDevice / visualStrainDevice) against tests/strain_ref.py.

The header defines every value as f64 arithmetic with only + - * / sqrt, each operation rounded once, in a fixed order; numpy evaluates
the same expressions in the same order (strain_ref.py), so the comparison is BIT FOR BIT: rows as uint32, body rows as uint64.  The
reference's invRestPose is the library's own host preprocessing (tetsim_prep_rest), the positions are what the body's host read returns.

Shapes: the 3 x 3 x 3-cell lattice (162 tets: one partial chunk), the 4 x 4 x 4-cell lattice (384 tets: two chunks, the second partial)
and a single tet."""
import ctypes as C

import numpy as np
import pytest
import torch

import strain_ref as R
from test_gpu_device_io import DT, KINDS, PP, WIDE
from test_gpu_snapshot import _hip_runtime, device_bytes
from test_strain_cpu import prep_rest
from tetsim_amd import SoftBodyHIP, TetSimError, boundary_surface, make_lattice
from tetsim_amd import _capi as capi

pytestmark = pytest.mark.gpu
W, BW = capi.STRAIN_WIDTH, capi.STRAIN_BODY_WIDTH
SENTINEL32, SENTINEL64 = 0x7FC0DEAD, 0x7FF8DEADDEADDEAD   # NaN payloads no kernel produces
ONE_TET = (np.array([[0, 0.5, 0], [0.5, 0.5, 0], [0, 1.0, 0], [0, 0.5, 0.5]], np.float32), np.array([[0, 1, 2, 3]], np.int32))


def u32(a):
    if isinstance(a, torch.Tensor):
        a = a.detach().cpu().numpy()
    return np.ascontiguousarray(a, dtype=np.float32).view(np.uint32)


def u64(a):
    if isinstance(a, torch.Tensor):
        a = a.detach().cpu().numpy()
    return np.ascontiguousarray(a, dtype=np.float64).view(np.uint64)


def reference(verts, tets, pos, first_tet=None):
    """(tet rows f32 [nt, 16], body rows f64 [bodies, 8]) of strain_ref for the rest mesh and the positions."""
    _, irp, _ = prep_rest(verts, tets, PP["density"])
    deg = R.degenerate_tets(verts, tets, irp)
    val = R.tet_values(pos, tets, irp)
    rows = R.tet_rows(val, deg)
    return rows, R.body_rows(val, rows, R.rest_volume(verts, tets), deg, first_tet)


def pulled(v, t, kind, params=PP):
    """The lattice with one corner particle grabbed and pulled away for 5 substeps."""
    body = SoftBodyHIP(v, t, None, dict(params), **KINDS[kind])
    corner = v[-1].astype(np.float32)
    body.startGrab(corner)
    body.moveGrabbed(corner + np.array([0.2, 0.15, 0.1], np.float32))
    body.simulateSubsteps(5, DT, params)
    return body


# ---- 1. bit equality with the reference ----------------------------------------------------------------------------------------------
@pytest.mark.parametrize("kind", list(KINDS))
def test_rows_equal_the_reference_bit_for_bit(kind):
    v, t = make_lattice(3)
    assert len(t) == 162
    body = pulled(v, t, kind)
    dev = body.tetStrainDevice()
    brow = body.bodyStrainDevice()
    torch.cuda.synchronize()
    assert dev.dtype == torch.float32 and dev.is_cuda and tuple(dev.shape) == (162, W) and tuple(brow.shape) == (1, BW) and brow.dtype == torch.float64
    pos = body.pos
    assert np.isfinite(pos).all() and np.abs(pos - v).max() > 1e-3
    rows, want_body = reference(v, t, pos)
    got = dev.cpu().numpy()
    print("%s: J in [%.6f, %.6f], largest stretch %.6f, max GREEN %.6f" % (kind, got[:, R.J_AT].min(), got[:, R.J_AT].max(), got[:, R.STRETCH_AT].max(), got[:, R.GREEN_AT].max()))
    assert np.array_equal(u32(got), u32(rows))
    assert got[:, R.GREEN_AT].max() > 1e-4 and np.isfinite(got).all() and (got[:, R.RESERVED_AT] == 0).all()
    assert np.array_equal(u64(brow), u64(want_body))
    assert np.array_equal(u32(body.tetStrain()), u32(rows))          # the host reader equals the device call
    assert body.tetStrainDevice() is dev                              # allocated once, reused


# ---- 2. chunk boundaries in a batch --------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("kind", ["polar-fast", "nh-fast"])
def test_a_body_of_a_batch_gives_the_bits_it_gives_alone(kind):
    parts = [ONE_TET, make_lattice(4), make_lattice(3)]
    shifts = ([-3.0, 0.0, 0.0], [0.0, 0.0, 0.0], [3.0, 0.0, 0.5])
    parts = [((v + np.array(s, np.float32)).astype(np.float32), t) for (v, t), s in zip(parts, shifts)]
    assert [len(t) for _, t in parts] == [1, 384, 162]
    batch = SoftBodyHIP.batch(parts, dict(WIDE), ref_fixed_bounds=False, **KINDS[kind])
    first_vert = np.concatenate([[0], np.cumsum([len(v) for v, _ in parts])])
    first_tet = np.concatenate([[0], np.cumsum([len(t) for _, t in parts])])
    rest = np.concatenate([v for v, _ in parts])
    tets = np.concatenate([t + int(o) for (_, t), o in zip(parts, first_vert)])
    rng = np.random.default_rng(5)
    pos = rest.copy()
    for b, amp in enumerate((0.02, 0.01, 0.02)):                       # every body in a state of its own
        lo, hi = first_vert[b], first_vert[b + 1]
        pos[lo:hi] = (pos[lo:hi] * np.float32(1.0 + 0.1 * b) + rng.normal(0.0, amp, (hi - lo, 3))).astype(np.float32)
    batch.writeState(pos, np.zeros_like(pos))
    batch.simulateSubsteps(3, DT, WIDE)
    rows, brow = batch.tetStrainDevice().cpu().numpy(), batch.bodyStrainDevice().cpu().numpy()
    again, bagain = batch.tetStrainDevice().cpu().numpy(), batch.bodyStrainDevice().cpu().numpy()
    assert np.array_equal(u32(rows), u32(again)) and np.array_equal(u64(brow), u64(bagain))
    now, vel = batch.pos, batch.vel
    want_rows, want_body = reference(rest, tets, now, first_tet)
    assert np.array_equal(u32(rows), u32(want_rows)) and np.array_equal(u64(brow), u64(want_body))
    assert (brow[:, 7] == 0).all() and np.isfinite(brow).all() and (brow[:, 0] >= brow[:, 1]).all()
    for b, (v, t) in enumerate(parts):
        solo = SoftBodyHIP(v, t, None, dict(WIDE), ref_fixed_bounds=False, **KINDS[kind])
        lo, hi = int(first_vert[b]), int(first_vert[b + 1])
        solo.writeState(now[lo:hi], vel[lo:hi])
        assert np.array_equal(u32(solo.pos), u32(now[lo:hi]))
        assert np.array_equal(u32(solo.tetStrainDevice()), u32(rows[first_tet[b]:first_tet[b + 1]])), (kind, b)
        assert np.array_equal(u64(solo.bodyStrainDevice()), u64(brow[b:b + 1])), (kind, b)


# ---- 3. degenerate and non-finite input ----------------------------------------------------------------------------------------------
@pytest.mark.parametrize("kind", ["nh-precise-coloured", "nh-fast"])
def test_a_flat_tet_and_a_nan_particle_poison_their_own_rows_only(kind):
    v, t = make_lattice(3)
    flat = np.array([[0, 1, 4, 5]], np.int32)                         # four corners of one cell face: volume 0 exactly
    td = np.concatenate([flat, t])                                    # (first: the reference's clearing of a singular invRestPose
    _, irp, _ = prep_rest(v, td)                                      # hits entries e .. e + 8 of the whole array, here its own)
    assert R.rest_volume(v, td)[0] == 0 and np.array_equal(irp[1:], prep_rest(v, t)[1])
    body, plain = SoftBodyHIP(v, td, None, dict(PP), **KINDS[kind]), SoftBodyHIP(v, t, None, dict(PP), **KINDS[kind])
    pos = (v * np.array([1.25, 1.0, 0.9], np.float32)).astype(np.float32)
    for x in (body, plain):
        x.writeState(pos, np.zeros_like(pos))
    rows, brow = body.tetStrainDevice().cpu().numpy(), body.bodyStrainDevice().cpu().numpy()
    want_rows, want_body = reference(v, td, pos)
    assert np.array_equal(u32(rows), u32(want_rows)) and np.array_equal(u64(brow), u64(want_body))
    assert np.isnan(rows[0, :15]).all() and rows[0, 15] == 0 and brow[0, 7] == 1 and np.isfinite(brow).all()
    assert np.array_equal(u32(rows[1:]), u32(plain.tetStrainDevice()))   # the other rows: as without the flat tet
    assert np.array_equal(u64(brow[:, :7]), u64(plain.bodyStrainDevice().cpu().numpy()[:, :7]))
    # a NaN particle, through the device import
    p = int(t[40, 2])
    bad = pos.copy()
    bad[p] = np.nan
    dp, dv = torch.from_numpy(bad).cuda(), torch.zeros(bad.shape, dtype=torch.float32, device="cuda")
    body.importTensors(dp, dv)
    rows, brow = body.tetStrainDevice().cpu().numpy(), body.bodyStrainDevice().cpu().numpy()
    hit = (td == p).any(axis=1)
    hit[0] = False
    assert 0 < hit.sum() < len(td) - 1
    assert np.isnan(rows[hit][:, [R.J_AT, R.DEV_AT, R.GREEN_AT]]).all() and np.isfinite(rows[~hit][1:]).all()
    assert np.array_equal(u32(rows[~hit]), u32(want_rows[~hit])) and brow[0, 7] == 1 + hit.sum()
    want_rows, want_body = reference(v, td, bad)                     # (which NaN an operation returns is the processor's choice: compared as NaN)
    assert np.array_equal(np.isnan(rows), np.isnan(want_rows)) and np.array_equal(u32(np.nan_to_num(rows)), u32(np.nan_to_num(want_rows)))
    assert np.array_equal(u64(brow), u64(want_body))


# ---- 4. strides and refused calls ----------------------------------------------------------------------------------------------------
def is_sentinel(t, value):
    kind = torch.int32 if value == SENTINEL32 else torch.int64
    return bool((t.contiguous().view(kind) == value).all())


@pytest.mark.parametrize("kind", ["polar-fast", "nh-fast"])
def test_strided_rows_leave_padding_and_guard_rows_alone(kind):
    v, t = make_lattice(3)
    body = pulled(v, t, kind)
    nt = len(t)
    packed, bpacked = body.tetStrainDevice().clone(), body.bodyStrainDevice().clone()
    buf = torch.full((nt + 2, 20), SENTINEL32, dtype=torch.int32, device="cuda").view(torch.float32)   # rows 80 bytes apart, a guard row each side
    view = buf[1:-1, :W]
    assert view.stride(0) * 4 == 80
    assert body.tetStrainDevice(out=view) is view
    bbuf = torch.full((1 + 2, 9), SENTINEL64, dtype=torch.int64, device="cuda").view(torch.float64)    # body rows 72 bytes apart
    bview = bbuf[1:-1, :BW]
    assert bview.stride(0) * 8 == 72
    body.bodyStrainDevice(out=bview)
    flat = torch.full(((nt + 1) * W + 1,), SENTINEL32, dtype=torch.int32, device="cuda").view(torch.float32)
    off = flat[1:1 + nt * W].view(nt, W)                              # packed rows at a dst that is only 4-byte aligned
    assert off.data_ptr() % 16 == 4
    body.tetStrainDevice(out=off)
    torch.cuda.synchronize()
    assert np.array_equal(u32(view), u32(packed)) and np.array_equal(u32(off), u32(packed)) and np.array_equal(u64(bview), u64(bpacked))
    assert is_sentinel(buf[0], SENTINEL32) and is_sentinel(buf[-1], SENTINEL32) and is_sentinel(buf[1:-1, W:], SENTINEL32)
    assert is_sentinel(bbuf[0], SENTINEL64) and is_sentinel(bbuf[-1], SENTINEL64) and is_sentinel(bbuf[1:-1, BW:], SENTINEL64)
    assert is_sentinel(flat[:1], SENTINEL32) and is_sentinel(flat[1 + nt * W:], SENTINEL32)


@pytest.mark.parametrize("kind", ["polar-fast", "nh-fast"])
def test_refusals_leave_dst_alone(kind):
    L = capi.lib()
    v, t = make_lattice(3)
    body = pulled(v, t, kind)
    h, nt = body._h, len(t)
    dst = torch.full((nt + 1, W), SENTINEL32, dtype=torch.int32, device="cuda").view(torch.float32)
    bdst = torch.full((2, BW), SENTINEL64, dtype=torch.int64, device="cuda").view(torch.float64)
    p, bp = dst.data_ptr(), bdst.data_ptr()
    host = np.full(nt * W, np.nan, np.float32)
    hip = _hip_runtime()
    short = C.c_void_p()
    assert hip.hipMalloc(C.byref(short), C.c_size_t(nt * 64 - 4)) == 0            # an allocation of its own, one float too short
    assert hip.hipMemset(short, 0xA5, C.c_size_t(nt * 64 - 4)) == 0
    d0 = device_bytes(body)
    for fn, args, text in ((L.tetsim_tet_strain_device, (None, 0), "null"), (L.tetsim_tet_strain_device, (p + 2, 0), "aligned"),
                           (L.tetsim_tet_strain_device, (p, 60), "row_stride"), (L.tetsim_tet_strain_device, (p, 66), "row_stride"),
                           (L.tetsim_tet_strain_device, (host.ctypes.data, 0), "not device memory"), (L.tetsim_tet_strain_device, (short.value, 0), "do not fit"),
                           (L.tetsim_body_strain_device, (None, 0), "null"), (L.tetsim_body_strain_device, (bp + 4, 0), "aligned"),
                           (L.tetsim_body_strain_device, (bp, 68), "row_stride"), (L.tetsim_body_strain_device, (bp, 56), "row_stride"),
                           (L.tetsim_body_strain_device, (host.ctypes.data, 0), "not device memory")):
        rc = fn(h, args[0], args[1], None)
        assert rc == capi.EINVAL, (args, rc, L.tetsim_last_error(h))
        assert text.encode() in L.tetsim_last_error(h), (args, L.tetsim_last_error(h))
    assert L.tetsim_read_tet_strain(h, None) == capi.EINVAL
    assert L.tetsim_visual_strain_device(h, 0, p, 0, None) == capi.ESTATE and b"no visual mesh" in L.tetsim_last_error(h)
    torch.cuda.synchronize()
    assert is_sentinel(dst, SENTINEL32) and is_sentinel(bdst, SENTINEL64) and np.isnan(host).all() and device_bytes(body) == d0   # (not even the tables were made)
    back = np.zeros(nt * 64 - 4, np.uint8)
    assert hip.hipMemcpy(C.c_void_p(back.ctypes.data), short, C.c_size_t(back.size), 2) == 0 and (back == 0xA5).all()
    assert hip.hipFree(short) == 0
    for bad in (dst[:nt].double(), dst[:nt - 1], dst[:nt, :W - 1], torch.zeros((nt, W), dtype=torch.float32)):
        with pytest.raises(ValueError):
            body.tetStrainDevice(out=bad)
    with pytest.raises(ValueError):
        body.bodyStrainDevice(out=bdst[:1].float())
    assert is_sentinel(dst, SENTINEL32)
    got = body.tetStrainDevice(out=dst[:nt])                           # ... and the next good call is right
    torch.cuda.synchronize()
    assert np.array_equal(u32(got), u32(reference(v, t, body.pos)[0])) and is_sentinel(dst[nt:], SENTINEL32)
    d1 = device_bytes(body)
    assert d1 >= d0 + 64 * nt + 64 * nt + 64                           # the table, the rows of the host read, a partial row
    body.bodyStrainDevice()
    body.tetStrain()
    assert device_bytes(body) == d1                                    # the first call alone allocates


def test_a_partitioned_body_is_refused():
    v, t = make_lattice(3)
    for i in range(2):
        part = SoftBodyHIP(v, t, None, dict(PP), solver="polar", precision="fast", part_count=2, part_index=i)
        dst = torch.full((len(t), W), SENTINEL32, dtype=torch.int32, device="cuda").view(torch.float32)
        bdst = torch.full((1, BW), SENTINEL64, dtype=torch.int64, device="cuda").view(torch.float64)
        for call in (lambda: part.tetStrainDevice(out=dst), part.tetStrain, lambda: part.bodyStrainDevice(out=bdst)):
            with pytest.raises(TetSimError) as e:
                call()
            assert e.value.code == capi.ESTATE and "partitioned" in str(e.value)
        torch.cuda.synchronize()
        assert is_sentinel(dst, SENTINEL32) and is_sentinel(bdst, SENTINEL64)


# ---- 5. stream ordering --------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("kind", ["polar-fast", "nh-fast"])
def test_a_side_stream_sees_the_rows_without_a_synchronisation(kind):
    v, t = make_lattice(3)
    body = pulled(v, t, kind)
    out = torch.empty((len(t), W), dtype=torch.float32, device="cuda")
    bout = torch.empty((1, BW), dtype=torch.float64, device="cuda")
    stream = torch.cuda.Stream()
    with torch.cuda.stream(stream):
        out.fill_(float("nan"))                                        # still running, on this stream, when the call is made
        bout.fill_(float("nan"))
        body.simulateSubsteps(5, DT, PP)
        body.tetStrainDevice(out=out, stream=stream)
        body.bodyStrainDevice(out=bout, stream=stream)
        kept, bkept = out.clone(), bout.clone()                        # read on that stream, in stream order
        body.simulateSubsteps(5, DT, PP)                               # later substeps do not disturb what was handed over
        host, bhost = kept.cpu().numpy(), bkept.cpu().numpy()
    twin = pulled(v, t, kind)
    twin.simulateSubsteps(5, DT, PP)
    rows, brow = reference(v, t, twin.pos)
    assert np.array_equal(u32(host), u32(rows)) and np.array_equal(u64(bhost), u64(brow))


# ---- 6. visual strain ----------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("kind", ["polar-fast", "nh-fast"])
def test_visual_strain_is_the_tet_rows_gathered_by_tet_number(kind):
    v, t = make_lattice(3)
    body = pulled(v, t, kind)
    vis, tris = boundary_surface(t, len(v), v)
    body.setVisualMesh(vis)
    body.setVisualTriangles(tris)
    rows = body.tetStrainDevice().cpu().numpy()
    tet_nr = vis[:, 0].astype(np.int64)
    assert len(vis) == body.info.num_vis_verts > 0 and len(np.unique(tet_nr)) > 10
    for channel, at in (("green", R.GREEN_AT), ("J", R.J_AT), ("stretch0", R.STRETCH_AT), (13, 13), ("F01", 3), (0, 0)):
        got = body.visualStrainDevice(channel)
        assert got.dtype == torch.float32 and tuple(got.shape) == (len(vis),)
        assert np.array_equal(u32(got), u32(rows[tet_nr, at])), channel
    wide = torch.full((len(vis) + 2, 3), SENTINEL32, dtype=torch.int32, device="cuda").view(torch.float32)
    body.visualStrainDevice("dev", out=wide[1:-1, 1])                  # one float every 12 bytes
    torch.cuda.synchronize()
    assert np.array_equal(u32(wide[1:-1, 1]), u32(rows[tet_nr, R.DEV_AT]))
    assert is_sentinel(wide[0], SENTINEL32) and is_sentinel(wide[-1], SENTINEL32) and is_sentinel(wide[1:-1, [0, 2]], SENTINEL32)
    for bad in (15, -1):
        with pytest.raises(TetSimError) as e:
            body.visualStrainDevice(bad)
        assert e.value.code == capi.EINVAL and "channel" in str(e.value)
    with pytest.raises(ValueError):
        body.visualStrainDevice("pressure")
