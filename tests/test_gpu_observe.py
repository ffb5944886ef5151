"""Per-body observations on the device (include/tetsim.h: tetsim_observe_bodies_device / tetsim_read_body_observations;
SoftBodyHIP.observeBodies / bodyObservations) against the exact reference of tests/observe_ref.py.

THE BOUND.  The kernel evaluates the header's definitions in f64, every operation rounded once (unit roundoff 2^-53), and adds a body's
terms up in a fixed tree.  The reference evaluates the same expressions over Fractions of the same f32 state, without any rounding, and
returns S: the sum of the absolute values of all products that enter a value once its differences and sums are multiplied out.  A value
computed with c roundings on its longest path, terms added in any order, is within c * 2^-53 * S of the exact one (every multiplied-out
product carries at most c factors (1 + d), |d| <= 2^-53).  observe_ref.bounds counts c per quantity -- the roundings the header's
expression has on its longest path, plus the body's tet count for the sums (a generous stand-in for the tree's depth), plus the division
for the quotients -- and this test allows exactly that: nothing here was measured on a GPU first, nothing is in tolerances.json.
The box, max_speed2 and the two counts must equal the reference bit for bit: minima and maxima do not depend on the order, squares of f32
values are exact in f64 and the two sums of max_speed2 are rounded the way Python rounds them, and a count is a count (the inverted tets
are compared where no tet's |V/V0| is below 1e-6, i.e. where no sign can depend on a rounding; asserted).

Bodies: the five kinds of tests/test_gpu_device_io.py.  Meshes: its three (the Dragon: 3,840 tets = 15 chunks, internal particle order;
lat4: one partial chunk; dragon3: body boundaries that are no multiple of 256 in the concatenation), a mixed batch lat4 + Dragon + lat4,
and the hub mesh (valence 44)."""
import ctypes as C
from fractions import Fraction

import numpy as np
import pytest
import torch

from conftest import load_mesh
import observe_ref
from test_gpu_device_io import DT, KINDS, PP, WIDE
from test_gpu_snapshot import _hip_runtime, device_bytes
from tetsim_amd import SoftBodyHIP, TetSimError
from tetsim_amd import _capi as capi

pytestmark = pytest.mark.gpu
MESHES = ["dragon", "lat4", "dragon3", "mixed", "hub"]
SHIFTS = [np.array(s, np.float32) for s in ([-3.0, 0.0, 0.0], [0.0, 0.0, 0.0], [3.0, 0.0, 0.5])]
SENTINEL = 0x7FF8DEADDEADDEAD   # a NaN payload no kernel produces
W = capi.OBS_WIDTH
SUMS = ("mass", "volume", "rest_volume", "min_volume_ratio")
EXACT = ((capi.OBS_AABB_MIN, "aabb_min"), (capi.OBS_AABB_MAX, "aabb_max"), (capi.OBS_MAX_SPEED2, "max_speed2"), (capi.OBS_NONFINITE, "nonfinite"))
AT = dict(mass=capi.OBS_MASS, volume=capi.OBS_VOLUME, rest_volume=capi.OBS_REST_VOLUME, min_volume_ratio=capi.OBS_MIN_VOLUME_RATIO,
          com=capi.OBS_COM, vcom=capi.OBS_VCOM)


def parts_of(mesh):
    """[(vertices, tets)] of the mesh's bodies; the bodies of a batch are shifted apart in x."""
    if mesh == "dragon3":
        names = ["dragon"] * 3
    elif mesh == "mixed":
        names = ["lat4", "dragon", "lat4"]
    else:
        return [load_mesh(mesh)]
    return [((v + s).astype(np.float32), t) for (v, t), s in zip(map(load_mesh, names), SHIFTS)]


class Case:
    """A body of `kind` over `mesh`, with what the reference needs: the rest positions, the tets and the ranges of the concatenation."""

    def __init__(self, mesh, kind):
        self.parts = parts_of(mesh)
        self.kw = KINDS[kind]
        if len(self.parts) == 1:
            self.pp = PP
            self.body = SoftBodyHIP(self.parts[0][0], self.parts[0][1], None, dict(PP), **self.kw)
        else:
            self.pp = WIDE
            self.body = SoftBodyHIP.batch(self.parts, dict(WIDE), ref_fixed_bounds=False, **self.kw)
        self.first_vert = np.concatenate([[0], np.cumsum([len(v) for v, _ in self.parts])])
        self.first_tet = np.concatenate([[0], np.cumsum([len(t) for _, t in self.parts])])
        self.rest = np.concatenate([v for v, _ in self.parts])
        self.tets = np.concatenate([t + int(o) for (_, t), o in zip(self.parts, self.first_vert)])
        assert [(tuple(map(int, a)), tuple(map(int, b))) for a, b in self.body.bodyRanges] == \
            [((int(self.first_vert[b]), int(self.first_vert[b + 1])), (int(self.first_tet[b]), int(self.first_tet[b + 1]))) for b in range(len(self.parts))]

    def reference(self, pos, vel):
        return observe_ref.observe(self.rest, self.tets, pos, vel, PP["density"], self.first_vert, self.first_tet)

    def solo(self, b):
        """Body b of the batch on its own, built from the shifted vertices."""
        return SoftBodyHIP(self.parts[b][0], self.parts[b][1], None, dict(WIDE), ref_fixed_bounds=False, **self.kw)


def rows_of(t):
    return t.detach().cpu().numpy().astype(np.float64).reshape(-1, W).copy()


def bits(a):
    if isinstance(a, torch.Tensor):
        a = a.detach().cpu().numpy()
    return np.ascontiguousarray(a, dtype=np.float64).view(np.uint64)


def f32bits(a):
    return np.ascontiguousarray(a, dtype=np.float32).view(np.uint32)


def check_against_reference(label, rows, ref, inverted=True):
    """Every body's row against its reference dict: the sums and quotients within observe_ref.bounds, the rest bit for bit."""
    assert rows.shape == (len(ref), W)
    for b, (row, o) in enumerate(zip(rows, ref)):
        bound = observe_ref.bounds(o)
        worst = 0.0
        for name in SUMS + ("com", "vcom"):
            for k in range(3 if name in ("com", "vcom") else 1):
                want = o[name][k] if name in ("com", "vcom") else o[name]
                allow = bound[name][k] if name in ("com", "vcom") else bound[name]
                got = float(row[AT[name] + k])
                if isinstance(want, float):                      # +inf (no tet) or NaN (a non-finite input)
                    assert (np.isnan(got) and np.isnan(want)) or got == want, (label, b, name, k, got, want)
                    continue
                err = abs(Fraction(got) - want)
                print("%s body %d %s[%d]: |error| %.3g, bound %.3g, value %.17g" % (label, b, name, k, float(err), float(allow), got))
                assert np.isfinite(got) and err <= allow, (label, b, name, k, got, float(want), float(err), float(allow))
                worst = max(worst, float(err / allow) if allow else 0.0)
        if o["mass"] != 0:                                       # the second-order terms the bound leaves to its "+ 1" (observe_ref.bounds)
            assert (observe_ref.R_MOMENT + o["tets"] + 2) * observe_ref.U * o["S"]["mass"] / abs(o["mass"]) < Fraction(1, 10 ** 6)
        for at, name in EXACT:
            want = np.atleast_1d(np.asarray(o[name], dtype=np.float64))
            assert np.array_equal(bits(row[at:at + len(want)]), bits(want)), (label, b, name, row[at:at + len(want)], want)
        if inverted:
            assert o["min_abs_ratio"] > 1e-6, (label, b, float(o["min_abs_ratio"]))
            assert row[capi.OBS_INVERTED_TETS] == o["inverted_tets"], (label, b)
        assert bits(row[capi.OBS_RESERVED])[0] == 0
        print("%s body %d: worst |error| / bound = %.3g" % (label, b, worst))


# ---- 1. against the reference, behind 20 substeps and without a synchronisation in between --------------------------------------------
@pytest.mark.parametrize("kind", list(KINDS))
@pytest.mark.parametrize("mesh", MESHES)
def test_observation_follows_the_step_and_equals_the_reference(mesh, kind):
    c = Case(mesh, kind)
    c.body.simulateSubsteps(20, DT, c.pp)
    obs = c.body.observeBodies()
    torch.cuda.synchronize()
    assert obs.dtype == torch.float64 and obs.is_cuda and tuple(obs.shape) == (len(c.parts), W)
    pos, vel = c.body.pos, c.body.vel
    assert np.isfinite(pos).all() and np.isfinite(vel).all() and np.abs(vel).max() > 0
    ref = c.reference(pos, vel)
    check_against_reference("%s/%s" % (mesh, kind), rows_of(obs), ref)
    # (what the state IS is the solver's business: the clustered FAST Neo-Hookean sweep leaves one sliver tet of the Dragon inside out
    # after these 20 substeps, V/V0 = -3.69, and the kernel and the exact reference agree on it)
    assert all(o["nonfinite"] == 0 for o in ref)


# ---- 2. constructed states: exact inputs, no simulation --------------------------------------------------------------------------------
@pytest.mark.parametrize("kind", list(KINDS))
def test_rest_positions_with_seeded_velocities(kind):
    c = Case("mixed", kind)
    vel = np.random.default_rng(11).normal(0.0, 1.5, c.rest.shape).astype(np.float32)
    c.body.writeState(c.rest, vel)
    rows = rows_of(c.body.observeBodies())
    ref = c.reference(c.rest, vel)
    check_against_reference("rest+vel/" + kind, rows, ref)
    for row, o in zip(rows, ref):                                # the positions are the rest positions: V and V0 are the same sum of the same numbers
        assert bits(row[capi.OBS_VOLUME]) == bits(row[capi.OBS_REST_VOLUME]) and row[capi.OBS_MIN_VOLUME_RATIO] == 1.0 and o["min_volume_ratio"] == 1


@pytest.mark.parametrize("kind", ["polar-fast", "nh-fast"])
def test_a_mirrored_dragon_is_inverted_and_a_nan_is_counted(kind):
    c = Case("dragon3", kind)
    zero = np.zeros_like(c.rest)
    before = rows_of(c.body.observeBodies())
    v0, v1 = int(c.first_vert[1]), int(c.first_vert[2])
    pos = c.rest.copy()
    pos[v0:v1, 0] = (np.float32(2.0) * pos[v0:v1, 0].mean(dtype=np.float64).astype(np.float32) - pos[v0:v1, 0]).astype(np.float32)   # (b) mirrored in x about its own centroid
    c.body.writeState(pos, zero)
    rows = rows_of(c.body.observeBodies())
    check_against_reference("mirrored/" + kind, rows, c.reference(pos, zero))
    assert rows[1, capi.OBS_INVERTED_TETS] == 3840 and rows[1, capi.OBS_MIN_VOLUME_RATIO] < 0 and rows[1, capi.OBS_VOLUME] < 0
    assert np.array_equal(bits(rows[[0, 2]]), bits(before[[0, 2]]))
    pos = c.rest.copy()
    pos[v0 + 7] = np.nan                                         # (c) one particle of body 1
    c.body.writeState(pos, zero)
    rows = rows_of(c.body.observeBodies())
    ref = c.reference(pos, zero)
    assert ref[1]["nonfinite"] == 1 and np.isnan(ref[1]["com"][0])
    check_against_reference("nan/" + kind, rows, ref, inverted=False)
    assert rows[1, capi.OBS_NONFINITE] == 1 and np.isnan(rows[1, capi.OBS_COM:capi.OBS_COM + 3]).all() and np.isnan(rows[1, capi.OBS_VOLUME])
    assert np.isfinite(rows[1, capi.OBS_AABB_MIN:capi.OBS_MAX_SPEED2 + 1]).all() and rows[1, capi.OBS_MASS] == before[1, capi.OBS_MASS]
    assert np.array_equal(bits(rows[[0, 2]]), bits(before[[0, 2]]))


# ---- 3. reproducible and position independent ------------------------------------------------------------------------------------------
@pytest.mark.parametrize("kind", list(KINDS))
@pytest.mark.parametrize("mesh", ["dragon3", "mixed"])
def test_same_bits_again_and_same_bits_alone(mesh, kind):
    c = Case(mesh, kind)
    c.body.simulateSubsteps(20, DT, c.pp)
    first = rows_of(c.body.observeBodies())
    again = rows_of(c.body.observeBodies())
    assert np.array_equal(bits(first), bits(again))
    pos, vel = c.body.pos, c.body.vel
    for b in range(len(c.parts)):
        solo = c.solo(b)
        lo, hi = int(c.first_vert[b]), int(c.first_vert[b + 1])
        solo.writeState(pos[lo:hi], vel[lo:hi])                  # the same state, whatever path the solo body would step through
        assert np.array_equal(f32bits(solo.pos), f32bits(pos[lo:hi])) and np.array_equal(f32bits(solo.vel), f32bits(vel[lo:hi]))
        alone = rows_of(solo.observeBodies())
        assert alone.shape == (1, W) and np.array_equal(bits(alone[0]), bits(first[b])), (mesh, kind, b, alone[0], first[b])


# ---- 4. the contract -------------------------------------------------------------------------------------------------------------------
def sentinel_rows(rows, width):
    return torch.full((rows, width), SENTINEL, dtype=torch.int64, device="cuda").view(torch.float64)


def is_sentinel(t):
    return bool((t.contiguous().view(torch.int64) == SENTINEL).all())


@pytest.mark.parametrize("kind", ["polar-fast", "nh-precise-coloured"])
def test_strided_rows_leave_padding_and_guard_rows_alone(kind):
    c = Case("dragon3", kind)
    c.body.simulateSubsteps(20, DT, c.pp)
    buf = sentinel_rows(3 + 2, 32)                               # rows 256 bytes apart, one guard row in front, one behind
    view = buf[1:-1, :W]
    assert view.stride(0) * 8 == 256 and view.data_ptr() == buf.data_ptr() + 256
    packed = c.body.observeBodies()
    assert c.body.observeBodies(out=view) is view
    torch.cuda.synchronize()
    assert np.array_equal(bits(view), bits(packed)) and not is_sentinel(view[:, :1])
    assert is_sentinel(buf[0]) and is_sentinel(buf[-1]) and is_sentinel(buf[1:-1, W:])
    assert np.array_equal(bits(c.body.bodyObservations()), bits(packed))
    assert c.body.observeBodies() is packed                      # allocated once, reused


@pytest.mark.parametrize("side_stream", [False, True], ids=["default-stream", "side-stream"])
@pytest.mark.parametrize("kind", ["polar-fast", "nh-fast"])
def test_a_reused_tensor_is_ordered_on_its_stream(kind, side_stream):
    """observe, clone, step, observe into the same tensor -- one synchronisation at the end.  The references come from a twin body."""
    c, twin = Case("dragon", kind), Case("dragon", kind)
    twin.body.simulateSubsteps(20, DT, c.pp)
    first = twin.body.bodyObservations()
    twin.body.simulateSubsteps(20, DT, c.pp)
    second = twin.body.bodyObservations()
    assert not np.array_equal(bits(first), bits(second))
    stream = torch.cuda.Stream() if side_stream else torch.cuda.current_stream()
    with torch.cuda.stream(stream):
        c.body.simulateSubsteps(20, DT, c.pp)
        t = c.body.observeBodies()
        kept = t.clone()
        c.body.simulateSubsteps(20, DT, c.pp)
        t2 = c.body.observeBodies(stream=stream if side_stream else None)
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
    for args, text in (((None, 0), "null"), ((p + 4, 0), "aligned"), ((p + 2, 160), "aligned"), ((p, 8), "row_stride"), ((p, 152), "row_stride"),
                       ((p, 164), "row_stride"), ((host.ctypes.data, 0), "not device memory"), ((short.value, 0), "do not fit")):
        rc = L.tetsim_observe_bodies_device(h, args[0], args[1], None)
        assert rc == capi.EINVAL, (args, rc, L.tetsim_last_error(h))
        assert text.encode() in L.tetsim_last_error(h), (args, L.tetsim_last_error(h))
    assert L.tetsim_read_body_observations(h, None) == capi.EINVAL
    torch.cuda.synchronize()
    assert is_sentinel(dst) and np.isnan(host).all() and device_bytes(c.body) == d0   # (not even the tables were made)
    back = np.zeros(nb * 8 * W - 8, np.uint8)
    assert hip.hipMemcpy(C.c_void_p(back.ctypes.data), short, C.c_size_t(back.size), 2) == 0 and (back == 0xA5).all()
    assert hip.hipFree(short) == 0
    for bad in (dst[:nb].float(), dst[:nb - 1], dst[:nb, :W - 1], torch.zeros((nb, W), dtype=torch.float64)):
        with pytest.raises(ValueError):
            c.body.observeBodies(out=bad)
    assert is_sentinel(dst)
    # ... and the next step and the next good call are right, in step with a twin that was never refused anything
    for x in (c, twin):
        x.body.simulateSubsteps(5, DT, x.pp)
    got = c.body.observeBodies(out=dst[:nb])
    torch.cuda.synchronize()
    assert np.array_equal(f32bits(c.body.pos), f32bits(twin.body.pos)) and np.array_equal(f32bits(c.body.vel), f32bits(twin.body.vel))
    assert np.array_equal(bits(got), bits(twin.body.bodyObservations())) and is_sentinel(dst[nb:])


@pytest.mark.parametrize("kind", list(KINDS))
def test_device_bytes_grow_with_the_first_call_only(kind):
    c = Case("mixed", kind)
    c.body.simulateSubsteps(3, DT, c.pp)
    d0 = device_bytes(c.body)
    first = rows_of(c.body.observeBodies())
    d1 = device_bytes(c.body)
    nt, chunks = len(c.tets), sum(-(-len(t) // 256) - (-len(v) // 256) for v, t in c.parts)
    assert d1 >= d0 + 24 * nt + 96 * chunks + 160 * len(c.parts)   # the table (24 bytes per tet), the partial rows, the host read's rows
    assert d1 <= d0 + 24 * nt + 128 * chunks + 256 * len(c.parts) + 4 * len(c.rest)   # ... the chunk and body tables; a polar body's index map
    host = c.body.bodyObservations()
    c.body.observeBodies(out=sentinel_rows(3, 32)[:, :W])
    c.body.simulateSubsteps(3, DT, c.pp)
    c.body.observeBodies()
    assert device_bytes(c.body) == d1
    assert np.array_equal(bits(host), bits(first))


def test_a_partitioned_body_is_refused():
    v, t = load_mesh("lat4")
    parts = [SoftBodyHIP(v, t, None, dict(PP), solver="polar", precision="fast", part_count=2, part_index=i) for i in range(2)]
    for part in parts:
        dst = sentinel_rows(1, W)
        with pytest.raises(TetSimError) as e:
            part.observeBodies(out=dst)
        assert e.value.code == capi.ESTATE and "partitioned" in str(e.value)
        with pytest.raises(TetSimError) as e:
            part.bodyObservations()
        assert e.value.code == capi.ESTATE and "partitioned" in str(e.value)
        torch.cuda.synchronize()
        assert is_sentinel(dst)


# ---- 5. particles and no tets ----------------------------------------------------------------------------------------------------------
def test_a_body_without_tets_has_a_box_and_no_mass():
    v, _ = load_mesh("notets")
    t = np.zeros((0, 4), dtype=np.int32)
    body = SoftBodyHIP(v, t, None, dict(PP), solver="neohookean")
    for _ in range(10):
        body.simulate(DT * 2, PP)
    rows = body.bodyObservations()
    pos, vel = body.pos, body.vel
    (ref,) = observe_ref.observe(v, t, pos, vel, PP["density"])
    check_against_reference("notets", rows, [ref], inverted=False)
    row = rows[0]
    assert row[capi.OBS_MASS] == 0 and not row[capi.OBS_COM:capi.OBS_VCOM + 3].any() and row[capi.OBS_MIN_VOLUME_RATIO] == np.inf
    assert row[capi.OBS_VOLUME] == 0 and row[capi.OBS_REST_VOLUME] == 0 and row[capi.OBS_INVERTED_TETS] == 0
    assert np.isfinite(row[capi.OBS_AABB_MIN:capi.OBS_AABB_MAX + 3]).all() and (row[capi.OBS_AABB_MIN:capi.OBS_AABB_MIN + 3] <= row[capi.OBS_AABB_MAX:capi.OBS_AABB_MAX + 3]).all()
    assert row[capi.OBS_MAX_SPEED2] > 0 and np.array_equal(row[capi.OBS_AABB_MIN:capi.OBS_AABB_MIN + 3], pos.min(axis=0).astype(np.float64))
