"""The per-body device calls on the crowd of tests/crowd.py: 300 bodies behind one handle, most of them single tets -- the batch shapes
at which place.hip, body_grabs.hip, snapshot.hip, the per-body reductions and the range sensors take the branches no batch of three reaches
(a 256-row chunk of more than eight bodies, host rows over several launches, a second workgroup of the one-lane-per-body kernels, waves of
sixteen bodies, hundreds of chunks with a handful of live lanes) -- and, on single lattices, a body of more than 256 chunks for the observe
and strain reductions.  Nothing here has a tolerance of its own: every comparison is on bits -- against the body ALONE, against the numpy
restatements, against the host variants -- or uses the bounds observe_ref / pose_ref derive.  tests/test_crowd_cpu.py shows without a GPU
that the references are usable at this shape.  profiles/crowd_mutation.txt: nine mutants of the kernels, each killed by this file.
Every test prints the fused_particle_pass of its bodies."""
import numpy as np
import pytest
import torch

import crowd
import observe_ref
import raycast_device_ref as ray_ref
from test_gpu_body_grabs import _same_bodies
from test_gpu_device_io import DT
from test_gpu_observe import check_against_reference, is_sentinel, sentinel_rows
from test_gpu_observe import rows_of as obs_rows
from test_gpu_place import placed, rows_tensor, values
from test_gpu_pose import check_rows as check_pose_rows
from test_gpu_pose import rows_of as pose_rows
from test_gpu_raycast_device import assert_same, cast
from test_gpu_snapshot import KINDS, cuda_mask, show
from test_gpu_strain import reference as strain_reference
from test_pose_cpu import prep_table
from tetsim_amd import RAY_HIT_DTYPE, SoftBodyHIP, make_lattice
from tetsim_amd import _capi as capi

pytestmark = pytest.mark.gpu
PP = crowd.PP
SAMPLE = crowd.SAMPLE
SOME = ["polar-fast", "polar-precise", "nh-fast"]
SEED = 5
FLT_MAX64 = np.finfo(np.float64).max


@pytest.fixture(scope="module")
def world():
    """(the crowd, its seeded positions and velocities): host arrays, shared and never written"""
    c = crowd.build()
    pos, vel = c.state(SEED)
    for a in (c.rest, c.tets, pos, vel):
        a.setflags(write=False)
    return c, pos, vel


def make_batch(c, kind, visual=False):
    b = SoftBodyHIP.batch(c.bodies, dict(PP), ref_fixed_bounds=False, **KINDS[kind])
    assert b.info.num_bodies == crowd.COUNT
    assert [r[0][0] for r in b.bodyRanges] == c.first_vert[:-1].tolist() and [r[1][0] for r in b.bodyRanges] == c.first_tet[:-1].tolist()
    if visual:
        b.setVisualMesh(c.vis)
        b.setVisualTriangles(c.tris)
    return b


def make_solo(c, b, kind, visual=False):
    v, t = c.bodies[b]
    extra = (c.vis_parts[b], c.tri_parts[b]) if visual else ()
    return SoftBodyHIP(v, t, None, dict(PP), *extra, ref_fixed_bounds=False, **KINDS[kind])


def load(body, pos, vel):
    """the state through the device import"""
    body.importTensors(torch.from_numpy(np.array(pos, dtype=np.float32)).cuda(), torch.from_numpy(np.array(vel, dtype=np.float32)).cuda())


def seeded(c, kind, pos, vel, substeps=0, visual=False):
    b = make_batch(c, kind, visual)
    load(b, pos, vel)
    if substeps:
        b.simulateSubsteps(substeps, DT, PP)
    return b


def solos(c, kind, pos, vel, substeps=0, visual=False):
    """{b: body b alone in the seeded state} for SAMPLE"""
    out = {}
    for b in SAMPLE:
        s = out[b] = make_solo(c, b, kind, visual)
        load(s, c.body(b, pos), c.body(b, vel))
        if substeps:
            s.simulateSubsteps(substeps, DT, PP)
    return out


def u32(a):
    return np.ascontiguousarray(a, dtype=np.float32).view(np.uint32)


def u64(a):
    if isinstance(a, torch.Tensor):
        a = a.detach().cpu().numpy()
    return np.ascontiguousarray(a, dtype=np.float64).view(np.uint64)


def state_bits(body):
    """{name: bits} of what the host can read of the state, the quaternions by the caller's tet id (each handle keeps its own tet order)"""
    out = {"pos": u32(body.pos), "vel": u32(body.vel)}
    if body.solver == "polar":
        q = np.empty_like(body.quats)
        q[body.localTets] = body.quats
        out["quats"] = u32(q)
    else:
        out["prevPos"] = u32(body.prevPos)
    return out


TET_FIELDS = ("quats", "volError")   # of state_bits / complete_bits: one row per tet; the others one per particle


def complete_bits(c, body):
    """state_bits and, for a Neo-Hookean body, the volError section of its state -- the last 8 * nt bytes of saveState(), row i the tet
    tetOrder[i] of the caller (a coloured or clustered order interleaves the bodies) -- by the caller's tet id"""
    out = state_bits(body)
    if body.solver != "polar":
        nt = len(c.tets)
        rows = np.frombuffer(body.saveState()[-8 * nt:], dtype=np.uint64)
        order = body.tetOrder
        assert sorted(order.tolist()) == list(range(nt))
        by_tet = np.empty((nt, 1), np.uint64)
        by_tet[order, 0] = rows
        out["volError"] = by_tet
    return out


def explain(c, got, want, bodies):
    """for a failure's message: per differing body and field, how many rows differ and by how much at most"""
    out = []
    for b in bodies[:4]:
        for n in got:
            g, w = (c.body_tets(b, got[n]), c.body_tets(b, want[n])) if n in TET_FIELDS else (c.body(b, got[n]), c.body(b, want[n]))
            rows = np.flatnonzero((g != w).any(axis=1))
            if len(rows):
                out.append((int(b), crowd.KINDS[b], n, len(rows), len(g), float(np.abs(g.view(np.float32).astype(np.float64) - w.view(np.float32)).max())))   # (volError: as two halves)
    return out


def differing(c, got, want, bodies=range(crowd.COUNT)):
    """the bodies of `bodies` whose part of state_bits `got` differs from their part of `want`"""
    return [b for b in bodies if any(not np.array_equal(c.body_tets(b, got[n]) if n in TET_FIELDS else c.body(b, got[n]),
                                                         c.body_tets(b, want[n]) if n in TET_FIELDS else c.body(b, want[n])) for n in got)]


class Sampled:
    """What test_gpu_body_grabs._same_bodies reads of a batch, narrowed to SAMPLE: it then pairs body k of SAMPLE with solo k."""

    def __init__(self, batch):
        self.pos, self.vel, self.solver = batch.pos, batch.vel, batch.solver
        if self.solver == "polar":
            self.quats, self.localTets = batch.quats, batch.localTets
        ranges = batch.bodyRanges
        self.bodyRanges = [ranges[b] for b in SAMPLE]


def against_solos(c, batch, alone):
    """the SAMPLE bodies that differ from their solo: pos, vel and quats by _same_bodies, prevPos here"""
    bad = [SAMPLE[k] for k in _same_bodies(Sampled(batch), [alone[b] for b in SAMPLE])]
    if batch.solver != "polar":
        prev = batch.prevPos
        bad += [b for b in SAMPLE if not np.array_equal(u32(c.body(b, prev)), u32(alone[b].prevPos))]
    return sorted(set(bad))


# ---- 2.1 per-body grabs -----------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("kind", list(KINDS))
def test_batch_equals_solos_under_body_grabs(world, kind):
    """Six frames of a table over all 300 rows: through the host call (three launches of 128, 128 and 44 rows), through the device call with
    a seeded mask whose masked-out bodies keep last frame's row, and through the device call with a mask of ones.  The host is given the
    table the masked device call leaves in force, so all three hold the same rows."""
    c, pos, vel = world
    host, dev, ones = (seeded(c, kind, pos, vel) for _ in range(3))
    alone = solos(c, kind, pos, vel)
    show("crowd grabs %s" % kind, host, dev, ones, *alone.values())
    rng = np.random.default_rng(17)
    all_ones = cuda_mask([1] * crowd.COUNT)
    held, in_force = c.grab_table(21, 0)
    in_force = in_force.copy()
    for frame in range(6):
        _, x = c.grab_table(21, frame)
        m = np.ones(crowd.COUNT, bool) if frame == 0 else rng.random(crowd.COUNT) < 0.5
        in_force[m] = x[m]
        host.setBodyGrabs(held, in_force)
        wide = torch.full((crowd.COUNT, 4), 7.0, dtype=torch.float32, device="cuda")   # rows of 16 bytes; every body's NEW row, wanted or not
        wide[:, :3] = torch.from_numpy(x).cuda()
        dev.setBodyGrabsDevice(torch.from_numpy(held).cuda(), wide[:, :3], bodies=None if frame == 0 else torch.from_numpy(m).cuda())
        ones.setBodyGrabsDevice(torch.from_numpy(held).cuda(), torch.from_numpy(in_force).cuda(), bodies=all_ones)
        for b in (host, dev, ones):
            b.simulateSubsteps(5, DT, PP)
        for b, s in alone.items():
            if held[b] >= 0:
                s.setGrab(int(held[b]), in_force[b])
            s.simulateSubsteps(5, DT, PP)
    assert sum(held[b] >= 0 for b in SAMPLE) >= 4 and not np.array_equal(in_force, c.grab_table(21, 5)[1])
    assert against_solos(c, host, alone) == [] and against_solos(c, dev, alone) == []
    want = state_bits(host)
    assert differing(c, state_bits(dev), want) == [] and differing(c, state_bits(ones), want) == []
    free = seeded(c, kind, pos, vel)                                                   # (the held bodies, and only they, differ from an unheld run)
    show("crowd grabs %s, unheld" % kind, free)
    for _ in range(6):
        free.simulateSubsteps(5, DT, PP)
    assert differing(c, state_bits(free), want) == np.flatnonzero(held >= 0).tolist()
    # off: every row back to "none", over three launches
    for b in (host, dev, ones):
        b.setBodyGrabs(None, None)
        b.simulateSubsteps(5, DT, PP)
    for s in alone.values():
        s.setGrab(-1, [0.0, 0.0, 0.0])
        s.simulateSubsteps(5, DT, PP)
    assert against_solos(c, host, alone) == [] and against_solos(c, dev, alone) == []
    assert differing(c, state_bits(dev), state_bits(host)) == [] and differing(c, state_bits(ones), state_bits(host)) == []
    for b in [host, dev, ones, free] + list(alone.values()):
        b.close()


# ---- 2.2 placement ----------------------------------------------------------------------------------------------------------------------
def split_values(c, batch):
    """test_gpu_place.values of a batch, body by body (the quaternions of a body are one range of the handle's own tet order)"""
    r = values(batch)
    return [{n: a[e0:e1] if n == "quats" else a[p0:p1] for n, a in r.items()} for (p0, p1), (e0, e1) in batch.bodyRanges]


@pytest.mark.parametrize("keep", [False, True], ids=["set-velocity", "keep-velocity"])
@pytest.mark.parametrize("kind", list(KINDS))
def test_placement_of_half_the_crowd(world, kind, keep):
    c, pos, vel = world
    run = crowd.runs()[0][0]
    rows, chosen = c.place_rows(31), c.mask(32)
    # two chosen bodies whose rows the device refuses and which stay where they are: single tets of the run, outside the forced pattern
    nan_body, zero_body = [run + k for k in range(12, 30) if k != 17 and chosen[run + k]][:2]
    bad = rows.copy()
    bad[nan_body, capi.PLACE_LINEAR + 1] = np.nan
    bad[zero_body, capi.PLACE_Q:capi.PLACE_Q + 4] = 0.0
    moved = chosen.copy()
    moved[[nan_body, zero_body]] = False
    a, twin = (seeded(c, kind, pos, vel, 5) for _ in range(2))
    alone = solos(c, kind, pos, vel, 5)
    show("crowd place %s" % kind, a, twin, *alone.values())
    before, before_bits = split_values(c, a), state_bits(a)
    a.placeBodiesDevice(rows_tensor(bad), bodies=torch.from_numpy(chosen).cuda(), keep_velocity=keep)
    after = split_values(c, a)
    for b in range(crowd.COUNT):
        want = placed(rows[b], before[b], keep) if moved[b] else before[b]
        for n in want:
            assert np.array_equal(u32(after[b][n]), u32(want[n])), (b, n, bool(chosen[b]))
    untouched = np.flatnonzero(~moved).tolist()
    assert differing(c, state_bits(a), before_bits) == np.flatnonzero(moved).tolist()
    assert all(x in untouched for x in (run + 8, run + 11, nan_body, zero_body)) and all(moved[first + k] for first, _ in crowd.runs() for k in (3, 9, 10, 17))
    # the host variant: its rows travel 32 per launch
    twin.placeBodies(rows, bodies=moved, keep_velocity=keep)
    assert differing(c, state_bits(twin), state_bits(a)) == []
    # the hidden sections -- predictions, carried shapes, prev -- show in the steps behind the placement
    for b, s in alone.items():
        if moved[b]:
            s.placeBodies(rows[b:b + 1], keep_velocity=keep)
        s.simulateSubsteps(5, DT, PP)
    a.simulateSubsteps(5, DT, PP)
    twin.simulateSubsteps(5, DT, PP)
    assert any(moved[b] for b in SAMPLE) and not all(moved[b] for b in SAMPLE)
    assert against_solos(c, a, alone) == [] and against_solos(c, twin, alone) == []
    for b in [a, twin] + list(alone.values()):
        b.close()


# ---- 2.3 snapshots with masks -----------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("kind", list(KINDS))
def test_masked_capture_and_restore_over_the_crowd(world, kind):
    """A masked restore whose parts share no dt -- the snapshot sits right behind the import, the capture behind 8 substeps -- makes the
    whole handle predict afresh (snapshot.hip: intersect_validity), so the twins do the same before the last five substeps, as
    test_gpu_snapshot.test_dt_mismatch_in_a_batch does.  The Neo-Hookean kinds compare the volError rows too: 8-byte rows, two to a
    16-byte unit, in solve order."""
    c, pos, vel = world
    m1, m2 = c.mask(41), c.mask(42)
    twins = {0: seeded(c, kind, pos, vel), 8: seeded(c, kind, pos, vel, 8), 16: seeded(c, kind, pos, vel, 8)}
    twins[16].simulateSubsteps(8, DT, PP)
    a = seeded(c, kind, pos, vel)
    show("crowd snapshot %s" % kind, a, *twins.values())
    snap = a.snapshot()
    a.simulateSubsteps(8, DT, PP)
    a.capture(snap, bodies=torch.from_numpy(m1).cuda())
    a.simulateSubsteps(8, DT, PP)
    a.restore(snap, bodies=torch.from_numpy(m2).cuda())
    source = np.where(~m2, 16, np.where(m1, 8, 0))             # outside M2: never restored; in M2: from the capture at 8 or the snapshot at 0
    assert all((source == s).sum() >= 40 for s in (0, 8, 16))

    def check(stage):
        got = complete_bits(c, a)
        want = {s: complete_bits(c, t) for s, t in twins.items()}
        for s in (0, 8, 16):
            bad = differing(c, got, want[s], np.flatnonzero(source == s))
            assert bad == [], (stage, s, bad, explain(c, got, want[s], bad))
        others = [len(differing(c, got, want[s], np.flatnonzero(source != s))) for s in (0, 8, 16)]
        assert others == [int((source != s).sum()) for s in (0, 8, 16)], (stage, others)   # (every body is told apart from the other moments)
        if "volError" in got:                                   # ... and so do the volError rows alone tell the three moments apart
            apart = [len(differing(c, {"volError": want[s]["volError"]}, {"volError": want[t]["volError"]})) for s, t in ((0, 8), (8, 16), (0, 16))]
            print("%s: bodies whose volError rows differ between the twins at 0 / 8, 8 / 16, 0 / 16 substeps: %s" % (stage, apart))
            assert min(apart) >= 150, (stage, apart)

    check("right after the restore")
    for t in twins.values():
        moved = t.exportTensors(("pos", "vel"))
        t.importTensors(moved["pos"], moved["vel"])
    for b in [a] + list(twins.values()):
        b.simulateSubsteps(5, DT, PP)
    check("five substeps later")
    snap.close()
    for b in [a] + list(twins.values()):
        b.close()


# ---- 2.4 nearest particle per body ------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("kind", SOME)
def test_nearest_particle_of_every_body(world, kind):
    c, pos, vel = world
    gone = crowd.runs()[1][0] + 1                              # a single tet none of whose particles can be picked
    assert gone not in SAMPLE and gone not in c.tie_bodies()
    bad = pos.copy()
    bad[c.first_vert[gone]:c.first_vert[gone + 1]] = np.nan
    pts = c.query_points(pos)
    want_ids, want_d2, tied = c.nearest(bad, pts)
    assert (tied >= 2).sum() >= 21 and tied[crowd.LAT8] == 2 and want_ids[crowd.LAT8] >= 256 and want_ids[gone] == -1
    batch = seeded(c, kind, bad, vel)
    alone = solos(c, kind, pos, vel)
    show("crowd nearest %s" % kind, batch, *alone.values())
    wide = torch.zeros((crowd.COUNT, 4), dtype=torch.float32, device="cuda")
    wide[:, :3] = torch.from_numpy(pts).cuda()
    ids, d2 = batch.nearestParticlesDevice(wide[:, :3])
    ids, d2 = ids.cpu().numpy(), d2.cpu().numpy()
    assert np.array_equal(ids, want_ids), np.flatnonzero(ids != want_ids)
    assert np.array_equal(u64(d2), u64(want_d2)), np.flatnonzero(d2 != want_d2)
    assert ids[gone] == -1 and d2[gone] == FLT_MAX64
    for b, s in alone.items():
        i, d = s.nearestParticle(pts[b])
        assert i == int(ids[b]) and np.array_equal(u64(d), u64(d2[b])), (b, i, d, ids[b], d2[b])
    for b in [batch] + list(alone.values()):
        b.close()


# ---- 2.5 observations, poses, strain rows -----------------------------------------------------------------------------------------------
def strided(rows, width, stride):
    """(buffer, view): `rows` rows of `width` doubles `stride` doubles apart in a sentinel-filled buffer that is one row too long"""
    buf = sentinel_rows(rows + 1, stride)
    return buf, buf[:rows, :width]


@pytest.mark.parametrize("kind", SOME)
def test_observations_poses_and_strain_of_every_body(world, kind):
    c, pos, vel = world
    batch = seeded(c, kind, pos, vel, 10)
    show("crowd observe %s" % kind, batch)
    n = crowd.COUNT
    obuf, oview = strided(n, capi.OBS_WIDTH, 24)
    pbuf, pview = strided(n, capi.POSE_WIDTH, 50)
    sbuf, sview = strided(n, capi.STRAIN_BODY_WIDTH, 9)
    assert oview.stride(0) == 24 and pview.stride(0) == 50 and sview.stride(0) == 9
    assert batch.observeBodies(out=oview) is oview and batch.observePoses(out=pview) is pview and batch.bodyStrainDevice(out=sview) is sview
    tet_rows = batch.tetStrainDevice()
    torch.cuda.synchronize()
    for buf, view, w in ((obuf, oview, capi.OBS_WIDTH), (pbuf, pview, capi.POSE_WIDTH), (sbuf, sview, capi.STRAIN_BODY_WIDTH)):
        assert is_sentinel(buf[n]) and is_sentinel(buf[:n, w:]) and not is_sentinel(view[:, :1])
    now, u = batch.pos, batch.vel
    assert np.isfinite(now).all() and np.isfinite(u).all() and np.abs(now - pos).max() > 1e-4
    obs, poses, srows = obs_rows(oview), pose_rows(pview), sview.cpu().numpy().copy()
    label = "crowd/" + kind
    check_against_reference(label, obs, observe_ref.observe(c.rest, c.tets, now, u, PP["density"], c.first_vert, c.first_tet))
    check_pose_rows(label, poses, prep_table(c.rest, c.tets, c.first_vert, c.first_tet, PP["density"])[0], now, u, c.first_vert)
    want_tets, want_body = strain_reference(c.rest, c.tets, now, c.first_tet)
    assert np.array_equal(u32(tet_rows.cpu().numpy()), u32(want_tets))
    assert np.array_equal(u64(srows), u64(want_body)), np.flatnonzero((u64(srows) != u64(want_body)).any(axis=1))
    assert np.array_equal(u64(batch.bodyObservations()), u64(obs)) and np.array_equal(u64(batch.bodyPoses()), u64(poses))
    alone = {b: make_solo(c, b, kind) for b in SAMPLE}
    show("crowd observe %s, alone" % kind, *alone.values())
    for b, s in alone.items():                                  # a body of a batch gives the bits it gives alone
        s.writeState(c.body(b, now), c.body(b, u))
        assert np.array_equal(u32(s.pos), u32(c.body(b, now))) and np.array_equal(u32(s.vel), u32(c.body(b, u)))
        assert np.array_equal(u64(s.observeBodies()), u64(obs[b:b + 1])), b
        assert np.array_equal(u64(s.observePoses()), u64(poses[b:b + 1])), b
        assert np.array_equal(u64(s.bodyStrainDevice()), u64(srows[b:b + 1])), b
        assert np.array_equal(u32(s.tetStrainDevice().cpu().numpy()), u32(c.body_tets(b, want_tets))), b
        s.close()
    batch.close()


# ---- 2.6 bounding spheres and range sensors ---------------------------------------------------------------------------------------------
@pytest.mark.parametrize("kind", SOME)
def test_spheres_and_rays_of_every_body(world, kind):
    c, pos, vel = world
    batch = seeded(c, kind, pos, vel, visual=True)
    alone = solos(c, kind, pos, vel, visual=True)
    show("crowd rays %s" % kind, batch, *alone.values())
    n = crowd.COUNT
    buf = torch.full((n + 1, 6), float("nan"), dtype=torch.float64, device="cuda")
    out = batch.visualBoundingSpheresDevice(out=buf[:n, :4])
    vis = batch.exportTensors(("visPos",))["visPos"].cpu().numpy()
    assert torch.isnan(buf[n]).all() and torch.isnan(buf[:, 4:]).all()
    assert np.array_equal(u32(vis), u32(c.visual_positions(pos)))              # (every row sits on a particle)
    spheres = out.cpu().numpy()
    want = c.spheres(vis)
    assert np.array_equal(u64(spheres), u64(want)), np.flatnonzero((u64(spheres) != u64(want)).any(axis=1))
    for b, s in alone.items():
        centre, r = s.visualBoundingSphere()
        assert np.array_equal(u64(spheres[b]), u64(np.append(centre, r))), b
    # 4 rays per body, grouped by body (workgroups of 64 bodies) and shuffled (up to 256 bodies in a workgroup)
    o, d, rb = c.rays(c.visual_positions(pos), SEED)
    want = c.raycast(vis, o, d, rb)
    assert ray_ref.hit_share_ok(want["hit"])
    grouped = cast(batch, o, d, bodies=rb)
    assert_same(grouped, want, "grouped")
    perm = np.random.default_rng(29).permutation(len(o))
    assert_same(cast(batch, o[perm], d[perm], bodies=rb[perm]), want[perm], "shuffled")
    assert ray_ref.hit_share_ok(grouped["hit"])
    for b, s in alone.items():                                                  # test_gpu_raycast_device.solo_answer, for the bodies that have a solo
        sel = np.flatnonzero(rb == b)
        h = s.raycastVisual(o[sel], d[sel])
        hit = h["hit"] == 1
        h["triangle"][hit] += c.first_tri[b]
        h["body"][hit] = b
        assert_same(grouped[sel], h, "solo %d" % b)
    assert_same(cast(batch, o, d), batch.raycastVisual(o, d), "without ray_body")
    assert grouped.dtype == RAY_HIT_DTYPE
    for b in [batch] + list(alone.values()):
        b.close()


# ---- 2.7 more than 256 chunks in one body -----------------------------------------------------------------------------------------------
_lat23 = []


def lat23():
    """Computed once: make_lattice(23) with seeded noise on its positions and seeded velocities, and the references of that state.  (The
    exact arithmetic of observe_ref takes 5 s for its 73,002 tets on one core, so both kinds share it.)"""
    if not _lat23:
        v, t = make_lattice(23)
        assert len(t) == 73002 > 256 * 256 >= len(make_lattice(22)[1]) and -(-len(t) // 256) == 286
        rng = np.random.default_rng(3)
        pos = (v + rng.normal(0.0, 0.03 / 23, v.shape)).astype(np.float32)
        vel = rng.normal(0.0, 1.5, v.shape).astype(np.float32)
        _lat23.extend([v, t, pos, vel, observe_ref.observe(v, t, pos, vel, PP["density"]), *strain_reference(v, t, pos)])
    return _lat23


@pytest.mark.parametrize("kind", ["polar-fast", "nh-fast"])
def test_a_body_of_more_than_256_tet_chunks(kind):
    """The finish kernels' thread t folds the chunk rows t, t + 256, ..: the smallest lattice above 65,536 tets, kept whole."""
    v, t, pos, vel, want_obs, want_tets, want_body = lat23()
    body = SoftBodyHIP(v, t, None, dict(PP), ref_fixed_bounds=False, **KINDS[kind])
    show("lat23 %s" % kind, body)
    body.writeState(pos, vel)
    obs = body.bodyObservations()
    brow = body.bodyStrainDevice()
    check_against_reference("lat23/" + kind, obs, want_obs)
    assert abs(obs[0, capi.OBS_MASS] - 1000.0) < 1e-2 and np.array_equal(u64(obs_rows(body.observeBodies())), u64(obs))
    assert np.array_equal(u64(brow), u64(want_body)), (brow.cpu().numpy(), want_body)
    assert np.array_equal(u32(body.tetStrain()), u32(want_tets)) and want_body[0, 7] == 0 and abs(want_body[0, 6] - 1.0) < 1e-5
    body.close()


def test_a_body_of_more_than_256_vertex_chunks():
    """The exact fields of the observation over 270 chunks of particles: the box, the fastest particle and the non-finite count, with the
    extremes and one of two non-finite particles behind the 256th chunk."""
    v, t = make_lattice(40)
    assert 256 * 256 < len(v) == 68921
    rng = np.random.default_rng(4)
    pos, vel = v.copy(), rng.normal(0.0, 1.5, v.shape).astype(np.float32)
    late = 256 * 256 + np.array([100, 900, 1700, 2500])       # chunks 256, 259, 262, 265
    pos[late[0]] += np.float32([0.75, 0.0, 0.0])
    pos[late[1]] += np.float32([0.0, 0.25, 0.75])
    vel[late[2]] = [9.0, -8.0, 7.0]
    pos[late[3], 1] = np.nan
    vel[1000, 2] = np.inf                                      # (chunk 3)
    body = SoftBodyHIP(v, t, None, dict(PP), solver="polar", precision="fast")
    show("lat40", body)
    body.writeState(pos, vel)
    row = body.bodyObservations()[0]
    ok = np.isfinite(pos).all(axis=1) & np.isfinite(vel).all(axis=1)
    u = vel[ok].astype(np.float64)
    speed2 = ((u[:, 0] * u[:, 0] + u[:, 1] * u[:, 1]) + u[:, 2] * u[:, 2]).max()
    assert speed2 == 194.0 and (~ok).sum() == 2
    assert np.array_equal(u64(row[capi.OBS_AABB_MIN:capi.OBS_AABB_MIN + 3]), u64(pos[ok].min(axis=0)))
    assert np.array_equal(u64(row[capi.OBS_AABB_MAX:capi.OBS_AABB_MAX + 3]), u64(pos[ok].max(axis=0)))
    assert row[capi.OBS_AABB_MAX] == pos[late[0], 0] and row[capi.OBS_AABB_MAX + 2] == pos[late[1], 2]
    assert np.array_equal(u64(row[capi.OBS_MAX_SPEED2]), u64(speed2)) and row[capi.OBS_NONFINITE] == 2
    body.close()
