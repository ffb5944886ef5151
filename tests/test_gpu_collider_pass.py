"""The collider pass (collide.h) on every stepping path, one substep at a time, against a high-precision reference at the edges of the
definition (collider_ref.py: collide_exact, edge_scene).

The twin construction of test_gpu_colliders.py: body b (no colliders) hangs from GRAB_ID for a warm-up, is saved, and steps ONE more
substep -- prev before it, p0 = b.pos after it.  Body a loads the blob, gets a scene and steps one substep: its pre-collider positions
are p0 bit for bit (save / load and path equality are held elsewhere), so a.pos must be the collider pass applied to (p0, prev).  The scene
is built FROM p0, so its edge cases are exact in f32: a sphere centred on a particle, a degenerate capsule on one, a capsule between the two
particles of a tet edge, boxes whose face gaps tie two and three ways on a particle, a thin box whose centre plane passes through one
(l_k == +0), a plane through one; two overlapping spheres in both list orders; eight entries; frictions 0, 50 and 1e4 (clamped).

What is asserted where the arithmetic is not restated bit for bit (FAST): untouched particles keep b's bits, planted particles do exactly
what their edge demands, and hit particles lie within a bound that is COMPUTED, not chosen: 4 x the largest error of the IEEE f32
restatement against the f64 reference on the same particles, never below 2 x 2^-24 x the largest coordinate (FAST replaces a correctly
rounded division by a 1-ulp reciprocal and a multiply; its fused multiply-adds only remove roundings).  Particles within EPS = 1e-5 m of a
branch of the definition (fragile) must stay finite and are left out; they may be at most 2 % of the hit particles.

Found with this file and fixed in collide.h: FAST computed the capsule parameter as num * rcp(ab2), which can fall an ulp short of 1 where
num >= ab2; a particle exactly on the end point b then stood an ulp off its nearest point, had L > 0, and was thrown out by the whole
radius along rounding noise (gather, fused, call and quad paths; the planted "capsule end b" turned it up).  FAST now decides t >= 1 at
num >= ab2.  The definition itself leaves b alone only where b - a is exact in f32 (a + (b - a) * 1 is b then): the scene picks such an edge.

The lattices are jittered by up to a tenth of a cell (a fixed seed): on a regular lattice the particles sit symmetrically about the planted
ones and tie by the hundred."""
import numpy as np
import pytest

from collider_ref import EPS, collide_exact, collide_f32, collide_f64, edge_scene, exact_velocity, f32_view, pj_velocity, swapped
from conftest import within
from test_gpu_body_grabs import _path
from test_gpu_colliders import DT, GRAB_ID, PP, _dragon, _grab
from test_gpu_random_meshes import random_mesh
from tetsim_amd import SoftBodyHIP, make_lattice

pytestmark = pytest.mark.gpu
WARM = 12   # substeps of warm-up: the body hangs and moves, and a lattice 0.5 mm above the floor has reached it
U = 2.0 ** -24
LOOSE = [0.1, 2.0, 0.1]   # a particle no tet references keeps a small polar body on the one-launch call (test_gpu_call_kernel_irregular.py)


def _bits(a):
    return np.ascontiguousarray(a).view(np.uint32)


def _same(a, b):
    return np.array_equal(_bits(a), _bits(b))


def jittered_lattice(n, y0, flat_bottom=False):
    v, t = make_lattice(n, y0=y0)
    j = np.random.default_rng(n).uniform(0.0, 0.1 / n, v.shape)
    if flat_bottom:
        j[v[:, 1] == v[:, 1].min(), 1] = 0.0                   # the lowest layer stays at y0: it reaches the floor together
    return (v + j).astype(np.float32), t


def mesh(name):
    if name == "dragon":
        return _dragon(0.3)
    if name == "loose":
        v, t = random_mesh(30, 1280)
        return np.concatenate([v, [LOOSE]]).astype(np.float32), t
    if name == "delaunay400":
        return random_mesh(2, 400)
    if name == "floor5":
        return jittered_lattice(5, 0.0005, flat_bottom=True)
    return jittered_lattice(int(name[3:]), 0.3)


POLAR, NH = dict(solver="polar", precision="fast"), dict(solver="neohookean", precision="fast")
# name: (mesh, constructor keywords, TetSimInfo.fused_particle_pass, physicsParams)
CASES = {
    "gather-dragon": ("dragon", dict(POLAR, gather=True), 0, PP),
    "fused-lat28": ("lat28", POLAR, (1, 2), PP),
    "frame-lean-dragon": ("dragon", dict(POLAR, lean_state=True), 2, PP),
    "quad-dragon": ("dragon", POLAR, 3, PP),
    "call-loose": ("loose", POLAR, 5, PP),
    "call-lean-loose": ("loose", dict(POLAR, lean_state=True), 5, PP),
    "nh-frame-dragon": ("dragon", dict(NH, order="original"), 4, PP),
    "nh-clustered-delaunay400": ("delaunay400", dict(NH, order="clustered"), 0, PP),
    "floor-quad-floor5": ("floor5", POLAR, (2, 3), dict(PP, friction=1e4)),
    "precise-polar-dragon": ("dragon", dict(solver="polar", precision="precise"), 0, PP),
    "precise-nh-coloured-dragon": ("dragon", dict(solver="neohookean", precision="precise", order="coloured"), (0, 4), PP),
    "precise-nh-clustered-dragon": ("dragon", dict(solver="neohookean", precision="precise", order="clustered"), 0, PP),
}


def _twins(name, kw, path, pp, count=2):
    """`count` bodies of one constructor, held as _grab() holds them; the last one warmed up, saved, and stepped one substep further.
    Returns (bodies, blob, prev, t, live): live = the particles a test may look at (all but one no tet references)."""
    v, t = mesh(name)
    bodies = [SoftBodyHIP(v, t, None, dict(pp), **kw) for _ in range(count)]
    _path(bodies[0], path)
    for x in bodies:
        x.setGrab(*_grab(v))
    b = bodies[-1]
    b.simulateSubsteps(WARM, DT, pp)
    blob, prev = b.saveState(), b.pos
    b.simulateSubsteps(1, DT, pp)
    live = np.zeros(len(v), bool)
    live[np.unique(t)] = True
    return bodies, blob, prev, t, live


def _scene(b, prev, t, live):
    return edge_scene(b.pos, prev, t, DT, skip=[GRAB_ID] + np.nonzero(~live)[0].tolist())


def check_reference(ex, planted, live, cols):
    """what the scene owes the test, on the reference alone: >= 8 hit particles per entry, fragile particles <= 2 % of the hit ones, every
    planted particle in the state its edge demands.  Returns (planted mask, fragile mask)."""
    n = len(ex["pos"])
    pl = np.zeros(n, bool)
    pl[[i for i, _, _ in planted.values()]] = True
    hit = ex["hits"].any(1)
    fragile = (ex["margin"] < EPS) & ~pl & live
    assert (ex["hits"][live].sum(0) >= 8).all(), ex["hits"][live].sum(0)
    assert (fragile & hit).sum() <= 0.02 * (hit & live).sum(), ((fragile & hit).sum(), hit.sum())
    for what, (i, entry, push) in planted.items():
        mine = ex["hits"][i]
        if push is None:
            assert not mine.any(), (what, mine)
        else:
            k = entry
            assert mine.sum() == 1 and mine[k], (what, mine)
            j = int(np.argmax(np.abs(push)))
            assert ex["face"][i, k] == j and ex["sign"][i, k] == 1.0, (what, ex["face"][i], ex["sign"][i])
    return pl, fragile


def capsule_regions(p0, c, hit):
    """among the particles the capsule hits: how many project before a, between a and b, beyond b"""
    c = f32_view([c])[0]
    ab = c["b"] - c["a"]
    t = ((p0[hit].astype(np.float64) - c["a"]) @ ab) / (ab @ ab)
    return int((t < 0).sum()), int(((t > 0) & (t < 1)).sum()), int((t > 1).sum())


def check_pass(case, a, b, prev, cols, planted, live, pp, order):
    """a (the scene `cols`, one substep from the blob) against b (one substep from the blob, no colliders)"""
    _, kw, _, _ = CASES[case]
    polar, fast = kw["solver"] == "polar", kw["precision"] == "fast"
    p0, v0 = b.pos, b.vel
    got, gotv = a.pos, a.vel
    mask = live.copy()
    mask[GRAB_ID] = False
    if order == 1:   # the two spheres swapped: entries 0 and 1 change places
        planted = {k: (i, {0: 1, 1: 0}.get(e, e), w) for k, (i, e, w) in planted.items()}
    ex = collide_exact(p0, prev, cols, DT, mask)
    pl, fragile = check_reference(ex, planted, live, cols)
    hit = ex["hits"].any(1)
    before, between, beyond = capsule_regions(p0, cols[3], ex["hits"][:, 3])
    assert before > 0 and between > 0 and beyond > 0, (before, between, beyond)
    assert np.isfinite(got[live]).all() and np.isfinite(gotv[live]).all()

    # 1. whom the reference does not hit keeps b's bits (position and velocity); polar: every quaternion does (the colliders act after the solve)
    calm = live & ~hit & ~fragile
    assert _same(got[calm], p0[calm]) and _same(gotv[calm], v0[calm]), np.nonzero(calm & np.any(_bits(got) != _bits(p0), axis=1))[0][:8]
    if polar:
        assert _same(a.quats, b.quats)

    # 2. planted particles: unmoved where the edge says no hit; the demanded face for the ties and the zero -- one rounded add along it
    for what, (i, entry, push) in planted.items():
        want = p0[i] if push is None else (p0[i] + push).astype(np.float32)
        assert _same(got[i] + np.float32(0.0), want + np.float32(0.0)), (case, what, i, got[i], want, p0[i])
        if push is None:
            assert _same(gotv[i], v0[i]), (case, what)

    # 3. hit particles
    sel = live & hit & ~fragile & ~pl
    if not fast:   # PRECISE: the restatement bit for bit, velocity too
        if polar:
            want = collide_f32(p0, prev, cols, DT, mask)
            wantv = pj_velocity(want, prev, DT, pp["gravity"])
        else:
            want = collide_f64(p0, prev, cols, DT, mask)
            wantv = ((want.astype(np.float64) - prev.astype(np.float64)) * (1.0 / float(DT))).astype(np.float32)
        moved = np.any(_bits(want) != _bits(p0), axis=1)
        assert _same(got[live], want[live]), np.nonzero(live & np.any(_bits(got) != _bits(want), axis=1))[0][:8]
        assert _same(gotv[live], np.where(moved[:, None], wantv, v0)[live])
        return
    ref32 = collide_f32(p0, prev, cols, DT, mask)
    e32 = float(np.abs(ref32[sel].astype(np.float64) - ex["pos"][sel]).max())
    bound = max(4.0 * e32, 2.0 * U * float(np.abs(p0[live]).max()))
    err = float(np.abs(got[sel].astype(np.float64) - ex["pos"][sel]).max())
    exv = exact_velocity(ex["pos"], prev, DT, pp["gravity"] if polar else None)
    vbound = bound / float(np.float32(DT)) + 4.0 * U * float(np.abs(exv[live]).max())
    verr = float(np.abs(gotv[sel].astype(np.float64) - exv[sel]).max())
    print("collider pass FAST %s order %d: hit %d fragile %d | pos error %.3g, f32 restatement %.3g, bound %.3g | vel error %.3g, bound %.3g | max r/L %.3g"
          % (case, order, sel.sum(), (fragile & hit).sum(), err, e32, bound, verr, vbound, ex["cond"][sel].max()))
    within("collider pass fast %s vs exact" % case, err, bound)
    within("collider pass fast %s vs exact (vel)" % case, verr, vbound)

    # 4. clamped friction (dt * friction > 1) leaves no tangential motion relative to the collider: p - q - V dt is parallel to n
    for k, c in enumerate(cols):
        if np.float32(DT) * np.float32(c["friction"]) <= 1.0:
            continue
        only = sel & ex["hits"][:, k] & (ex["hits"].sum(1) == 1)
        assert only.sum() >= 4, (k, only.sum())
        w = got[only].astype(np.float64) - prev[only].astype(np.float64) - np.asarray(c.get("velocity", [0, 0, 0]), np.float64) * float(np.float32(DT))
        nrm = ex["normal"][only, k]
        slip = np.linalg.norm(w - nrm * (w * nrm).sum(1)[:, None], axis=1).max()
        # (the exact result has no slip at all; a position within `bound` per coordinate is within sqrt(3) * bound as a vector, and
        # taking its tangential part does not lengthen it)
        assert slip <= np.sqrt(3.0) * bound, (case, k, slip, bound)


@pytest.mark.parametrize("case", list(CASES))
def test_collider_pass_of_one_substep_against_the_exact_reference(case):
    name, kw, path, pp = CASES[case]
    (a, b), blob, prev, t, live = _twins(name, kw, path, pp)
    cols, planted = _scene(b, prev, t, live)
    assert len(cols) == 8 and {float(c["friction"]) for c in cols} == {0.0, 50.0, 1e4} and any(np.any(c.get("velocity", 0)) for c in cols)
    if case.startswith("floor"):
        assert (b.pos[:, 1] == 0.0).sum() >= 4                 # the floor branch acted in that substep, with its friction clamped
        assert np.float32(DT) * np.float32(pp["friction"]) > 1.0
    results = []
    for order, cs in enumerate((cols, swapped(cols))):
        a.loadState(blob)
        a.setColliders(cs)
        a.simulateSubsteps(1, DT, pp)
        check_pass(case, a, b, prev, cs, planted, live, pp, order)
        results.append(a.pos)
    assert not _same(results[0][live], results[1][live])       # the list order matters where the spheres overlap


# ---- the edge scene in the multi-substep kernels, through equalities the library promises -------------------------------------------

@pytest.mark.parametrize("case", ["quad-dragon", "frame-lean-dragon", "call-loose", "nh-frame-dragon"])
def test_one_call_of_four_substeps_equals_four_calls_with_the_edge_scene(case):
    name, kw, path, pp = CASES[case]
    (x, y, none, b), blob, prev, t, live = _twins(name, kw, path, pp, count=4)
    cols, _ = _scene(b, prev, t, live)
    for body in (x, y, none):
        body.loadState(blob)
    x.setColliders(cols)
    y.setColliders(cols)
    x.simulateSubsteps(4, DT, pp)
    none.simulateSubsteps(4, DT, pp)
    for _ in range(4):
        y.simulateSubsteps(1, DT, pp)
    assert _same(x.pos[live], y.pos[live]) and _same(x.vel[live], y.vel[live])
    assert not _same(x.pos[live], none.pos[live])


@pytest.mark.parametrize("kw", [POLAR, NH], ids=["polar-fast", "nh-fast"])
def test_edge_scenes_as_body_colliders_of_a_batch_equal_the_solos(kw):
    meshes = [_dragon(0.3), jittered_lattice(5, 0.3), _dragon(0.5)]
    batch = SoftBodyHIP.batch(meshes, dict(PP), **kw)
    solos = [SoftBodyHIP(v, t, None, dict(PP), **kw) for v, t in meshes]
    lists = []
    for (v, t), solo in zip(meshes, solos):
        solo.simulateSubsteps(WARM, DT, PP)
        blob, prev = solo.saveState(), solo.pos
        solo.simulateSubsteps(1, DT, PP)
        lists.append(edge_scene(solo.pos, prev, t, DT)[0])
        solo.loadState(blob)
        solo.setColliders(lists[-1])
    batch.simulateSubsteps(WARM, DT, PP)
    batch.setBodyColliders(lists)
    for n in (1, 3):
        pos, vel = [], []
        for body in [batch] + solos:
            body.simulateSubsteps(n, DT, PP)
        pos, vel = batch.pos, batch.vel
        for ((p0, p1), _), solo in zip(batch.bodyRanges, solos):
            assert _same(pos[p0:p1], solo.pos) and _same(vel[p0:p1], solo.vel), n
