"""The one-launch call of large polar bodies (pj_blocked.hip: pjb_call_kernel, TetSimInfo.fused_particle_pass == 5) where lattices do not
reach: irregular meshes, checkpoints and long calls.

Every partial sum, prediction (pos_pred.w) and end-of-substep position (pos_final.w) the call writes carries the sequence number of its
substep, and waves of later substeps of the same grid poll for it.  On a lattice the partial-sum lists are at most 9 long (the 8-wide
gather's second round is the last), every tile is full and the tile count is whatever it is; Delaunay meshes have lists of 40, ragged
tiles and any tile count.  A body with a particle no tet references takes this path at any size (tetsim_create.hip), with every
substep's workgroups resident together -- the hardest case for the polls.  The checkpoint tests hold the stamps out of the blob
(tetsim_state.hip: clear_stamps), the long-call tests the launch inside the 2^32 - 1 work-items a dispatch holds (dev_common.h: call_chunk).
TETSIM_PJ_ONE_LAUNCH=0 (read at creation) keeps the tet kernel + particle kernel pair: the twin of most tests here."""
import ctypes as C
import functools
import os

import numpy as np
import pytest

from conftest import load_mesh, within
from test_gpu_random_meshes import random_mesh

from oracle import OraclePJ
from tetsim_amd import SoftBodyHIP, _capi as capi, make_lattice

pytestmark = pytest.mark.gpu
PP = dict(gravity=-9.81, friction=1000.0, density=1000.0, devCompliance=1e-5, volCompliance=0.0,
          worldBounds=[-2.5, -1.0, -2.5, 2.5, 10.0, 2.5])
DT = (1.0 / 60.0) / 20
CALLS = ((20, DT), (1, DT), (7, DT), (3, DT * 2), (20, DT))    # mixed lengths, a dt change; a grab from the third call to the fifth
LOOSE = [0.1, 2.0, 0.1]
GRID_ITEMS = 2 ** 32 - 1                                       # work-items one dispatch holds


def _same(a, b):
    return np.array_equal(np.asarray(a).view(np.uint32), np.asarray(b).view(np.uint32))


def _polar(v, t, one_launch=True, **kw):
    if one_launch:
        return SoftBodyHIP(v, t, None, dict(PP), solver="polar", precision="fast", **kw)
    os.environ["TETSIM_PJ_ONE_LAUNCH"] = "0"
    try:
        return SoftBodyHIP(v, t, None, dict(PP), solver="polar", precision="fast", **kw)
    finally:
        del os.environ["TETSIM_PJ_ONE_LAUNCH"]


def _tiles(v, t):
    """How many tiles the tile cutter makes of this mesh (tetsim_prep_tiles, host only)."""
    L, n = capi.lib(), C.c_uint32()
    vv, tt = np.ascontiguousarray(v, np.float32).ravel(), np.ascontiguousarray(t, np.int32).ravel()
    assert L.tetsim_prep_tiles(vv.ctypes.data_as(C.POINTER(C.c_float)), len(vv) // 3, tt.ctypes.data_as(C.POINTER(C.c_int32)), len(tt) // 4,
                               None, None, 0, None, None, None, C.byref(n)) == 0
    return n.value


@functools.lru_cache(maxsize=1)
def _delaunay():
    """604,715 tets over 90,000 particles (the default min_vol drops most tets at this density), 1 cm above the floor."""
    v, t = random_mesh(11, 90000, min_vol=2e-9)
    v = v.copy()
    v[:, 1] -= v[:, 1].min() - np.float32(0.01)
    return v, t


def _partial_lists(v, t):
    """Per particle, how many tiles touch it: the length of its partial-sum list."""
    L, n = capi.lib(), C.c_uint32()
    nt = len(t)
    vv, tt = np.ascontiguousarray(v, np.float32).ravel(), np.ascontiguousarray(t, np.int32).ravel()
    tile_tets, off, slot = np.empty(nt, np.int32), np.empty(nt + 1, np.uint32), np.empty(4 * nt, np.uint8)
    assert L.tetsim_prep_tiles(vv.ctypes.data_as(C.POINTER(C.c_float)), len(v), tt.ctypes.data_as(C.POINTER(C.c_int32)), nt, None, None, 0,
                               tile_tets.ctypes.data_as(C.POINTER(C.c_int32)), off.ctypes.data_as(C.POINTER(C.c_uint32)),
                               slot.ctypes.data_as(C.POINTER(C.c_uint8)), C.byref(n)) == 0
    tile_of = np.repeat(np.arange(n.value), np.diff(off[:n.value + 1]).astype(np.int64))
    pairs = np.unique(np.stack([t[tile_tets].ravel(), np.repeat(tile_of, 4)], axis=1), axis=0)
    return n.value, np.bincount(pairs[:, 0], minlength=len(v))


def test_large_delaunay_body_against_the_oracle():
    """Mode 5 under the oracle on an irregular mesh: ragged tiles, nb % 8 == 3, partial-sum lists of up to 40 (the 8-wide gather's fifth
    round), valences of up to 92 (the reference's 36-slot table drops the rest, and so must the body), floor contact from the start."""
    v, t = _delaunay()
    nb, lists = _partial_lists(v, t)
    valence = np.bincount(t.ravel(), minlength=len(v))
    assert nb % 8 == 3 and lists.max() > 24 and (lists > 8).sum() > 100 and valence.max() > 36
    body = _polar(v, t)
    assert body.info.fused_particle_pass == 5
    orc = OraclePJ(v, t, PP, slot_quirk=True)
    # the cap drops every contribution past the 36th; the slot-0 quirk drops one more only where the particle of tet 0's first corner keeps
    # its row within the cap -- here it has 62 tets, and a 37th contribution takes the slot the quirk frees
    quirk = 1 if 1 < valence[t[0, 0]] <= 36 else 0
    assert valence[t[0, 0]] > 36
    assert body.info.dropped_slots == int(np.maximum(valence - 36, 0).sum()) + quirk == 4 * len(t) - int((orc.slots >= 0).sum())
    done = 0
    for upto, tol in ((1, 2e-6), (20, 5e-5), (60, 5e-4)):
        body.simulateSubsteps(upto - done, DT, PP)              # one call: 1, 19, 40 substeps
        for _ in range(upto - done):
            orc.simulate(DT, PP)
        done = upto
        within("polar fast one-launch call delaunay 90k vs oracle @%d" % upto, np.abs(body.pos - orc.pos).max(), tol)
    assert body.pos[:, 1].min() == 0.0                          # contact was part of it


@pytest.mark.parametrize("kw", [dict(), dict(lean_state=True), dict(constant_rest_shape=True)])
def test_large_delaunay_body_equals_its_two_kernel_twins(kw):
    """Same arithmetic as the tet kernel + particle kernel pair: bit for bit, through calls of 20, 1, 7, 3 (2 x dt) and 20, a grab set and
    released -- against the TETSIM_PJ_ONE_LAUNCH=0 twin, and (carried record) against eager tetsim_step.  Partial-sum lists of up to 40, and
    tiles that stage a particle whose every contribution in them the 36-slot table dropped: the particle's lane must wait for those too
    before it overwrites the prediction they stage (their zero sums are on its list: host_prep.cpp)."""
    v, t = _delaunay()
    v = v - np.float32([0.0, 0.008, 0.0])                      # 2 mm above the floor: contact within these 51 substeps
    a, b = _polar(v, t, **kw), _polar(v, t, one_launch=False, **kw)
    c = _polar(v, t, one_launch=False, **kw) if not kw else None   # (tetsim_step is the pair whatever the environment said)
    assert a.info.fused_particle_pass == 5 and b.info.fused_particle_pass == 0
    bodies = [x for x in (a, b, c) if x is not None]
    for k, (n, dt) in enumerate(CALLS):
        if k == 2:
            for x in bodies:
                x.setGrab(11, [0.1, 0.5, -0.1])
        if k == 4:
            for x in bodies:
                x.endGrab()
        a.simulateSubsteps(n, dt, PP)
        b.simulateSubsteps(n, dt, PP)
        if c is not None:
            for _ in range(n):
                c.simulate(dt, PP)
        for x in bodies[1:]:
            assert _same(a.pos, x.pos) and _same(a.vel, x.vel), (kw, k)
    for x in bodies[1:]:
        assert _same(a.quats, x.quats), kw
    assert np.isfinite(a.pos).all() and a.pos[:, 1].min() == 0.0


# (seed, points, tiles % 8, particles % 256) -- the particle count includes the loose particle
SMALL = [(30, 1280, 0, 1), (31, 2302, 1, 255), (32, 2560, 7, 1), (30, 4352, 7, 255), (33, 4096, 1, 1)]


def _loose(seed, npts):
    v, t = random_mesh(seed, npts)
    return np.concatenate([v, [LOOSE]]).astype(np.float32), t


@pytest.mark.parametrize("seed,npts,nb8,nv256", SMALL)
def test_small_irregular_bodies_forced_into_one_launch(seed, npts, nb8, nv256):
    """A particle no tet references keeps a body of any size on the kernel pair, whose calls are one launch: every substep's workgroups
    resident at once.  Tile counts with nb % 8 = 0, 1, 7 (padded tile blocks that must return), particle counts just above and just below
    a multiple of 256 (a last particle workgroup of one lane, or of 255).  The loose particle's row is no parity evidence and is left out:
    device and oracle both divide 0 / 0 there, and the oracle's fmaxf / fminf world clamp turns the NaN into a bound -- GLSL leaves clamp of
    a NaN undefined."""
    v, t = _loose(seed, npts)
    assert _tiles(v, t) % 8 == nb8 and len(v) % 256 == nv256 and 1000 <= len(t) <= 30000
    a, b = _polar(v, t), _polar(v, t, one_launch=False)
    assert a.info.fused_particle_pass == 5 and b.info.fused_particle_pass == 0
    orc = OraclePJ(v, t, PP, slot_quirk=True)
    done = 0
    for upto, tol in ((1, 2e-6), (20, 5e-5), (60, 5e-4)):
        a.simulateSubsteps(upto - done, DT, PP)
        b.simulateSubsteps(upto - done, DT, PP)
        for _ in range(upto - done):
            orc.simulate(DT, PP)
        done = upto
        pa = a.pos[:-1]
        assert _same(pa, b.pos[:-1]) and _same(a.vel[:-1], b.vel[:-1]), (seed, npts, upto)
        within("polar fast one-launch call loose-particle delaunay vs oracle @%d" % upto, np.abs(pa - orc.pos[:-1]).max(), tol)
    assert np.isfinite(a.pos[:-1]).all()


def test_batch_with_a_large_irregular_body_equals_the_solo_runs():
    """A batch of the 90 k-point Delaunay body and a 3,000-point one runs as one launch per call (mode 5); each body equals its solo run bit
    for bit -- the large one solo in mode 5, the small one solo in a persistent frame kernel (mode 2 or 3)."""
    meshes = [_delaunay(), random_mesh(6, 3000)]
    batch = SoftBodyHIP.batch(meshes, dict(PP), solver="polar", precision="fast")
    solos = [_polar(v, t) for v, t in meshes]
    assert batch.info.fused_particle_pass == 5 and solos[0].info.fused_particle_pass == 5 and solos[1].info.fused_particle_pass in (2, 3)
    for n in (20, 1, 9):
        for x in [batch] + solos:
            x.simulateSubsteps(n, DT, PP)
    pos, vel = batch.pos, batch.vel
    for ((p0, p1), _), solo in zip(batch.bodyRanges, solos):
        assert _same(pos[p0:p1], solo.pos) and _same(vel[p0:p1], solo.vel)


# ---- checkpoints --------------------------------------------------------------------------------------------------------------------
def _state_bodies(mesh):
    if mesh == "lattice46":
        return make_lattice(46, y0=0.01)                        # 584,016 tets = 2,282 tiles
    return _loose(31, 2302)


@pytest.mark.parametrize("mesh", ["lattice46", "loose"])
@pytest.mark.parametrize("kw", [dict(), dict(lean_state=True)])
def test_checkpoints_of_one_launch_bodies(mesh, kw):
    """tetsim_save_state / _load_state of a mode-5 body.  The call leaves stamps in pos_pred.w and pos_final.w, and every body numbers its
    calls from the same start: a restored stamp would pass for a fresh one in the body that loads it, whose waves could then take the blob's
    predictions before this call's substep 0 wrote them.  So (1) the blob holds none: it equals its two-kernel twin's byte for byte;
    (2) a fresh body, and one that made as many calls as the saver, continue from it as the saver and the twin do; (3) blobs cross between
    the two paths in both directions."""
    v, t = _state_bodies(mesh)
    a, b = _polar(v, t, **kw), _polar(v, t, one_launch=False, **kw)
    assert a.info.fused_particle_pass == 5 and b.info.fused_particle_pass == 0
    # (1) the same calls, the same blob
    for n in (7, 1, 12):
        a.simulateSubsteps(n, DT, PP)
        b.simulateSubsteps(n, DT, PP)
    blob_a, blob_b = a.saveState(), b.saveState()
    assert len(blob_a) == len(blob_b) and blob_a == blob_b, (mesh, kw)
    # (3) across the paths: the mode-5 blob into a two-kernel body, the two-kernel blob into a mode-5 body
    a2, b2 = _polar(v, t, **kw), _polar(v, t, one_launch=False, **kw)
    a2.loadState(blob_b)
    b2.loadState(blob_a)
    for x in (a, b, a2, b2):
        x.simulateSubsteps(10, DT, PP)
    for x in (b, a2, b2):
        assert _same(a.pos, x.pos) and _same(a.vel, x.vel), (mesh, kw)
    # (2) the saver made one call of one substep; a fresh body, and one after one call of its own, load its blob and make a call of ten
    s, twin = _polar(v, t, **kw), _polar(v, t, one_launch=False, **kw)
    s.simulateSubsteps(1, DT, PP)
    twin.simulateSubsteps(1, DT, PP)
    blob = s.saveState()
    fresh, used = _polar(v, t, **kw), _polar(v, t, **kw)
    used.simulateSubsteps(1, DT, PP)
    fresh.loadState(blob)
    used.loadState(blob)
    for x in (s, twin, fresh, used):
        x.simulateSubsteps(10, DT, PP)
    for x in (twin, fresh, used):
        assert _same(s.pos, x.pos) and _same(s.vel, x.vel), (mesh, kw)
    assert _same(s.quats, fresh.quats) and _same(s.quats, used.quats)


def test_checkpoint_of_a_clustered_one_launch_neohookean_body():
    """The clustered FAST Neo-Hookean call as one launch (nh_kernels.inc: nh_call_kernel): a fresh body that loads the blob continues
    bit for bit."""
    v, t = load_mesh("dragon")
    v = v - np.float32([0.0, v[:, 1].min() - 0.01, 0.0])
    kw = dict(solver="neohookean", precision="fast", order="clustered")
    a = SoftBodyHIP(v, t, None, dict(PP), **kw)
    for n in (10, 3):
        a.simulateSubsteps(n, DT * 2, PP)
    blob = a.saveState()
    b = SoftBodyHIP(v, t, None, dict(PP), **kw)
    b.loadState(blob)
    for n in (5, 1, 12):
        a.simulateSubsteps(n, DT * 2, PP)
        b.simulateSubsteps(n, DT * 2, PP)
        assert _same(a.pos, b.pos) and _same(a.vel, b.vel) and a.volError == b.volError, n
    assert a.pos[:, 1].min() == 0.0


# ---- long calls ---------------------------------------------------------------------------------------------------------------------
def test_long_polar_call_is_chunked_inside_the_dispatch_limit():
    """One call of 8,192 substeps on a body of 2,696 blocks per substep is 22 M workgroups of 256 lanes: more work-items than a dispatch
    holds.  It is cut into launches that fit and equals the same substeps in calls of 20, bit for bit."""
    v, t = make_lattice(46, y0=0.01)
    a, b = _polar(v, t), _polar(v, t)
    assert a.info.fused_particle_pass == 5
    nb = _tiles(v, t)
    per_sub = ((((nb + 7) // 8 * 8) + (len(v) + 255) // 256) + 7) // 8 * 8
    assert nb == 2282 and per_sub == 2696 and per_sub * 8192 * 256 > GRID_ITEMS
    n = 8192
    a.simulateSubsteps(n, DT, PP)
    for _ in range(n // 20):
        b.simulateSubsteps(20, DT, PP)
    b.simulateSubsteps(n % 20, DT, PP)
    assert _same(a.pos, b.pos) and _same(a.vel, b.vel) and np.isfinite(a.pos).all()


def _cluster_blocks(t, nv):
    """Workgroups of one substep of the clustered one-launch sweep: per colour, its clusters in workgroups of 64 (tetsim_create.hip)."""
    L = capi.lib()
    nt = len(t)
    out = [np.full(nt, -1, np.int32) for _ in range(4)]
    nl, nc = C.c_uint32(), C.c_uint32()
    ip = lambda a: a.ctypes.data_as(C.POINTER(C.c_int32))
    assert L.tetsim_prep_clusters(ip(np.ascontiguousarray(t, np.int32).ravel()), nt, nv, *[ip(a) for a in out], C.byref(nl), C.byref(nc)) == 0
    _, launch, lane, _ = out
    return nl.value, sum((int(lane[launch == l].max()) + 1 + 63) // 64 for l in range(nl.value))


def test_long_neohookean_call_is_chunked_inside_the_dispatch_limit():
    """The clustered FAST Neo-Hookean one-launch call stamps substep x colour inside one block of 65,536 numbers, so a call is cut at
    65,000 // colours substeps -- and on the 55-cell lattice that many substeps of 2,608 workgroups are more work-items than a dispatch
    holds.  One call of 8,125 substeps equals calls of 25, bit for bit."""
    v, t = make_lattice(55, y0=0.01)
    colours, blocks = _cluster_blocks(t, len(v))
    per_sub = (blocks + 7) // 8 * 8
    assert colours == 8 and blocks == 2601 and per_sub * (65000 // colours) * 256 > GRID_ITEMS
    kw = dict(solver="neohookean", precision="fast", order="clustered")
    a, b = SoftBodyHIP(v, t, None, dict(PP), **kw), SoftBodyHIP(v, t, None, dict(PP), **kw)
    assert a.info.num_levels == colours
    n = 65000 // a.info.num_levels
    a.simulateSubsteps(n, DT, PP)
    for _ in range(n // 25):
        b.simulateSubsteps(25, DT, PP)
    assert n % 25 == 0 and _same(a.pos, b.pos) and _same(a.vel, b.vel) and np.isfinite(a.pos).all()
