"""The clustered FAST Neo-Hookean sweep as one launch (nh_kernels.inc: nh_sweep1_kernel, one launch per substep; nh_call_kernel, one launch
per call) where lattices do not reach: irregular meshes, ragged colours, free particles, the colour counts at which the creation code
changes path, checkpoints, and the stamps themselves.

tetsim_create.hip picks the path: the call kernel for bodies whose every particle some tet touches and that have 2..127 colours (its
8-bit hand-over distances reach back up to 2 x colours - 1), the one-launch sweep for up to 255 colours, one launch per colour beyond.
Every hand-over carries a stamp (tetsim_api.hip: next_epoch_block), and the call kernel also polls prev.w for its own fold's stamp of
one substep before -- a lane where the prediction used to leave the inverse mass, whose bits can equal a stamp.
TETSIM_NH_ONE_LAUNCH=0 (read at creation) keeps one launch per colour with the same arithmetic: the twin of every test here."""
import math
import os

import numpy as np
import pytest

from conftest import within
from oracle import OracleNH
from tetsim_amd import SoftBodyHIP, make_lattice
from test_capi_cpu import STAMP_BITS, STAMP_DENSITY
from test_cluster_plan import FANS, fan
from test_gpu_call_kernel_irregular import _delaunay
from test_gpu_random_meshes import random_mesh

pytestmark = pytest.mark.gpu
PP = dict(gravity=-9.81, friction=1000.0, density=1000.0, devCompliance=1e-5, volCompliance=0.0,
          worldBounds=[-2.5, -1.0, -2.5, 2.5, 10.0, 2.5])
DT = (1.0 / 60.0) / 20
NH = dict(solver="neohookean", precision="fast", order="clustered")
CALLS = ((20, DT), (1, DT), (7, DT), (3, DT * 2), (20, DT))    # a grab from the third call to the fifth; calls 2 and 4 through tetsim_step
SOFT = dict(PP, devCompliance=1e-3)
FREE = [[0.1, 2.0, 0.1], [-0.3, 1.2, 0.2], [0.25, 0.9, -0.3]]   # particles no tet references


def _same(a, b):
    return np.array_equal(np.asarray(a).view(np.uint32), np.asarray(b).view(np.uint32))


def _nh(v, t, one_launch=True, pp=PP, **kw):
    args = dict(NH, **kw)
    if one_launch:
        return SoftBodyHIP(v, t, None, dict(pp), **args)
    os.environ["TETSIM_NH_ONE_LAUNCH"] = "0"
    try:
        return SoftBodyHIP(v, t, None, dict(pp), **args)
    finally:
        del os.environ["TETSIM_NH_ONE_LAUNCH"]


def _equal(a, b):
    return _same(a.pos, b.pos) and _same(a.vel, b.vel) and a.volError == b.volError


def _against_oracle(label, bodies, orc, free=0, pp=PP):
    """Calls of 1, 19 and 40 substeps: every body inside the FAST envelope around the sequential oracle, volError too."""
    done = 0
    for upto, tol in ((1, 2e-6), (20, 5e-5), (60, 5e-4)):
        for x in bodies:
            x.simulateSubsteps(upto - done, DT, pp)
        for _ in range(upto - done):
            orc.simulate(DT, pp)
        done = upto
        for x in bodies:
            within("%s @%d" % (label, upto), np.abs(x.pos - orc.pos).max(), tol)
            within("%s volError @%d" % (label, upto), abs(x.volError - orc.volError) / abs(orc.volError), 1e-2)
            if free:
                within("neo-hookean fast free particles vs oracle @%d" % upto, np.abs(x.pos[-free:] - orc.pos[-free:]).max(), 1e-5)
        for x in bodies[1:]:
            assert _equal(bodies[0], x), (label, upto)


def test_large_delaunay_body_against_the_oracle():
    """604,715 tets in 35 colours of 1 to ~6 k clusters, 1 cm above the floor: the call kernel against the oracle on the permuted tets."""
    v, t = _delaunay()
    body = _nh(v, t)
    assert body.info.num_levels == 35
    orc = OracleNH(v, t[body.tetOrder], PP)
    _against_oracle("neo-hookean fast one-launch call delaunay 90k vs oracle", [body], orc)
    assert body.pos[:, 1].min() == 0.0                          # contact was part of it


def test_large_delaunay_body_equals_its_twin():
    """Calls of 20, 1, 7, 3 (2 x dt) and 20 substeps, a grab set and released; the calls of 1 and 3 go through tetsim_step (the one-launch
    sweep with the folded particle pass), the others through the call kernel -- bit for bit against one launch per colour."""
    v, t = _delaunay()
    v = v - np.float32([0.0, 0.008, 0.0])                      # 2 mm above the floor: contact within these 51 substeps
    a, b = _nh(v, t), _nh(v, t, one_launch=False)
    for k, (n, dt) in enumerate(CALLS):
        if k == 2:
            for x in (a, b):
                x.setGrab(11, [0.1, 0.5, -0.1])
        if k == 4:
            for x in (a, b):
                x.endGrab()
        if k in (1, 3):
            for _ in range(n):
                a.simulate(dt, PP)
        else:
            a.simulateSubsteps(n, dt, PP)
        b.simulateSubsteps(n, dt, PP)
        assert _equal(a, b), k
    assert np.isfinite(a.pos).all() and a.pos[:, 1].min() == 0.0


SMALL = [(1, 60), (2, 400), (6, 3000)]


@pytest.mark.parametrize("seed,npts", SMALL)
def test_small_ragged_delaunay_bodies(seed, npts):
    """Delaunay bodies of 11 to 27 colours, some of one to five clusters: the call kernel equals its twin and stays inside the envelope;
    the FAST single-workgroup frame kernel (original and coloured orders, TetSimInfo.fused_particle_pass == 4) against the oracle too."""
    v, t = random_mesh(seed, npts)
    a, b = _nh(v, t), _nh(v, t, one_launch=False)
    assert 2 <= a.info.num_levels <= 127 and np.unique(t).size == len(v)     # the call kernel's body
    _against_oracle("neo-hookean fast one-launch call small delaunay vs oracle", [a, b], OracleNH(v, t[a.tetOrder], PP))
    for order in ("original", "coloured"):
        c = _nh(v, t, order=order)
        assert c.info.fused_particle_pass == 4
        _against_oracle("neo-hookean fast frame kernel small delaunay vs oracle", [c], OracleNH(v, t[c.tetOrder], PP))


@pytest.mark.parametrize("seed,npts", [(2, 400), (6, 3000)])
def test_free_particles(seed, npts):
    """Particles no tet references keep a body off the call kernel: the one-launch sweep per substep, the free particles on the untouched
    list of the particle pass between two substeps.  Bit-equal to the twin, inside the envelope, and the free particles fall as the
    oracle's do."""
    v, t = random_mesh(seed, npts)
    v = np.concatenate([v, FREE]).astype(np.float32)
    a, b = _nh(v, t), _nh(v, t, one_launch=False)
    assert 2 <= a.info.num_levels <= 255 and np.unique(t).size == len(v) - len(FREE)
    _against_oracle("neo-hookean fast one-launch sweep free-particle delaunay vs oracle", [a, b], OracleNH(v, t[a.tetOrder], PP), free=len(FREE))
    assert (a.pos[-len(FREE):, 1] < np.float32(FREE)[:, 1]).all()


@pytest.mark.parametrize("m,colours", FANS)
def test_colour_edges(m, colours):
    """Fans of 127 (call kernel), 128 and 255 (one-launch sweep) and 256 colours (one launch per colour: its twin is the same path, and
    it is held to the oracle).  Mixed calls, then one call that crosses the 65,000 // colours chunk, then a mixed tail.  A fan's tets are
    slivers (a dihedral angle of 2 pi / m at the shared edge) whose stiff solve amplifies FAST's rounding: the bodies here are soft."""
    v, t = fan(m)
    a, b = _nh(v, t, pp=SOFT), _nh(v, t, one_launch=False, pp=SOFT)
    assert a.info.num_levels == b.info.num_levels == colours
    if colours == 256:
        _against_oracle("neo-hookean fast soft fan 256 colours vs oracle", [a, b], OracleNH(v, t[a.tetOrder], SOFT), pp=SOFT)
    for k, n in enumerate((20, 1, 7, 65000 // colours + 9, 3, 1, 2)):
        if k == 1:
            a.simulate(DT, SOFT)
        else:
            a.simulateSubsteps(n, DT, SOFT)
        b.simulateSubsteps(n, DT, SOFT)
        assert _equal(a, b), (m, n)
    assert np.isfinite(a.pos).all()


@pytest.mark.parametrize("mesh", ["delaunay400", "fan128"])
def test_checkpoints_across_bodies(mesh):
    """Body A makes a call of 5 substeps and saves; its blob equals the blob of its twin after the same calls byte for byte (no stamp in
    it: prev.w is 0 there).  A fresh body and a fresh twin load it; all three continue through tetsim_step_n and tetsim_step, bit for bit."""
    v, t = random_mesh(2, 400) if mesh == "delaunay400" else fan(636)
    a, twin = _nh(v, t), _nh(v, t, one_launch=False)
    for x in (a, twin):
        x.simulateSubsteps(5, DT, PP)
    blob = a.saveState()
    assert blob == twin.saveState(), mesh
    fresh, fresh_twin = _nh(v, t), _nh(v, t, one_launch=False)
    fresh.loadState(blob)
    fresh_twin.loadState(blob)
    bodies = (a, fresh, fresh_twin)
    for n in (4, 1, 9, 3):
        for x in bodies:
            if n == 1:
                x.simulate(DT, PP)
            else:
                x.simulateSubsteps(n, DT, PP)
        assert _equal(a, fresh) and _equal(a, fresh_twin), (mesh, n)


def _drag(bodies, gid, call):
    """The grabbed corner particle on a circle: the body never comes to rest."""
    phi = 0.05 * call
    for x in bodies:
        x.setGrab(gid, [0.3 + 0.1 * math.cos(phi), 0.6, 0.3 + 0.1 * math.sin(phi)])


def test_stamp_in_the_inverse_mass_lane():
    """The 3-cell lattice at STAMP_DENSITY: its eight inner particles have the inverse mass 0x3F800009, which is the stamp the call kernel
    waits for in prev.w at substep 2 of the 16,256th tetsim_step_n call (block 0x3F80: tests/test_capi_cpu.py).  Before the fold's
    store lands, the lane holds what the call's prediction left there; when that was the inverse mass, the first toucher took the
    position from the start of the call as the previous one.  Every call has 3 substeps; the twin never polls prev."""
    v, t = make_lattice(3, y0=0.3)
    pp = dict(PP, density=STAMP_DENSITY)
    a, b = _nh(v, t, pp=pp), _nh(v, t, one_launch=False, pp=pp)
    assert a.info.num_levels == 8 and (a.invMass.view(np.uint32) == STAMP_BITS).sum() == 8
    colliding = 16256
    for call in range(1, colliding + 8):
        _drag((a, b), len(v) - 1, call)
        a.simulateSubsteps(3, DT, pp)
        b.simulateSubsteps(3, DT, pp)
        if call % 2000 == 0 or call >= colliding - 2:
            assert _equal(a, b), call
    assert np.isfinite(a.pos).all()


def test_epoch_wrap():
    """Past 65,535 blocks of stamps the exchange array is wiped and the count restarts (next_epoch_block): a call-kernel body and its twin
    stay bit-equal through it."""
    v, t = make_lattice(2, y0=0.3)
    a, b = _nh(v, t), _nh(v, t, one_launch=False)
    assert a.info.num_levels == 8
    wrap = 65535                                                # the call whose block restarts the count
    for call in range(1, wrap + 6):
        if call % 7 == 0:
            _drag((a, b), len(v) - 1, call)
        n = 3 if call >= wrap - 3 or call % 1000 == 0 else 1
        a.simulateSubsteps(n, DT, PP)
        b.simulateSubsteps(n, DT, PP)
        if call % 16384 == 0 or call >= wrap - 3:
            assert _equal(a, b), call
    assert np.isfinite(a.pos).all()
