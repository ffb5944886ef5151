"""The reads and writes of the state, anchored to data that never went through them.  The pinned reads, the visual mesh's reads and
the device export run ONE gather kernel (device_io.hip), so the tests that compare them with each other compare a kernel with
itself; the copying particle reads and tetsim_write_state permute on the host.  Here the other side of every comparison is the
caller's own input (the upload at creation permutes in its own loop), a checkpoint, the CPU oracle, or a golden recorded from the
reference.  Every comparison is on the bits."""
import numpy as np
import pytest

from conftest import load_f32, load_mesh, sha16
from oracle import OracleNH
from test_gpu_partition_state import _group, _slab_owner
from test_gpu_skinning import PP
from tetsim_amd import SoftBodyHIP

pytestmark = pytest.mark.gpu
DT = (1.0 / 60.0) / 20

BODIES = {
    "dragon-polar-fast": ("dragon", dict(solver="polar", precision="fast")),
    "dragon-polar-precise": ("dragon", dict(solver="polar", precision="precise")),
    "dragon-nh-precise-coloured": ("dragon", dict(solver="neohookean", precision="precise", order="coloured")),
    "lat4-polar-fast": ("lat4", dict(solver="polar", precision="fast")),
    "tetless-polar-fast": ("notets", dict(solver="polar", precision="fast")),
}


def mesh(name):
    v, t = load_mesh(name)
    return v, (np.zeros((0, 4), np.int32) if name == "notets" else t)


def bits(a):
    return np.ascontiguousarray(a, dtype=np.float32).view(np.uint32)


def device_order_positions(body):
    """The positions in the DEVICE's particle order: the first section of a polar body's checkpoint (tetsim_state.hip: a 64-byte
    header, then pos_final as float4 rows).  The API has no getter for the internal order; the blob is the one place where it
    shows, and its layout is private: if it changes, the permutation check below fails loudly and this offset follows it."""
    n = body.info.local_particles
    return np.frombuffer(body.saveState(), dtype="<f4", count=4 * n, offset=64).reshape(n, 4)[:, :3]


@pytest.mark.parametrize("name", list(BODIES))
def test_a_fresh_body_reads_back_the_callers_vertices(name):
    v, t = mesh(BODIES[name][0])
    body = SoftBodyHIP(v, t, None, dict(PP), **BODIES[name][1])
    assert body.info.owned_particles == len(v) > 0
    if name.startswith("dragon-polar"):   # not vacuous: the device holds the rows in another order than the caller's
        dev = device_order_positions(body)
        assert not np.array_equal(bits(dev), bits(v))
        assert np.array_equal(bits(dev[np.lexsort(dev.T)]), bits(v[np.lexsort(v.T)]))
    assert np.array_equal(bits(body.pos), bits(v))
    assert np.array_equal(bits(body.posPinned), bits(v))
    assert not bits(body.vel).any()


@pytest.mark.parametrize("name,parts", [("lat4", 2), ("dragon", 3)])
def test_a_fresh_partition_reads_back_its_owned_vertices(name, parts):
    v, t = load_mesh(name)
    owner = _slab_owner(len(v), 4, parts) if name == "lat4" else None   # the Dragon: the library's partitioner, ragged cuts
    bodies = _group(v, t, parts, owner, "fast")
    ids = [b.ownedIds for b in bodies]
    assert np.array_equal(np.sort(np.concatenate(ids)), np.arange(len(v)))
    for b, own in zip(bodies, ids):
        assert 0 < len(own) < len(v)
        assert np.array_equal(bits(b.pos), bits(v[own]))
        assert np.array_equal(bits(b.posPinned), bits(v[own]))
        assert not bits(b.vel).any()


def seeded_state(v, seed):
    """Positions near the mesh; velocities whose 3n components all differ in their bits (a swapped row or component shows)."""
    rng = np.random.default_rng(seed)
    pos = (v + rng.normal(0.0, 0.003, v.shape) + [0.0, 0.25, 0.0]).astype(np.float32)
    vel = ((np.arange(v.size, dtype=np.float32).reshape(v.shape) + 1.0) * np.float32(2.0 ** -15)).astype(np.float32)
    assert len(np.unique(bits(vel))) == vel.size
    return pos, rng.permutation(vel)      # (rows shuffled: no monotone pattern a sort could restore)


@pytest.mark.parametrize("name,kw", [("dragon", dict(solver="polar", precision="fast")),
                                     ("lat4", dict(solver="neohookean", precision="precise", order="original"))])
def test_a_written_state_reads_back_and_steps_like_a_restored_one(name, kw):
    v, t = load_mesh(name)
    a = SoftBodyHIP(v, t, None, dict(PP), **kw)
    a.simulateSubsteps(5, DT, PP)                    # (not a pristine state: velocities, a prediction made for DT)
    inv_mass = a.invMass
    pos, vel = seeded_state(v, 11)
    a.writeState(pos, vel)
    assert np.array_equal(bits(a.pos), bits(pos)) and np.array_equal(bits(a.vel), bits(vel))
    assert np.array_equal(bits(a.posPinned), bits(pos))
    assert np.array_equal(bits(a.invMass), bits(inv_mass))     # (the host's copy: it cannot see a pos.w lost on the device -- the oracle below can)
    twin = SoftBodyHIP(v, t, None, dict(PP), **kw)
    twin.loadState(a.saveState())
    a.simulate(DT, PP)
    twin.simulate(DT, PP)
    assert np.array_equal(bits(a.pos), bits(twin.pos)) and np.array_equal(bits(a.vel), bits(twin.vel))   # (the blob was saved AFTER the write: this pins the checkpoint, not pos.w)
    assert not np.array_equal(bits(a.pos), bits(pos))
    if kw["solver"] == "neohookean":
        # ... and like the CPU oracle handed the same numbers (PRECISE in the original order equals it bit for bit, test_gpu_neohookean.py).
        # Its inverse masses never left the host: a position row that lost its fourth float on the way in would stay where it is.
        orc = OracleNH(v, t, PP)
        n = 3 * len(v)
        np.ctypeslib.as_array(orc._lib.orc_nh_pos(orc._h), shape=(n,))[:] = pos.ravel()
        np.ctypeslib.as_array(orc._lib.orc_nh_vel(orc._h), shape=(n,))[:] = vel.ravel()
        orc.simulate(DT, PP)
        assert (inv_mass > 0).all()
        assert np.array_equal(bits(a.pos), bits(orc.pos)) and np.array_equal(bits(a.vel), bits(orc.vel))


def test_visual_rows_equal_the_reference_goldens(golden):
    """The Dragon's 29,800 visual vertices after 10 substeps, positions and three.js vertex normals from ONE body: the goldens and
    the rule (bit for bit, Neo-Hookean PRECISE) of test_gpu_skinning.py, through the shared read."""
    import os
    from conftest import GOLDEN
    v, t = load_mesh("dragon")
    vis = load_f32("dragon_vis.f32").reshape(-1, 4)
    tris = np.fromfile(os.path.join(GOLDEN, "dragon_vistris.u16"), dtype="<u2").astype(np.int32).reshape(-1, 3)
    body = SoftBodyHIP(v, t, None, dict(PP), vis, tris, solver="neohookean", precision="precise")
    for _ in range(10):
        body.simulate((1.0 / 60.0) / 10, PP)
    pos, nrm = body.visualPositions(), body.visualVertexNormals()
    assert np.array_equal(bits(pos), bits(load_f32("dragon_vispos_10.f32").reshape(-1, 3))) and sha16(pos) == "8df79c236ba69d61"
    assert np.array_equal(bits(nrm), bits(load_f32("dragon_visnormal_10.f32").reshape(-1, 3))) and sha16(nrm) == "77a1f9768ab27ed3"
