"""The LAYOUT of a checkpoint (tetsim_state.hip: state_sections): which section stands where in a saveState() blob, how large it is, and
that no call's sequence number travels in it.  The other state tests compare blobs with blobs or with snapshots, by round trip, which a
reordered or resized section table would survive; here a blob is taken apart and compared, on bits, with what the host readers return.

Behind the 64-byte header, Neo-Hookean: [nv] float4 pos (w = inverse mass) | [nv] float4 prevPos (w = 0) | [nv] float4 vel | [nt] f64
volError terms.  Polar: [nvl] float4 end-of-substep positions (w = 0) | [nvl] float4 vel | [nvl] float4 predictions (w = 0) | [nt] float4
quaternions | the carried shape: 3 x [nt] float4, lean state 2 x [nt] float4 + [nt] float, constant rest shape nothing, gather
formulation four float4 planes of nt rounded up.  Polar particles are renumbered on the device, so their rows compare as multisets.
Meshes: lat4; lat4 without its last three tets plus one unreferenced particle (381 tets: the 4- and 8-byte sections end in a short
16-byte unit, polar-fast takes the one-launch call); lat4 + lat12 as one batch."""
import numpy as np
import pytest

from tetsim_amd import SoftBodyHIP
from test_gpu_device_io import DT, PP, WIDE
from test_gpu_snapshot import HEADER, KINDS, SHIFTS, bits, mesh, show, solo

pytestmark = pytest.mark.gpu
PAIR = ("lat4", "lat12")
SHAPE_BYTES = {"polar-fast": lambda nt: 3 * 16 * nt, "polar-fast-lean": lambda nt: 2 * 16 * nt + 4 * nt, "polar-fast-constant-rest": lambda nt: 0}


def make(name, kind):
    """(body, its parameters, a solo twin of every body or None)."""
    if name != "pair":
        return solo(name, kind), PP, None
    shifted = [((mesh(n)[0] + np.array([s, 0, 0], np.float32)).astype(np.float32), mesh(n)[1]) for n, s in zip(PAIR, SHIFTS)]
    return SoftBodyHIP.batch(shifted, dict(WIDE), ref_fixed_bounds=False, **KINDS[kind]), WIDE, [solo(n, kind, s) for n, s in zip(PAIR, SHIFTS)]


def sorted_rows(a):
    """The rows of an [n, 3] array of bits in one canonical order: equal multisets give equal arrays."""
    a = np.ascontiguousarray(a)
    return a[np.lexsort(a.T[::-1])]


def take(blob, at, rows, dtype, width):
    n = rows * width * np.dtype(dtype).itemsize
    assert at + n <= len(blob), "the blob ends inside a section"
    return np.frombuffer(blob, dtype=dtype, count=rows * width, offset=at).reshape(rows, width), at + n


@pytest.mark.parametrize("name", ["lat4", "loose", "pair"])
@pytest.mark.parametrize("kind", list(KINDS))
def test_a_blob_holds_what_the_host_readers_return(kind, name):
    body, pp, twins = make(name, kind)
    show("%s %s" % (kind, name), body)
    if kind == "polar-fast" and name == "loose":
        assert body.info.fused_particle_pass == 5
    body.simulateSubsteps(7, DT, pp)
    blob = body.saveState()
    nv, nt = body.info.num_particles, body.info.num_elems
    at = HEADER
    if body.solver == "neohookean":
        pos, at = take(blob, at, nv, np.uint32, 4)
        prev, at = take(blob, at, nv, np.uint32, 4)
        vel, at = take(blob, at, nv, np.uint32, 4)
        ve, at = take(blob, at, nt, np.float64, 1)
        assert np.array_equal(pos[:, :3], bits(body.pos)) and np.array_equal(pos[:, 3], bits(body.invMass))
        assert np.array_equal(prev[:, :3], bits(body.prevPos)) and not prev[:, 3].any()
        assert np.array_equal(vel[:, :3], bits(body.vel))
        total = 0.0
        for term in ve[:, 0]:   # (element order, one rounding per term, as tetsim_read_vol_error sums)
            total += float(term)
        assert total / nt == body.volError
        assert at == len(blob) == HEADER + 48 * nv + 8 * nt
    else:
        nvl = body.info.local_particles
        pos, at = take(blob, at, nvl, np.uint32, 4)
        vel, at = take(blob, at, nvl, np.uint32, 4)
        pred, at = take(blob, at, nvl, np.uint32, 4)
        quats, at = take(blob, at, nt, np.uint32, 4)
        assert np.array_equal(sorted_rows(pos[:, :3]), sorted_rows(bits(body.pos)))
        assert np.array_equal(sorted_rows(vel[:, :3]), sorted_rows(bits(body.vel)))
        assert not pos[:, 3].any() and not pred[:, 3].any()
        assert np.array_equal(quats, bits(body.quats))
        rest = len(blob) - at
        print("shape sections: %d bytes, nt = %d" % (rest, nt))
        if kind == "polar-precise":
            assert rest % 64 == 0 and rest >= 64 * nt
        else:
            assert rest == SHAPE_BYTES[kind](nt)
        if twins:
            for twin, (_, (e0, e1)) in zip(twins, body.bodyRanges):
                twin.simulateSubsteps(7, DT, pp)
                assert np.array_equal(quats[e0:e1], bits(twin.quats))
    for b in [body] + (twins or []):
        b.close()
