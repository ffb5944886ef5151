"""The visual mesh's read-out, bit for bit on every path: skinned positions, rotated normals and three.js vertex normals of the device
against tests/skin_ref.py evaluated on the body's own `pos` and `quats` -- compared as uint32, no tolerance.

What this pins is the indexing tetsim_set_visual_mesh builds on the host (tetsim_visual.hip): `corner` through api2dev, `qidx` through
tet_perm into the device's tile order, a batch's rows, and the quaternion recovery of a lean-state body (ensure_quats) in front of the
skin.  Every polar body starts from skin_ref.twisted_start, so every tet has a rotation of its own (asserted: at least 99 % of the
quaternions are distinct bit patterns, at least half of the rotated normals differ from the rest normal by more than 0.1) and a
quaternion read from the wrong tet is a different quaternion; tests/test_skin_ref_cpu.py shows the same two conditions on the
reference's solver alone.  `quats` comes in the device's own order with `localTets` naming each row's tet: the pairing the GLSL goldens
(tests/test_gpu_polar_reference.py) and tests/test_gpu_lean_state.py compare quaternions by.

Partitioned bodies are tests/test_gpu_partition_state.py's (their positions are exact there)."""
import functools
import os

import numpy as np
import pytest

import skin_ref as R
from conftest import GOLDEN, load_f32
from tetsim_amd import SoftBodyHIP

pytestmark = pytest.mark.gpu
PP0, DT, SUBSTEPS = R.TWIST_PP, R.TWIST_DT, R.TWIST_SUBSTEPS      # the start tests/test_skin_ref_cpu.py proves non-vacuous on the oracle
_mesh = functools.lru_cache(maxsize=None)(R.twist_mesh)


@functools.lru_cache(maxsize=None)
def _dragon_visual():
    vis = load_f32("dragon_vis.f32").reshape(-1, 4)                # the artist's 29,800 rows and 59,657 triangles
    tris = np.fromfile(os.path.join(GOLDEN, "dragon_vistris.u16"), dtype="<u2").astype(np.int32).reshape(-1, 3)
    return vis, tris


def _visual(name, nt, seed=0):
    """(visVerts, rest normals, triangles): the edge rows and seeded rows in and outside the simplex; the Dragon: behind the artist's
    mesh.  Triangles: a seeded soup over all rows (repeated corners included); the Dragon: behind the artist's triangles."""
    rng = np.random.default_rng(seed + 100)
    vis = R.edge_vis_rows(nt, 1500, seed)
    tris = np.empty((0, 3), np.int32)
    if name == "dragon":
        artist, tris = _dragon_visual()
        vis = np.concatenate([artist, vis])
    tris = np.concatenate([tris, rng.integers(0, len(vis), size=(3000, 3)).astype(np.int32)])
    return vis, R.unit_normals(len(vis), seed), tris


def _twist(body, v):
    body.writeState(R.twisted_start(v), np.zeros_like(v))


def _step(body, how):
    if how == "call":
        body.simulateSubsteps(SUBSTEPS, DT, PP0)          # one call: the persistent / one-launch kernels
    else:
        for _ in range(SUBSTEPS):
            body.simulate(DT, PP0)


def _input_order_quats(body):
    q = body.quats                                        # rows in the device's order; localTets names each row's tet
    out = np.full_like(q, np.nan)
    out[body.localTets] = q
    return out


def _assert_same(got, ref, what):
    """Bit for bit, the sign of zero included; NaN by position."""
    got, ref = np.ascontiguousarray(got, dtype=np.float32), np.ascontiguousarray(ref, dtype=np.float32)
    assert got.shape == ref.shape, what
    gn, rn = np.isnan(got), np.isnan(ref)
    assert np.array_equal(gn, rn), "%s: NaN in other places" % what
    bad = np.flatnonzero(((got.view(np.uint32) != ref.view(np.uint32)) & ~gn).any(axis=1)) if got.size else []
    assert len(bad) == 0, "%s: %d of %d rows differ, first row %d: got %r, expected %r" % (what, len(bad), len(got), bad[0], got[bad[0]], ref[bad[0]])


def _check_polar(body, t, vis, n0, tris, what):
    # The visual mesh FIRST, straight behind the last substep: a lean-state body's quaternions are stale then, and the skin has to
    # bring them up to date itself (ensure_quats in front of skin_kernel) -- reading `quats` first would do that for it.
    got_p, got_n = body.visualPositions(with_normals=True)
    pos, q = body.pos, _input_order_quats(body)
    assert np.isfinite(pos).all() and np.isfinite(q).all(), what
    ref_n = R.rotate_normals_f32(n0, q[vis[:, 0].astype(np.int64)])
    # not vacuous: every tet has a quaternion of its own, and the quaternions turn the normals visibly
    assert R.distinct_rows(q) >= 0.99, what
    assert R.normals_moved(n0, ref_n) >= 0.5, what
    _assert_same(got_p, R.skin_f32(pos, t, vis), what + ": visualPositions")
    _assert_same(got_n, ref_n, what + ": rotated normals")
    _assert_same(body.visualPositions(), got_p, what + ": visualPositions without normals")
    if tris is not None:
        _assert_same(body.visualVertexNormals(), R.vertex_normals_threejs(got_p, tris), what + ": visualVertexNormals")


def _assert_path(body, nt, tile_ordered, fused, what):
    """Which path the body took, from TetSimInfo and the tet order it reports."""
    order = body.localTets
    print("%s: fused_particle_pass %d, tets %s" % (what, body.info.fused_particle_pass, "in the caller's order" if np.array_equal(order, np.arange(nt)) else "in tile order"))
    assert np.array_equal(np.sort(order), np.arange(nt)), what
    assert (not np.array_equal(order, np.arange(nt))) == tile_ordered, what
    assert body.info.fused_particle_pass == fused, what


# name -> (mesh, constructor options, how it is stepped, the path it takes)
#   tile_ordered: FAST bodies without the gather formulation keep their tets in tile order (localTets is a permutation, qidx goes
#                 through it); PRECISE and gather bodies keep the caller's order
#   fused:        TetSimInfo.fused_particle_pass -- 3: the small-body frame kernel on 64-tet tiles, four lanes per tet (pj_quad.hip);
#                 2: the persistent kernel on 256-tet tiles (lean-state bodies take it); 0: one kernel pair per substep
# On these bodies `simulateSubsteps` is ONE launch of the persistent frame kernels (3, 2).  Paths 1 (one fused kernel per substep) and 5
# (pjb_call_kernel, the one-launch call of large bodies) need 2,048 tiles or more, over half a million tets: NOT reached here -- the skin
# reads the same arrays behind them (pj.pos_final, pj.quat), and tests/test_gpu_lean_state.py holds their quats equal to the pair's.
POLAR = {
    "dragon-precise": ("dragon", dict(precision="precise"), "simulate", dict(tile_ordered=False, fused=0)),
    "dragon-fast": ("dragon", dict(precision="fast"), "simulate", dict(tile_ordered=True, fused=3)),
    "lat4-precise": ("lat4", dict(precision="precise"), "simulate", dict(tile_ordered=False, fused=0)),
    "lat4-fast": ("lat4", dict(precision="fast"), "call", dict(tile_ordered=True, fused=3)),
    "lat12-precise-simulate": ("lat12", dict(precision="precise"), "simulate", dict(tile_ordered=False, fused=0)),
    "lat12-precise-call": ("lat12", dict(precision="precise"), "call", dict(tile_ordered=False, fused=0)),
    "lat12-fast-simulate": ("lat12", dict(precision="fast"), "simulate", dict(tile_ordered=True, fused=3)),
    "lat12-fast-call": ("lat12", dict(precision="fast"), "call", dict(tile_ordered=True, fused=3)),
    "lat12-lean-simulate": ("lat12", dict(precision="fast", lean_state=True), "simulate", dict(tile_ordered=True, fused=2)),
    "lat12-lean-call": ("lat12", dict(precision="fast", lean_state=True), "call", dict(tile_ordered=True, fused=2)),
    "lat12-gather-simulate": ("lat12", dict(precision="fast", gather=True), "simulate", dict(tile_ordered=False, fused=0)),
    "lat12-gather-call": ("lat12", dict(precision="fast", gather=True), "call", dict(tile_ordered=False, fused=0)),
}

@pytest.mark.parametrize("case", sorted(POLAR))
def test_polar_skin_and_normals_bit_for_bit(case):
    name, kw, how, path = POLAR[case]
    v, t = _mesh(name)
    vis, n0, tris = _visual(name, len(t))
    body = SoftBodyHIP(v, t, None, dict(PP0), solver="polar", **kw)
    body.setVisualMesh(vis, n0)
    body.setVisualTriangles(tris)
    _assert_path(body, len(t), path["tile_ordered"], path["fused"], case)
    _twist(body, v)
    _step(body, how)
    _check_polar(body, t, vis, n0, tris, case)
    body.close()


@pytest.mark.parametrize("precision", ["precise", "fast"])
def test_a_batch_of_three_meshes_bit_for_bit(precision):
    """The Dragon, lat4 and hub behind one handle: the rows of the visual mesh name tets of all three in no order, each row takes ITS
    body's corners and ITS tet's quaternion."""
    names = ["dragon", "lat4", "hub"]
    parts = [_mesh(n) for n in names]
    body = SoftBodyHIP.batch(parts, dict(PP0), solver="polar", precision=precision)
    voff = np.concatenate([[0], np.cumsum([len(v) for v, _ in parts])])
    v = np.concatenate([v for v, _ in parts])
    t = np.concatenate([tt + int(voff[i]) for i, (_, tt) in enumerate(parts)])
    vis, n0, tris = _visual("batch", len(t), seed=5)
    tet_body = np.searchsorted(np.cumsum([len(tt) for _, tt in parts]), vis[:, 0].astype(np.int64), side="right")
    assert (np.diff(tet_body) != 0).sum() > len(vis) // 4 and set(tet_body) == {0, 1, 2}       # interleaved, not grouped by body
    body.setVisualMesh(vis, n0)
    body.setVisualTriangles(tris)
    assert body.info.num_bodies == 3 and [r[1][1] for r in body.bodyRanges] == list(np.cumsum([len(tt) for _, tt in parts]))
    # FAST: tiles of 64 tets that never span two bodies, the four-lane frame kernel; PRECISE: the caller's order, a kernel pair per substep
    _assert_path(body, len(t), precision == "fast", 3 if precision == "fast" else 0, "batch-" + precision)
    body.writeState(np.concatenate([R.twisted_start(pv) for pv, _ in parts]), np.zeros_like(v))
    _step(body, "call")
    _check_polar(body, t, vis, n0, tris, "batch-" + precision)
    body.close()


NH = {"precise-original": dict(precision="precise", order="original"), "precise-coloured": dict(precision="precise", order="coloured"),
      "fast-clustered": dict(precision="fast", order="clustered")}


@pytest.mark.parametrize("name", ["lat4", "dragon"])
@pytest.mark.parametrize("kind", sorted(NH))
def test_neohookean_skin_bit_for_bit(kind, name):
    """Softbody.js's updateVisMesh arithmetic (f64 steps, f32 stores) on rows the artist never drew, from a twisted state."""
    v, t = _mesh(name)
    vis, _, tris = _visual(name, len(t), seed=2)
    body = SoftBodyHIP(v, t, None, dict(PP0), vis, tris, solver="neohookean", **NH[kind])
    body.writeState(R.twisted_start(v, angle=0.5), np.zeros_like(v))
    _step(body, "call" if kind == "fast-clustered" else "simulate")
    pos = body.pos
    assert np.isfinite(pos).all() and np.abs(pos - v).max() > 0.01
    got = body.visualPositions()
    _assert_same(got, R.skin_js(pos, t, vis), "%s %s: visualPositions" % (name, kind))
    assert not R.same_bits(got, R.skin_f32(pos, t, vis))          # (the two orders of arithmetic are told apart by these rows)
    _assert_same(body.visualVertexNormals(), R.vertex_normals_threejs(got, tris), "%s %s: visualVertexNormals" % (name, kind))
    body.close()


# ---- visual rows at the edges (lat4: 384 tets, six 64-tet tiles in FAST) -----------------------------------------------------------------
KINDS = {"polar-precise": dict(solver="polar", precision="precise"), "polar-fast": dict(solver="polar", precision="fast"),
         "polar-lean": dict(solver="polar", precision="fast", lean_state=True), "nh-precise": dict(solver="neohookean", precision="precise")}


def _edge_body(kind):
    v, t = _mesh("lat4")
    body = SoftBodyHIP(v, t, None, dict(PP0), **KINDS[kind])
    _twist(body, v)
    _step(body, "simulate")
    pos = body.pos                                       # (positions only: `quats` would bring a lean-state body's quaternions up to date)
    assert np.isfinite(pos).all() and np.abs(pos - v).max() > 0.01, kind
    return body, t


def _check_rows(body, t, vis, kind, what, spread):
    """spread: the rows lie on tets all over the mesh, enough of them for the half-of-the-rows condition."""
    n0 = R.unit_normals(len(vis), seed=9)
    polar = kind.startswith("polar")
    body.setVisualMesh(vis, n0 if polar else None)
    assert body.numVisVerts == len(vis)
    if not polar:
        pos = body.pos
        assert np.isfinite(pos).all(), what
        _assert_same(body.visualPositions(), R.skin_js(pos, t, vis), what + ": visualPositions")
        return
    got_p, got_n = body.visualPositions(with_normals=True)      # first: see _check_polar
    pos, q = body.pos, _input_order_quats(body)
    assert np.isfinite(pos).all() and np.isfinite(q).all(), what
    ref_n = R.rotate_normals_f32(n0, q[vis[:, 0].astype(np.int64)])
    # not vacuous.  The body's quaternions whatever the rows; the moved normals where the rows can carry the condition: one row is on the
    # first tet, where the twist angle is about 0, and 300 rows on ONE tet move together or not at all -- those sets only need THEIR
    # quaternion to be no other tet's (then a wrong qidx is a wrong normal) and not the identity's bit pattern
    assert R.distinct_rows(q) >= 0.99, what
    if spread:
        assert R.normals_moved(n0, ref_n) >= 0.5, what
    else:
        mine = q[int(vis[0, 0])]
        assert (np.ascontiguousarray(q).view(np.uint32) == mine.view(np.uint32)).all(axis=1).sum() == 1, what
        assert not np.array_equal(mine, np.float32([0, 0, 0, 1])) and not R.same_bits(ref_n, n0), what
    _assert_same(got_n, ref_n, what + ": rotated normals")
    _assert_same(got_p, R.skin_f32(pos, t, vis), what + ": visualPositions")


@pytest.mark.parametrize("kind", sorted(KINDS))
@pytest.mark.parametrize("rows", [1, 255, 256, 257, "300-on-one-tet", "300-on-the-last-tet"])
def test_visual_rows_at_the_edges(rows, kind):
    """Row counts around a 256-lane block; the first and the last tet; weights of exactly 1 and 0, outside the simplex, cancelling in
    1 - (...), denormal (skin_ref.edge_vis_rows); 300 rows that all read one tet."""
    body, t = _edge_body(kind)
    if isinstance(rows, int):
        vis = R.edge_vis_rows(len(t), rows)
    else:
        vis = R.one_tet_vis_rows(len(t) - 1 if "last" in rows else 137)
    _check_rows(body, t, vis, kind, "%s, %s rows" % (kind, rows), spread=isinstance(rows, int) and rows >= 255)
    body.close()


@pytest.mark.parametrize("kind", sorted(KINDS))
def test_a_visual_mesh_of_no_rows(kind):
    body, _ = _edge_body(kind)
    polar = kind.startswith("polar")
    body.setVisualMesh(np.zeros((0, 4), np.float32), np.zeros((0, 3), np.float32) if polar else None)
    body.setVisualTriangles(np.zeros((0, 3), np.int32))
    assert body.numVisVerts == 0 and body.info.num_vis_verts == 0
    p = body.visualPositions()
    assert p.shape == (0, 3) and p.dtype == np.float32
    if polar:
        p, n = body.visualPositions(with_normals=True)
        assert p.shape == (0, 3) and n.shape == (0, 3)
    assert body.visualVertexNormals().shape == (0, 3)
    assert body.visualVertexNormalsFrom(np.zeros((0, 3), np.float32)).shape == (0, 3)
    body.simulate(DT, PP0)                                  # the body steps on
    assert np.isfinite(body.pos).all()
    body.close()


# ---- vertex normals at the edges ------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("kind", ["polar-fast", "nh-precise"])
def test_vertex_normals_at_the_edges(kind):
    """visualVertexNormalsFrom on positions no simulation produces (skin_ref.edge_triangle_soup): a vertex in no, in one and in 300
    triangles, a vertex named twice, collinear corners, an underflowing and an overflowing running sum, a NaN coordinate.  NaN by
    position, everything else by bits: `length() || 1` leaves signed zeros and, next to a NaN, the finite components as they are."""
    pos, tris, names = R.edge_triangle_soup()
    body, t = _edge_body(kind)
    body.setVisualMesh(R.edge_vis_rows(len(t), len(pos)))
    body.setVisualTriangles(tris)
    ref = R.vertex_normals_threejs(pos, tris)
    got = body.visualVertexNormalsFrom(pos)
    _assert_same(got, ref, kind + ": visualVertexNormalsFrom")
    # (what the reference gives there is asserted in tests/test_skin_ref_cpu.py; here: the device did reach those branches)
    assert np.isnan(got[names["huge"]]).any() and np.isnan(got[names["nan"]]).any() and np.isfinite(got[names["nan"]]).any()
    assert np.signbit(got[names["tiny"]]).any() and not got[names["tiny"]].any()
    # the same positions in another order of the rows' reads: the body's own skin is untouched by the call
    _assert_same(body.visualVertexNormals(), R.vertex_normals_threejs(body.visualPositions(), tris), kind + ": visualVertexNormals afterwards")
    body.close()
