"""The crowd of tests/crowd.py without a GPU: the builder's own assertions, and that the references of the per-body calls are usable at this
shape before tests/test_gpu_crowd.py takes them to the device -- body b of the concatenation gets exactly what body b gets alone, the ray
set holds the hit-share condition, and the nearest-particle query points carry real f64 ties."""
import numpy as np

import crowd
import observe_ref
import place_ref
import pose_ref
import raycast_device_ref
import raycast_ref
import strain_ref
from test_pose_cpu import prep_table
from test_strain_cpu import prep_rest

SEED = 5


def bits(a):
    return np.ascontiguousarray(a, dtype=np.float64).view(np.uint64)


def strain_reference(verts, tets, pos, first_tet=None):
    """tests/test_gpu_strain.py: reference"""
    _, irp, _ = prep_rest(verts, tets, crowd.PP["density"])
    deg = strain_ref.degenerate_tets(verts, tets, irp)
    val = strain_ref.tet_values(pos, tets, irp)
    rows = strain_ref.tet_rows(val, deg)
    return rows, strain_ref.body_rows(val, rows, strain_ref.rest_volume(verts, tets), deg, first_tet)


def test_the_builder_holds_its_own_facts():
    c = crowd.build()
    assert len(c.bodies) == 300 and crowd.KINDS[crowd.LAT8] == "lat8" and [n for _, n in crowd.runs()] == [30, 40, 43, 40, 72, 25]
    assert c.first_vert[-1] == len(c.rest) == 3105 and c.first_tet[-1] == len(c.tets) == 6388
    assert len(c.vis) == c.first_row[-1] and len(c.tris) == c.first_tri[-1] and c.tris.max() == len(c.vis) - 1
    assert np.array_equal(c.row_body[c.tris[:, 0]], c.row_body[c.tris[:, 2]])            # no triangle spans two bodies
    assert np.array_equal(c.rest[c.row_particle], c.visual_positions(c.rest))
    pos, vel = c.state(SEED)
    again = c.state(SEED)
    assert np.array_equal(pos, again[0]) and np.array_equal(vel, again[1]) and not np.array_equal(pos, c.state(SEED + 1)[0])
    for b in range(crowd.COUNT):                                                          # noise of about 3 % of the edge, velocities of about 0.2 m/s
        moved = np.abs(c.body(b, pos) - c.body(b, c.rest)).max()
        assert 0.005 * c.edge[b] < moved < 0.15 * c.edge[b], (b, moved)
        assert 0.02 < np.abs(c.body(b, vel)).max() < 1.5
    local = pos - np.concatenate([np.tile(crowd.shift(b), (len(v), 1)) for b, (v, _) in enumerate(c.bodies)])
    assert len(np.unique(np.concatenate([local, vel], axis=1), axis=0)) == len(pos)       # no two rows alike, whatever their bodies
    for seed in (1, 2):
        m = c.mask(seed)
        assert 120 < m.sum() < 180
        for first, _ in crowd.runs():
            assert m[[first + 3, first + 9, first + 10, first + 17]].all() and not m[[first + 8, first + 11]].any()
    assert not np.array_equal(c.mask(1), c.mask(2))
    held, targets = c.grab_table(3, 0)
    assert (held >= 0).sum() == 101 and all(held[b] >= 0 for b in (32, 128, 299, crowd.LAT8)) and np.isfinite(targets).all()
    assert all(held[b] < c.first_vert[b + 1] - c.first_vert[b] for b in range(crowd.COUNT))
    rows = c.place_rows(4)
    assert all(place_ref.row_ok(r) for r in rows) and len(np.unique(rows, axis=0)) == crowd.COUNT


def test_every_reference_gives_a_body_of_the_concatenation_what_it_gives_the_body_alone():
    c = crowd.build()
    pos, vel = c.state(SEED)
    density = crowd.PP["density"]
    obs = observe_ref.observe(c.rest, c.tets, pos, vel, density, c.first_vert, c.first_tet)
    tbl = prep_table(c.rest, c.tets, c.first_vert, c.first_tet, density)[0]
    poses = pose_ref.raw(tbl, pos, vel, c.first_vert)
    tet_rows, body_rows = strain_reference(c.rest, c.tets, pos, c.first_tet)
    assert np.isfinite(tet_rows).all() and np.isfinite(body_rows).all() and not body_rows[:, 7].any()
    vis = c.visual_positions(pos)
    o, d, rb = c.rays(vis, SEED)
    hits = c.raycast(vis, o, d, rb)
    spheres = c.spheres(vis)
    rows = c.place_rows(SEED)
    quats = np.random.default_rng(SEED).standard_normal((len(c.tets), 4)).astype(np.float32)
    placed = c.placed(rows, np.ones(crowd.COUNT, bool), dict(pos=pos, vel=vel, quats=quats), True)
    for b in crowd.SAMPLE:
        v, t = c.bodies[b]
        p, u = c.body(b, pos), c.body(b, vel)
        assert observe_ref.observe(v, t, p, u, density)[0] == obs[b], b
        alone = prep_table(v, t, None, None, density)[0]
        assert np.array_equal(alone.view(np.uint64), c.body(b, tbl).view(np.uint64)), b
        assert pose_ref.raw(alone, p, u)[0] == poses[b], b
        r1, b1 = strain_reference(v, t, p)
        assert np.array_equal(r1.view(np.uint32), c.body_tets(b, tet_rows).view(np.uint32)) and np.array_equal(bits(b1[0]), bits(body_rows[b])), b
        sel = np.flatnonzero(rb == b)
        rows_b = vis[c.first_row[b]:c.first_row[b + 1]]
        want = raycast_ref.raycast(rows_b, c.tri_parts[b], o[sel], d[sel])
        hit = want["hit"] == 1
        assert np.array_equal(hits["hit"][sel], want["hit"]) and np.array_equal(hits["body"][sel], np.where(hit, b, -1)), b
        assert np.array_equal(hits["triangle"][sel], np.where(hit, want["triangle"] + c.first_tri[b], -1)), b
        assert np.array_equal(bits(hits["distance"][sel]), bits(want["distance"])) and np.array_equal(bits(hits["point"][sel]), bits(want["point"])), b
        assert np.array_equal(bits(spheres[b]), bits(np.append(*raycast_ref.bounding_sphere(rows_b)))), b
        pp, pu = place_ref.place_particles(rows[b], p, u, True)
        assert np.array_equal(pp, c.body(b, placed["pos"])) and np.array_equal(pu, c.body(b, placed["vel"])), b
        assert np.array_equal(place_ref.place_quats(rows[b], c.body_tets(b, quats)), c.body_tets(b, placed["quats"])), b
        assert np.abs(pp - p).max() > 0.1


def test_the_rays_hit_and_miss_on_the_reference_alone():
    c = crowd.build()
    vis = c.visual_positions(c.state(SEED)[0])
    o, d, rb = c.rays(vis, SEED)
    assert len(o) == 1200 and np.array_equal(rb, np.repeat(np.arange(300), 4))
    own = c.raycast(vis, o, d, rb)
    assert raycast_device_ref.hit_share_ok(own["hit"])
    kinds = np.array(crowd.KINDS)
    for k in ("tet", "lat1", "lat2"):                                                     # ... and so do the rays of every kind there is a crowd of
        assert raycast_device_ref.hit_share_ok(own["hit"][np.isin(rb, np.flatnonzero(kinds == k))]), k
    assert (own["hit"][rb == crowd.LAT8] == 1).any()
    assert not raycast_device_ref.invalid_rays(o, d, 0.0, np.inf, rb, crowd.COUNT).any()


def test_the_query_points_carry_real_ties():
    c = crowd.build()
    pos, _ = c.state(SEED)
    pts = c.query_points(pos)
    ids, d2, tied = c.nearest(pos, pts)
    tie = c.tie_bodies()
    kinds = np.array(crowd.KINDS)
    assert sum(kinds[b] == "tet" for b in tie) >= 20 and crowd.LAT8 in tie
    assert (tied[tie] == 2).all() and (tied[np.setdiff1d(np.arange(300), tie)] == 1).all()
    assert all(ids[b] == 0 for b in tie if b != crowd.LAT8)                              # particles 0 and 1 of a single tet: 0 wins
    assert ids[crowd.LAT8] == crowd.LAT8_TIE[0] == 511 and crowd.LAT8_TIE[1] // 256 == 2   # chunks 1 and 2 of the lat8: the earlier chunk wins
    assert (ids >= 0).all() and (d2 > 0).all() and len(np.unique(pts, axis=0)) == 300
    bad = pos.copy()                                                                      # a body of NaN particles has nothing to pick
    bad[c.first_vert[40]:c.first_vert[41]] = np.nan
    ids2, d22, _ = c.nearest(bad, pts)
    assert ids2[40] == -1 and d22[40] == np.finfo(np.float64).max and np.array_equal(np.delete(ids2, 40), np.delete(ids, 40))
