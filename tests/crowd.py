"""The crowd: one deterministic batch of 300 small bodies for the per-body device calls (tests/test_crowd_cpu.py, tests/test_gpu_crowd.py).

300 is more than 256 (a second workgroup of every one-lane-per-body kernel), more than 2 x 128 with a rest of 44 (body_grabs.hip:
launch_value_rows) and 9 x 32 + 12 (place.hip: kRowsPerLaunch).  The bodies are single tets (4 particles, 1 tet), make_lattice(1) (8 / 6),
make_lattice(2) (27 / 48), a few make_lattice(4) (125 / 384) and exactly one make_lattice(8) (729 / 3,072: three nearest-particle chunks,
more than 1,024 snapshot units), in the order PLAN gives: single tets in runs of 25 and more -- so that a 256-row chunk spans more than
eight bodies and a wave of visual rows holds sixteen -- with every other kind next to every other and next to a run.  (The one lat8 has two
neighbours: a single tet in front, a lat1 behind.)  Body b stands in its own cell of a 20 x 15 grid, 1.5 m apart: every body fits a 1 m box.

No GPU is needed here.  build() asserts the facts the GPU tests rely on; state(seed) is the state they start from."""
import numpy as np

import place_ref
import raycast_device_ref
from tetsim_amd import boundary_surface, make_lattice, place_rows

COUNT = 300
PLAN = (("lat1", 1), ("lat2", 1), ("lat4", 1), ("lat1", 1), ("tet", 30), ("lat2", 2), ("lat1", 3), ("tet", 40), ("lat8", 1), ("lat1", 2), ("lat4", 1),
        ("lat2", 2), ("tet", 43), ("lat2", 1), ("lat1", 1), ("lat4", 1), ("lat2", 1), ("lat1", 1), ("tet", 40), ("lat4", 1), ("lat1", 5), ("lat2", 5),
        ("tet", 72), ("lat1", 1), ("lat2", 1), ("lat4", 1), ("lat1", 6), ("lat2", 6), ("tet", 25), ("lat2", 1), ("lat1", 1), ("lat2", 1), ("lat1", 1))
KINDS = [k for k, n in PLAN for _ in range(n)]
LAT8 = KINDS.index("lat8")
SAMPLE = (0, 1, 31, 32, 127, 128, 255, 256, 299, LAT8, LAT8 - 1, LAT8 + 1)
SPACING, COLUMNS = 1.5, 20
# every body stays inside these for the few substeps a test takes (the floor is 1.5 m below them)
PP = dict(gravity=-9.81, friction=1000.0, density=1000.0, devCompliance=1e-5, volCompliance=0.0, worldBounds=[-20.0, -1.0, -20.0, 20.0, 10.0, 20.0])
QUANTUM = 2.0 ** -16   # state(): every position is a multiple of it, so the midpoint of two particles is an f32 value
LAT8_TIE = (511, 512)  # neighbours along x in the lat8, the last particle of its second chunk of 256 and the first of its third
RAYS_PER_BODY = 4
_TET = (np.array([[0, 0.5, 0], [0.5, 0.5, 0], [0, 1.0, 0], [0, 0.5, 0.5]], np.float32), np.array([[0, 1, 2, 3]], np.int32))
_EDGE = dict(tet=0.5, lat1=1.0, lat2=0.5, lat4=0.25, lat8=0.125)


def mesh(kind):
    return _TET if kind == "tet" else make_lattice(int(kind[3:]))


def shift(b):
    return np.array([(b % COLUMNS - (COLUMNS - 1) / 2.0) * SPACING, 0.0, (b // COLUMNS - 7.0) * SPACING], np.float32)


def runs():
    """[(first body, length)] of the runs of single tets"""
    out, b = [], 0
    for kind, n in PLAN:
        if kind == "tet":
            out.append((b, n))
        b += n
    return out


class Crowd:
    """bodies [(verts, tets)] (shifted), rest / tets (the concatenation), first_vert / first_tet / first_row / first_tri [301], and the
    visual mesh: vis [rows, 4] and tris in the batch's numbering, vis_parts / tri_parts per body, row_body, row_particle (every visual row
    sits on a particle of its tet: one weight is 1)."""

    def __init__(self):
        self.bodies = []
        for b, kind in enumerate(KINDS):
            v, t = mesh(kind)
            self.bodies.append(((v + shift(b)).astype(np.float32), t))
        self.first_vert = np.concatenate([[0], np.cumsum([len(v) for v, _ in self.bodies])])
        self.first_tet = np.concatenate([[0], np.cumsum([len(t) for _, t in self.bodies])])
        self.rest = np.concatenate([v for v, _ in self.bodies])
        self.tets = np.concatenate([t + int(o) for (_, t), o in zip(self.bodies, self.first_vert)]).astype(np.int32)
        self.vis_parts, self.tri_parts, row_particle = [], [], []
        for b, (v, t) in enumerate(self.bodies):
            vis, tri = boundary_surface(t, len(v), v)
            w = np.concatenate([vis[:, 1:4], (np.float32(1) - vis[:, 1] - vis[:, 2] - vis[:, 3])[:, None]], axis=1)
            assert np.array_equal(np.sort(w, axis=1), np.tile(np.float32([0, 0, 0, 1]), (len(w), 1)))
            row_particle.append(t[vis[:, 0].astype(np.int64), np.argmax(w, axis=1)] + int(self.first_vert[b]))
            self.vis_parts.append(vis)
            self.tri_parts.append(tri)
        self.first_row = np.concatenate([[0], np.cumsum([len(p) for p in self.vis_parts])])
        self.first_tri = np.concatenate([[0], np.cumsum([len(p) for p in self.tri_parts])])
        self.vis = np.concatenate([p + np.array([self.first_tet[b], 0, 0, 0], np.float32) for b, p in enumerate(self.vis_parts)])
        self.tris = np.concatenate([p + int(self.first_row[b]) for b, p in enumerate(self.tri_parts)]).astype(np.int32)
        self.row_body = np.repeat(np.arange(COUNT), np.diff(self.first_row))
        self.row_particle = np.concatenate(row_particle)
        self.edge = np.array([_EDGE[k] for k in KINDS])
        self._check()

    def _check(self):
        assert len(self.bodies) == COUNT == len(KINDS) and KINDS.count("lat8") == 1 and 0 < LAT8 < COUNT - 1
        assert KINDS.count("tet") >= 150 and all(n >= 20 for _, n in runs()) and KINDS.count("lat4") >= 3
        assert len(set(SAMPLE)) == 12
        for first in (self.first_vert, self.first_tet):      # some chunk of 256 rows spans more than 8 bodies
            body_of = np.repeat(np.arange(COUNT), np.diff(first))
            spans = [body_of[min(r + 255, len(body_of) - 1)] - body_of[r] + 1 for r in range(0, len(body_of), 256)]
            assert max(spans) > 8, spans
            assert any(int(f) % 4 for f in first[1:-1])       # ... and some body boundary is no multiple of 4 rows
        assert KINDS[127] != KINDS[128] and KINDS[255] != KINDS[256]
        assert self.first_vert[LAT8 + 1] - self.first_vert[LAT8] == 729 > 2 * 256 and self.first_tet[LAT8 + 1] - self.first_tet[LAT8] == 3072
        pairs = {frozenset(p) for p in zip(KINDS[:-1], KINDS[1:]) if p[0] != p[1]}
        small = ("tet", "lat1", "lat2", "lat4")
        assert all(frozenset((a, b)) in pairs for i, a in enumerate(small) for b in small[i + 1:])
        lo = np.array([v.min(axis=0) for v, _ in self.bodies])
        hi = np.array([v.max(axis=0) for v, _ in self.bodies])
        for a in range(COUNT):                                # no two boxes overlap: a gap along x or z
            apart = (lo[a + 1:, 0] > hi[a, 0]) | (hi[a + 1:, 0] < lo[a, 0]) | (lo[a + 1:, 2] > hi[a, 2]) | (hi[a + 1:, 2] < lo[a, 2])
            assert apart.all(), a
        for b in np.flatnonzero(np.array(KINDS) == "tet"):    # a single tet: 4 visual rows, 4 triangles -- 16 such bodies in a wave of 64 rows
            assert len(self.vis_parts[b]) == 4 and len(self.tri_parts[b]) == 4
        wb = PP["worldBounds"]
        assert lo[:, 0].min() > wb[0] + 1 and hi[:, 0].max() < wb[3] - 1 and lo[:, 2].min() > wb[2] + 1 and hi[:, 2].max() < wb[5] - 1

    # ---- the seeded state ----------------------------------------------------------------------------------------------------------
    def state(self, seed):
        """(pos, vel) float32: rest + noise of about 3 % of the body's edge length (a multiple of QUANTUM, so that sums of two positions
        are exact), velocities of about 0.2 m/s; both from the body's own stream of the generator, so that no two bodies have equal rows."""
        pos, vel = np.empty_like(self.rest), np.empty_like(self.rest)
        for b in range(COUNT):
            rng = np.random.default_rng([seed, b])
            lo, hi = self.first_vert[b], self.first_vert[b + 1]
            noise = np.round(rng.normal(0.0, 0.03 * self.edge[b], (hi - lo, 3)) / QUANTUM) * QUANTUM
            pos[lo:hi] = (self.rest[lo:hi].astype(np.float64) + noise).astype(np.float32)
            vel[lo:hi] = (rng.normal(0.0, 0.2, (hi - lo, 3)) + rng.normal(0.0, 0.1, 3)).astype(np.float32)
        assert np.array_equal(pos.astype(np.float64) / QUANTUM, np.round(pos.astype(np.float64) / QUANTUM))
        return pos, vel

    def body(self, b, a):
        """rows of body b of a per-particle array"""
        return a[self.first_vert[b]:self.first_vert[b + 1]]

    def body_tets(self, b, a):
        return a[self.first_tet[b]:self.first_tet[b + 1]]

    # ---- body masks ----------------------------------------------------------------------------------------------------------------
    def mask(self, seed):
        """[300] bool, about half, seeded; inside every run of single tets bodies 3, 9, 10 and 17 of the run are chosen and 8 and 11 are not:
        chosen and unchosen bodies side by side behind the eighth body of a chunk and inside one 16-byte unit."""
        m = np.random.default_rng(seed).random(COUNT) < 0.5
        for first, _ in runs():
            m[[first + 3, first + 9, first + 10, first + 17]] = True
            m[[first + 8, first + 11]] = False
        return m

    # ---- body grabs ----------------------------------------------------------------------------------------------------------------
    def grab_table(self, seed, frame):
        """(particles int32 [300], targets float32 [300, 3]) of a frame: every third body (b % 3 == 2: 32, 128 and 299 of SAMPLE) and the
        lat8 held by a seeded particle, the target 5 cm below where the particle rests and moved 1 cm per frame; the others -1."""
        rng = np.random.default_rng(seed)
        held = np.array([int(rng.integers(0, self.first_vert[b + 1] - self.first_vert[b])) if b % 3 == 2 or b == LAT8 else -1 for b in range(COUNT)], np.int32)
        at = self.rest[self.first_vert[:-1] + np.maximum(held, 0)].astype(np.float64)
        return held, (at + [0.01 * frame, -0.05, 0.005 * frame]).astype(np.float32)

    # ---- placement -----------------------------------------------------------------------------------------------------------------
    def place_rows(self, seed):
        """float32 [300, 16]: an unnormalised quaternion, a pivot near the body's centre, a small offset inside its cell, a linear and an
        angular velocity, all seeded per body"""
        rows = np.empty((COUNT, 16), np.float32)
        for b, (v, _) in enumerate(self.bodies):
            rng = np.random.default_rng([seed, b])
            rows[b] = place_rows(rng.standard_normal(4) * 1.7, v.mean(axis=0) + rng.uniform(-0.05, 0.05, 3), rng.uniform(-0.1, 0.1, 3) + [0.0, 0.4, 0.0],
                                 rng.uniform(-1.0, 1.0, 3), rng.uniform(-2.0, 2.0, 3))[0]
        return rows

    def placed(self, rows, chosen, values, keep):
        """place_ref, body by body, of {pos, vel, quats | prevPos} (quats in the caller's tet order): bodies that are not chosen, or whose row
        place_ref.row_ok refuses, stay as they are."""
        out = {n: a.copy() for n, a in values.items()}
        for b in np.flatnonzero(chosen):
            if not place_ref.row_ok(rows[b]):
                continue
            p, e = slice(self.first_vert[b], self.first_vert[b + 1]), slice(self.first_tet[b], self.first_tet[b + 1])
            out["pos"][p], out["vel"][p] = place_ref.place_particles(rows[b], values["pos"][p], values["vel"][p], keep)
            if "quats" in values:
                out["quats"][e] = place_ref.place_quats(rows[b], values["quats"][e])
            else:
                out["prevPos"][p] = place_ref.place_points(rows[b], values["prevPos"][p])
        return out

    # ---- nearest particle ----------------------------------------------------------------------------------------------------------
    def tie_bodies(self):
        """the first single tet of every run and 19 more of the first three runs, and the lat8: bodies whose query point is a midpoint"""
        r = runs()
        return sorted({f for f, _ in r} | {r[k][0] + j for k in range(3) for j in range(2, 16, 2)} | {LAT8})

    def query_points(self, pos):
        """float32 [300, 3], one point per body: near the body's centre and off its surface; for tie_bodies() the midpoint of two of its
        particles (a single tet: particles 0 and 1, the ends of an edge whose other two corners are farther away; the lat8: LAT8_TIE) --
        an f32 value, both particles at the same f64 distance."""
        pts = np.empty((COUNT, 3), np.float32)
        for b in range(COUNT):
            x = self.body(b, pos).astype(np.float64)
            rng = np.random.default_rng([77, b])
            pts[b] = (x.mean(axis=0) + rng.uniform(-0.3, 0.3, 3) * self.edge[b]).astype(np.float32)
        for b in self.tie_bodies():
            x = self.body(b, pos).astype(np.float64)
            i, j = LAT8_TIE if b == LAT8 else (0, 1)
            mid = (x[i] + x[j]) / 2
            assert np.array_equal(mid.astype(np.float32).astype(np.float64), mid)
            pts[b] = mid
        return pts

    def nearest(self, pos, pts):
        """(ids int32 [300], dist2 float64 [300], tied [300]: how many particles share the minimum): Softbody.js:279-291 per body in f64,
        a0*a0 + a1*a1 + a2*a2 in that order, NaN never picked, the lowest index among equals; -1 and DBL_MAX for a body with none."""
        ids, d2, tied = np.full(COUNT, -1, np.int32), np.full(COUNT, np.finfo(np.float64).max), np.zeros(COUNT, np.int64)
        for b in range(COUNT):
            a = pts[b].astype(np.float64) - self.body(b, pos).astype(np.float64)
            with np.errstate(invalid="ignore"):
                d = (a[:, 0] * a[:, 0] + a[:, 1] * a[:, 1]) + a[:, 2] * a[:, 2]
            d = np.where(np.isnan(d), np.finfo(np.float64).max, d)
            i = int(np.argmin(d))                              # (the first minimum)
            if d[i] < np.finfo(np.float64).max:
                ids[b], d2[b], tied[b] = i, d[i], int((d == d[i]).sum())
        return ids, d2, tied

    # ---- range sensors ---------------------------------------------------------------------------------------------------------------
    def visual_positions(self, pos):
        """every visual row sits on a particle: weights 1, 0, 0, 0"""
        return np.asarray(pos, np.float32)[self.row_particle]

    def rays(self, vis_pos, seed):
        """(origins, directions, bodies): RAYS_PER_BODY rays per body, aimed at ITS rows as raycast_device_ref.seeded_rays aims them,
        grouped by body: two from a sphere of three radii towards a point inside its bounding sphere, two straight down z at one of its rows."""
        o, d, b = [], [], []
        for k in range(COUNT):
            rows = vis_pos[self.first_row[k]:self.first_row[k + 1]]
            ok, dk = raycast_device_ref.seeded_rays(rows, RAYS_PER_BODY, [seed, k])
            o.append(ok), d.append(dk), b.append(np.full(RAYS_PER_BODY, k, np.int32))
        return np.concatenate(o), np.concatenate(d), np.concatenate(b)

    def raycast(self, vis_pos, o, d, bodies):
        return raycast_device_ref.raycast(vis_pos, self.tris, self.row_body, COUNT, o, d, bodies=bodies)

    def spheres(self, vis_pos):
        return raycast_device_ref.bounding_spheres(vis_pos, self.row_body, COUNT)


_crowd = None


def build():
    """the crowd, built once per process"""
    global _crowd
    if _crowd is None:
        _crowd = Crowd()
    return _crowd

