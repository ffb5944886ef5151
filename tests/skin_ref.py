"""The visual mesh's read-out, restated in numpy in the order in which the kernels (tetsim_amd/csrc/skin_kernels.hip) and the reference's
JS / GLSL write it, every intermediate rounded where the source rounds it -- so a device result can be compared as uint32, no tolerance.

* skin_f32               the vertex shader's skin (SoftbodyGPU.js:429-435), all f32: the polar bodies' visualPositions()
* skin_js                updateVisMesh (Softbody.js:259-271), f64 arithmetic with an f32 store per step: the Neo-Hookean bodies'
* rotate_normals_f32     Rotate(objectNormal, tetQuaternion) (SoftbodyGPU.js:428,440) as skin_kernel writes it, all f32
* vertex_normals_threejs three.js r160 BufferGeometry.computeVertexNormals + normalizeNormals (Softbody.js:273)

tests/test_skin_ref_cpu.py checks these against the reference's recorded output and against plain high precision, without a GPU.
Below them: what the CPU and the GPU tests share (the twisted start and its parameters, the two non-vacuity measures, visual rows and
triangle soups at the edges).  numpy only."""
import numpy as np

U32 = 2.0 ** -24          # unit roundoff of f32
TINY32 = 2.0 ** -126      # smallest normal f32


def same_bits(a, b):
    a, b = np.ascontiguousarray(a, dtype=np.float32), np.ascontiguousarray(b, dtype=np.float32)
    return a.shape == b.shape and np.array_equal(a.view(np.uint32), b.view(np.uint32))


def skin_f32(pos, tets, vis):
    """The vertex shader's arithmetic (SoftbodyGPU.js:429-435) in numpy f32: ((p0*b0 + p1*b1) + p2*b2) + p3*b3, b3 = 1 - ((b0 + b1) + b2)."""
    pos = np.asarray(pos, dtype=np.float32)
    e = vis[:, 0].astype(np.int64)
    b0, b1, b2 = (vis[:, k].astype(np.float32)[:, None] for k in (1, 2, 3))
    b3 = np.float32(1.0) - ((b0 + b1) + b2)
    p = [pos[tets[e, k]] for k in range(4)]
    return ((p[0] * b0 + p[1] * b1) + p[2] * b2) + p[3] * b3


def skin_js(pos, tets, vis):
    """updateVisMesh (Softbody.js:259-271): b3 = 1.0 - b0 - b1 - b2 in f64; the Float32Array row starts at 0 and takes four
    `a += p * b` steps, each an f64 multiply and add with an f32 store."""
    pos = np.asarray(pos, dtype=np.float32)
    e = vis[:, 0].astype(np.int64)
    b0, b1, b2 = (vis[:, k].astype(np.float32).astype(np.float64)[:, None] for k in (1, 2, 3))
    b3 = 1.0 - b0 - b1 - b2
    a = np.zeros((len(vis), 3), np.float32)
    with np.errstate(all="ignore"):
        for k, b in enumerate((b0, b1, b2, b3)):
            a = (a.astype(np.float64) + pos[tets[e, k]].astype(np.float64) * b).astype(np.float32)
    return a


def rotate_normals_f32(n0, quat_rows):
    """skin_kernel's rotation of the rest normal n by its tet's quaternion q = (x, y, z, w), all f32:
    i = (q.yzx * n.zxy - n.yzx * q.zxy) + q.w * n;  out = n + 2 * (q.yzx * i.zxy - i.yzx * q.zxy)."""
    n, q = np.asarray(n0, dtype=np.float32), np.asarray(quat_rows, dtype=np.float32)
    nx, ny, nz = n[:, 0], n[:, 1], n[:, 2]
    qx, qy, qz, qw = q[:, 0], q[:, 1], q[:, 2], q[:, 3]
    two = np.float32(2.0)
    ix = (qy * nz - ny * qz) + qw * nx
    iy = (qz * nx - nz * qx) + qw * ny
    iz = (qx * ny - nx * qy) + qw * nz
    return np.stack([nx + two * (qy * iz - iy * qz), ny + two * (qz * ix - iz * qx), nz + two * (qx * iy - ix * qy)], axis=1)


def vertex_normals_threejs(pos, tri):
    """BufferGeometry.computeVertexNormals + normalizeNormals of three.js r160, restated (pinned against the reference's own
    output by tests/test_oracle_golden.py::test_vertex_normals_golden_is_threejs_computeVertexNormals): f64 face normals from f32
    positions, accumulated in triangle order with an f32 store per add, normalised in f64 by `length() || 1` (0 and NaN are falsy),
    stored f32."""
    pos, tri = np.asarray(pos, dtype=np.float32), np.asarray(tri, dtype=np.int64).reshape(-1, 3)
    with np.errstate(all="ignore"):      # (an overflowing sum becomes inf, inf * 0 becomes NaN: as in JavaScript, silently)
        P = pos.astype(np.float64)
        cb, ab = P[tri[:, 2]] - P[tri[:, 1]], P[tri[:, 0]] - P[tri[:, 1]]
        face = np.stack([cb[:, 1] * ab[:, 2] - cb[:, 2] * ab[:, 1], cb[:, 2] * ab[:, 0] - cb[:, 0] * ab[:, 2],
                         cb[:, 0] * ab[:, 1] - cb[:, 1] * ab[:, 0]], axis=1)
        # three.js walks the triangles in order and adds each face normal to its three corners through Float32Array stores, so vertex
        # v's normal is the f32-rounded running sum over ITS corners in triangle order: round r adds every vertex's r-th one at once
        flat = tri.ravel()
        order = np.argsort(flat, kind="stable")            # (by vertex; within a vertex in triangle order, corner order)
        vs, ts = flat[order], order // 3
        rank = np.arange(len(vs)) - np.searchsorted(vs, vs)
        n = np.zeros_like(pos)
        for r in range(int(rank.max()) + 1 if len(vs) else 0):
            m = rank == r
            n[vs[m]] = (n[vs[m]].astype(np.float64) + face[ts[m]]).astype(np.float32)
        N = n.astype(np.float64)
        length = np.sqrt(N[:, 0] * N[:, 0] + N[:, 1] * N[:, 1] + N[:, 2] * N[:, 2])
        length[(length == 0) | np.isnan(length)] = 1.0
        return (N * (1.0 / length)[:, None]).astype(np.float32)


# ---- shared inputs ---------------------------------------------------------------------------------------------------------------
# the start of every exact test, on the oracle (tests/test_skin_ref_cpu.py) and on the device (tests/test_gpu_skin_exact.py) alike:
# twisted_start, gravity off (the body stays away from the walls), TWIST_SUBSTEPS substeps of TWIST_DT
TWIST_PP = dict(gravity=0.0, friction=1000.0, density=1000.0, devCompliance=1e-5, volCompliance=0.0,
                worldBounds=[-2.5, -1.0, -2.5, 2.5, 10.0, 2.5])
TWIST_DT = (1.0 / 60.0) / 20
TWIST_SUBSTEPS = 5
TWIST_MESHES = ("dragon", "lat4", "lat12", "hub")


def twist_mesh(name):
    """(verts, tets) of a mesh the exact tests use: a golden mesh, or "lat12", the 12-cell lattice."""
    if name == "lat12":
        from tetsim_amd import make_lattice
        return make_lattice(12, y0=0.3)
    from conftest import load_mesh
    return load_mesh(name)


def distinct_rows(q):
    """The share of rows of q that are distinct as bit patterns."""
    q = np.ascontiguousarray(q, dtype=np.float32)
    return len(np.unique(q.view(np.uint32).reshape(len(q), -1), axis=0)) / len(q)


def normals_moved(n0, rotated):
    """The share of rows whose rotated normal differs from the rest normal by more than 0.1 in some component."""
    return float((np.abs(np.asarray(rotated) - np.asarray(n0)).max(axis=1) > 0.1).mean())


def twisted_start(verts, seed=0, angle=1.5, jitter=0.01):
    """The rest positions rotated about the body's long axis (through its centre) by an angle that grows linearly from 0 to `angle` rad
    along that axis, plus a seeded jitter of `jitter` x the body's shortest bounding-box side / 16 per coordinate: every tet gets a
    rotation of its own, so a quaternion read from the wrong tet is a different quaternion."""
    v = np.asarray(verts, dtype=np.float64)
    lo, hi = v.min(axis=0), v.max(axis=0)
    ax = int(np.argmax(hi - lo))
    a, b = (ax + 1) % 3, (ax + 2) % 3
    c = 0.5 * (lo + hi)
    th = angle * (v[:, ax] - lo[ax]) / (hi[ax] - lo[ax])
    out = v.copy()
    out[:, a] = c[a] + np.cos(th) * (v[:, a] - c[a]) - np.sin(th) * (v[:, b] - c[b])
    out[:, b] = c[b] + np.sin(th) * (v[:, a] - c[a]) + np.cos(th) * (v[:, b] - c[b])
    out += np.random.default_rng(seed).uniform(-1.0, 1.0, size=v.shape) * (jitter * (hi - lo).min() / 16.0)
    return out.astype(np.float32)


def unit_normals(n, seed=0):
    n0 = np.random.default_rng(seed).standard_normal((n, 3)).astype(np.float32)
    return n0 / np.linalg.norm(n0, axis=1, keepdims=True)


def _special_weights():
    f = np.float32
    third, tenth = f(1.0) / f(3.0), f(0.1)
    return np.array([
        [1.0, 0.0, 0.0],                    # a weight of exactly 1, the others exactly 0: the row IS corner 0
        [0.0, 0.0, 0.0],                    # ... corner 3 (b3 = 1)
        [0.0, 1.0, 0.0], [0.0, 0.0, 1.0],
        [-0.5, 1.7, 0.25],                  # outside the simplex
        [1.7, -0.5, -0.5], [-0.5, -0.5, -0.5], [1.7, 1.7, 1.7],
        [0.5, 0.25, 0.25],                  # 1 - (...) cancels to exactly 0
        [third, third, third],              # ... to one rounding of 1/3
        [f(0.7), f(0.2), tenth],            # ... to the roundings of the three weights
        [0.5, 0.25, f(0.25) - f(2.0 ** -24)],   # ... to 2^-24, the last bit below 1
        [f(1.0) - f(2.0 ** -24), f(2.0 ** -25), f(2.0 ** -26)],   # ... to 0 where the exact value is 2^-25 + 2^-26: the sum rounds
        [1e-40, 1e-45, -1e-42],             # denormal weights (1e-45 rounds to the smallest one)
        [-1e-45, 0.25, 1e-39], [f(2.0 ** -126), f(2.0 ** -127), f(-2.0 ** -149)],
    ], dtype=np.float32)


def edge_vis_rows(nt, count, seed=0):
    """`count` rows (tetNr, b0, b1, b2) on a mesh of nt tets.  The first rows are the edges, cut off at `count`: the first and the last
    tet, weights of exactly 1 and 0, weights outside the simplex (-0.5, 1.7), weights whose sum cancels in 1 - (...), denormal weights;
    the rest are seeded draws, half inside the simplex (Dirichlet), half uniform in [-0.5, 1.7], on tets drawn all over the mesh."""
    rng = np.random.default_rng(seed)
    w = _special_weights()
    tet = np.empty(len(w), np.int64)
    tet[0::2], tet[1::2] = 0, nt - 1                    # (the first tet and the last one alternate through the special rows)
    rows = np.concatenate([tet[:, None].astype(np.float32), w], axis=1)
    more = max(count - len(rows), 0)
    inside = rng.dirichlet(np.ones(4), size=more)[:, :3]
    outside = rng.uniform(-0.5, 1.7, size=(more, 3))
    draw = np.where((np.arange(more) % 2 == 0)[:, None], inside, outside).astype(np.float32)
    rest = np.concatenate([rng.integers(0, nt, size=(more, 1)).astype(np.float32), draw], axis=1)
    return np.ascontiguousarray(np.concatenate([rows, rest])[:count], dtype=np.float32)


def one_tet_vis_rows(tet, count=300, seed=0):
    """`count` rows on ONE tet: every lane of a wave and of the next block reads the same corners and the same quaternion."""
    rng = np.random.default_rng(seed)
    w = rng.uniform(-0.5, 1.7, size=(count, 3)).astype(np.float32)
    return np.ascontiguousarray(np.concatenate([np.full((count, 1), tet, np.float32), w], axis=1))


def edge_triangle_soup(seed=0):
    """(positions [n, 3] f32, triangles [m, 3] int32, names) that no simulation produces, for visualVertexNormalsFrom.  names maps what
    each vertex is there for to its row:
    lonely: in no triangle -> (0, 0, 0);  single: in one triangle;  hub: in 300 triangles (an f32 running sum of 300 f64 face normals);
    twice: named twice by its triangle (a zero face normal);  line: three collinear corners;
    tiny: coordinates around 1e-30, whose face normals (1e-60) underflow in the f32 sum -> length 0 -> `|| 1` -> signed zeros;
    huge: around 1e19 (2e19 .. 4e19), whose sum overflows to inf -> 1 / inf = 0 -> inf * 0 = NaN next to signed zeros, as in three.js;
    nan: a NaN coordinate -> NaN sums -> a NaN length -> `|| 1`: the finite components survive."""
    rng = np.random.default_rng(seed)
    pos, tri, names = [], [], {}

    def add(p):
        pos.append(np.asarray(p, dtype=np.float64))
        return len(pos) - 1
    names["lonely"] = add([0.3, -0.2, 0.9])
    a, b, c = add([0.0, 0.0, 0.0]), add([1.0, 0.1, 0.0]), add([0.2, 1.0, 0.3])
    tri.append((a, b, c))
    names["single"] = a
    hub = add([0.1, 0.2, 0.3])
    ring = [add([np.cos(t) + 0.05 * rng.standard_normal(), np.sin(t) + 0.05 * rng.standard_normal(), 0.3 * rng.standard_normal()])
            for t in np.linspace(0.0, 2.0 * np.pi, 301)[:-1]]
    for k in range(300):
        tri.append((hub, ring[k], ring[(k + 1) % 300]) if k % 7 else (ring[(k + 1) % 300], hub, ring[k]))   # (the hub in every corner position)
    names["hub"] = hub
    t0, t1 = add([0.5, 0.5, -1.0]), add([-0.4, 0.8, -1.2])
    tri += [(t0, t0, t1), (t1, t0, t0), (t0, t1, t0)]
    names["twice"] = t0
    l0, l1, l2 = add([0.0, 0.0, 2.0]), add([0.5, 0.25, 2.125]), add([1.0, 0.5, 2.25])
    tri.append((l0, l1, l2))
    names["line"] = l1
    s = [add(1e-30 * rng.uniform(-1.0, 1.0, 3)) for _ in range(5)]
    tri += [(s[0], s[1], s[2]), (s[0], s[2], s[3]), (s[4], s[0], s[3]), (s[1], s[0], s[4])]
    names["tiny"] = s[0]
    g = [add(4e19 * rng.uniform(0.5, 1.0, 3) * rng.choice([-1.0, 1.0], 3)) for _ in range(5)]
    tri += [(g[0], g[1], g[2]), (g[0], g[2], g[3]), (g[4], g[0], g[3]), (g[1], g[0], g[4])]
    names["huge"] = g[0]
    q = [add([2.0, 0.0, 0.0]), add([2.0, 1.0, 0.0]), add([np.nan, 0.5, 1.0]), add([3.0, 0.5, -1.0])]
    tri += [(q[0], q[1], q[2]), (q[1], q[0], q[3])]
    names["nan"] = q[2]
    # ... and a seeded soup over the ring (the named vertices keep exactly the triangles above): random corners, repeated ones included
    soup = np.array(ring)[rng.integers(0, len(ring), size=(200, 3))]
    tris = np.concatenate([np.array(tri, dtype=np.int64), soup]).astype(np.int32)
    return np.array(pos).astype(np.float32), tris, names
