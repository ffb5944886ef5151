"""tests/skin_ref.py is itself checked, without a GPU: against the reference's recorded output, against plain high precision, and for
what tests/test_gpu_skin_exact.py relies on (the twisted start really gives every tet a rotation of its own; the edge inputs really
hold the edges).  The normals' tie to the recorded three.js output is tests/test_oracle_golden.py::
test_vertex_normals_golden_is_threejs_computeVertexNormals."""
import numpy as np
import pytest

import skin_ref as R
from conftest import load_f32, load_mesh
from oracle import OraclePJ
from tetsim_amd import make_lattice

LD = np.longdouble
PP0, DT = R.TWIST_PP, R.TWIST_DT


def gamma(n):
    """(1 + d1) .. (1 + dn) = 1 + t with |t| <= n u / (1 - n u), |di| <= u = 2^-24 (Higham, Accuracy and Stability, lemma 3.1)."""
    return n * R.U32 / (1.0 - n * R.U32)


def oracle_quats_after_twist(v, t, substeps=R.TWIST_SUBSTEPS):
    """The reference's solver (OraclePJ) started from skin_ref.twisted_start, gravity off: (positions, quaternions) after `substeps`."""
    orc = OraclePJ(v, t, PP0)
    orc.writeParticles(np.arange(len(v)), R.twisted_start(v), np.zeros_like(v))
    for _ in range(substeps):
        orc.simulate(DT, PP0)
    return orc.pos, orc.quats


def test_skin_js_equals_the_recorded_js_output():
    """updateVisMesh inside the reference, recorded by tests/golden/make_golden.mjs after 10 substeps of the Dragon: bit for bit."""
    _, t = load_mesh("dragon")
    pos = load_f32("dragon_pos_10.f32").reshape(-1, 3)
    vis = load_f32("dragon_vis.f32").reshape(-1, 4)
    assert R.same_bits(R.skin_js(pos, t, vis), load_f32("dragon_vispos_10.f32").reshape(-1, 3))


def _skin_inputs():
    v, t = load_mesh("dragon")
    pos = R.twisted_start(v)
    vis = np.concatenate([load_f32("dragon_vis.f32").reshape(-1, 4)[::7], R.edge_vis_rows(len(t), 600), R.one_tet_vis_rows(len(t) // 2)])
    lv, lt = make_lattice(4, y0=0.0)          # (a lattice has coordinates of exactly 0: products that are exactly 0, and subnormal ones next to them)
    return [(pos, t, vis), (lv, lt, R.edge_vis_rows(len(lt), 300, seed=1))]


def test_skin_f32_against_high_precision():
    """4 products and 3 sums: every product goes through its own rounding and at most 3 of the sums, (1 + d)^4, so the f32 result is
    within gamma(4) sum_k |p_k| |b_k| of the exact sum of products -- inside the 7 * 2^-24 * sum_k |p_k| |b_k| asserted here.  b3 is an
    input of that sum as the f32 it is; its own three roundings are bounded separately: the two sums inside by gamma(2) (|b0| + |b1| +
    |b2|), the subtraction from 1 by u |b3|.  A product below the smallest normal f32 (denormal weights) rounds to a multiple of 2^-149
    instead: such rows get 4 * 2^-150 on top, half a spacing per product (the sums of such numbers are exact)."""
    normal_rows = underflow_rows = 0
    for pos, t, vis in _skin_inputs():
        got = R.skin_f32(pos, t, vis).astype(LD)
        e = vis[:, 0].astype(np.int64)
        b = [vis[:, k].astype(LD) for k in (1, 2, 3)]
        b3_f32 = np.float32(1.0) - ((vis[:, 1] + vis[:, 2]) + vis[:, 3])
        b3_exact = LD(1.0) - ((b[0] + b[1]) + b[2])
        assert np.all(np.abs(b3_f32.astype(LD) - b3_exact) <= gamma(2) * (np.abs(b[0]) + np.abs(b[1]) + np.abs(b[2])) + R.U32 * np.abs(b3_f32).astype(LD))
        b.append(b3_f32.astype(LD))
        p = [pos[t[e, k]].astype(LD) for k in range(4)]
        prod = [p[k] * b[k][:, None] for k in range(4)]
        exact = ((prod[0] + prod[1]) + prod[2]) + prod[3]
        mag = sum(np.abs(x) for x in prod)
        under = np.zeros(len(vis), bool)
        for x in prod:
            under |= ((np.abs(x) < R.TINY32) & (x != 0)).any(axis=1)
        bound = 7 * LD(R.U32) * mag + np.where(under, 4 * 2.0 ** -150, 0.0)[:, None]
        assert np.all(np.abs(got - exact) <= bound)
        normal_rows += int((~under).sum())
        underflow_rows += int(under.sum())
    assert normal_rows > 5000 and underflow_rows >= 3      # both kinds of row were there


def test_rotate_normals_f32_against_high_precision():
    """With |.| for the sums of absolute values: i.x = (q.y n.z - n.y q.z) + q.w n.x is 3 products under at most 2 sums each, so within
    gamma(3) I.x, I.x = |q.y n.z| + |n.y q.z| + |q.w n.x|.  T.x = q.y i.z - i.y q.z multiplies those errors by |q.y|, |q.z| and adds a
    product and a difference, (1 + gamma(3)) (1 + d)^2 <= 1 + gamma(5): within gamma(5) (|q.y| I.z + |q.z| I.y).  Doubling is exact.  The last
    sum adds one rounding of the whole: out.x is within gamma(6) (|n.x| + 2 (|q.y| I.z + |q.z| I.y)) of the exact value, and so on
    cyclically.  Unit vectors and unit quaternions: a product can underflow only next to terms of normal size, and then by less than
    2^-149 for each of the 5 products behind a component (doubled once): 10 * 2^-149 is added."""
    rng = np.random.default_rng(3)
    _, q = oracle_quats_after_twist(*load_mesh("lat4"))
    q = np.concatenate([q, np.float32([[0, 0, 0, 1], [1, 0, 0, 0], [0, -1, 0, 0], [0.5, 0.5, 0.5, 0.5], [0, 0, 1e-30, 1]])])
    q = q[rng.integers(0, len(q), size=4000)]
    n = R.unit_normals(4000, seed=4)
    n[:3] = np.eye(3, dtype=np.float32)
    got = R.rotate_normals_f32(n, q).astype(LD)
    N, Q = n.astype(LD), q.astype(LD)
    w = Q[:, 3:4]
    yzx, zxy = [1, 2, 0], [2, 0, 1]
    i_exact = (Q[:, yzx] * N[:, zxy] - N[:, yzx] * Q[:, zxy]) + w * N
    exact = N + 2 * (Q[:, yzx] * i_exact[:, zxy] - i_exact[:, yzx] * Q[:, zxy])
    aQ, aN = np.abs(Q[:, :3]), np.abs(N)
    I = aQ[:, yzx] * aN[:, zxy] + aN[:, yzx] * aQ[:, zxy] + np.abs(w) * aN
    bound = gamma(6) * (aN + 2 * (aQ[:, yzx] * I[:, zxy] + I[:, yzx] * aQ[:, zxy])) + 10 * 2.0 ** -149
    assert np.all(np.abs(got - exact) <= bound)
    # ... and it is a rotation: the textbook form n + 2 q.xyz x (q.xyz x n + w n) in f64, to the same bound
    qv = q[:, :3].astype(np.float64)
    text = n + 2.0 * np.cross(qv, np.cross(qv, n.astype(np.float64)) + q[:, 3:].astype(np.float64) * n)
    assert np.all(np.abs(got - text) <= bound + 1e-15)


@pytest.mark.parametrize("name", R.TWIST_MESHES)
def test_the_twisted_start_gives_every_tet_its_own_rotation(name):
    """What keeps test_gpu_skin_exact.py from being vacuous, shown on the reference's solver alone: after 5 substeps from the twisted
    start at least 99 % of the quaternions are distinct bit patterns, and for at least half of the visual rows the rotated normal
    differs from the rest normal by more than 0.1 in some component."""
    v, t = R.twist_mesh(name)
    pos, q = oracle_quats_after_twist(v, t)
    assert np.isfinite(pos).all() and np.isfinite(q).all()
    assert R.distinct_rows(q) >= 0.99
    vis = R.edge_vis_rows(len(t), 2000)
    n0 = R.unit_normals(len(vis))
    assert R.normals_moved(n0, R.rotate_normals_f32(n0, q[vis[:, 0].astype(np.int64)])) >= 0.5
    # ... and on lat4 with the row counts of test_visual_rows_at_the_edges that carry this condition there
    if name == "lat4":
        for count in (255, 256, 257):
            rows = R.edge_vis_rows(len(t), count)
            k0 = R.unit_normals(count, seed=9)
            assert R.normals_moved(k0, R.rotate_normals_f32(k0, q[rows[:, 0].astype(np.int64)])) >= 0.5
    wb = PP0["worldBounds"]
    assert (pos > np.float32(wb[:3]) + 0.05).all() and (pos < np.float32(wb[3:]) - 0.05).all()     # away from the walls


def test_edge_vis_rows_hold_the_edges():
    nt = 384
    for count in (1, 255, 256, 257):
        assert R.edge_vis_rows(nt, count).shape == (count, 4)
    assert R.same_bits(R.edge_vis_rows(nt, 257)[:16], R.edge_vis_rows(nt, 255)[:16])   # the special rows come first at every count
    vis = R.edge_vis_rows(nt, 257)
    tet, w = vis[:, 0], vis[:, 1:]
    assert tet[0] == 0 and tet[1] == nt - 1 and set(tet.astype(int)) <= set(range(nt)) and len(set(tet.astype(int))) > 100
    b3 = np.float32(1.0) - ((w[:, 0] + w[:, 1]) + w[:, 2])
    assert (w == 1.0).any() and ((w == 0.0).all(axis=1)).any()
    assert (w == np.float32(-0.5)).any() and (w == np.float32(1.7)).any() and (b3 < -3.0).any() and (b3 > 2.0).any()
    assert (b3 == 0.0).any() and ((b3 != 0.0) & (np.abs(b3) < 1e-6)).any()               # cancels exactly, and to rounding
    assert ((w != 0.0) & (np.abs(w) < R.TINY32)).sum() >= 6                              # denormal
    one = R.one_tet_vis_rows(17)
    assert one.shape == (300, 4) and (one[:, 0] == 17).all()


def test_edge_triangle_soup_holds_the_edges():
    pos, tri, names = R.edge_triangle_soup()
    count = np.bincount(tri.ravel(), minlength=len(pos))
    assert count[names["lonely"]] == 0 and count[names["single"]] == 1 and count[names["hub"]] == 300
    assert any(len(set(r)) < 3 and names["twice"] in r for r in tri.tolist())
    n = R.vertex_normals_threejs(pos, tri)
    zero = np.zeros(3, np.float32)
    assert np.array_equal(n[names["lonely"]], zero) and np.array_equal(n[names["twice"]], zero) and np.array_equal(n[names["line"]], zero)
    assert np.array_equal(n[names["tiny"]], zero) and np.signbit(n[names["tiny"]]).any()        # underflow keeps the sign: -0 is there
    assert abs(np.linalg.norm(n[names["hub"]].astype(np.float64)) - 1.0) < 1e-6
    assert abs(np.linalg.norm(n[names["single"]].astype(np.float64)) - 1.0) < 1e-6
    assert np.isnan(n[names["huge"]]).any()
    k = n[names["nan"]]
    assert np.isnan(k).any() and np.isfinite(k).any() and np.abs(k[np.isfinite(k)]).max() > 0    # `|| 1`: the finite components survive unscaled
    assert np.isfinite(np.delete(n, np.flatnonzero(np.isnan(n).any(axis=1)), axis=0)).all()
