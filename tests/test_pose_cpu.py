"""Per-body pose without a GPU: the host-built table against exact arithmetic, the numpy reference of the derived values
(tests/pose_ref.py) against LAPACK, the placement round trip against bounds derived here, the binding against the header.

THE MARGIN against numpy.linalg.eigh, and why pose_ref.SWEEPS is what it is.  The reference diagonalises the symmetric 4x4 N with a fixed
number of cyclic Jacobi sweeps in f64 (u = 2^-53).  A rotation computes t, c, s with a handful of roundings and rewrites seven entries
with at most three roundings each: a backward error below 8u ||N||_F, as in tests/test_strain_cpu.py (rotations keep the Frobenius
norm).  Six rotations per sweep, and the ten entries of N are formed with at most two roundings each from A ("+ 16" covers them and the
reading of the diagonal).  So the computed eigenvalues are those of N up to
    d = (48 * sweeps + 16) * u * ||N||_F                                   (Weyl's theorem)
PROVIDED the sweeps have converged: what they leave off the diagonal adds its norm to the error and is NOT in d.  lambda_max is compared
with eigh's within d and GAP within 2d.  The eigenvector of an eigenvalue whose distance to the rest of the spectrum is GAP turns by at
most (perturbation) / GAP (Davis-Kahan), so the unit quaternion is compared, up to sign, within d / GAP.  Where d / GAP exceeds 1e-3 the
orientation is ill-defined in f64 and the row must SAY so: GAP <= 1e3 * d there, and eigh agrees that the gap is that small; such cases
are at most 5 % of the seeded set (the collinear ones: a line has no orientation about itself).  SWEEPS is the smallest count that meets
this on every input below; the test checks both the count in use and that one sweep fewer fails.

The best rotation by another route: Kabsch's, R = U diag(1, 1, det(U V^T)) V^T from the SVD of S m (x - COM) q^T.  The rotation angle
between two unit quaternions is twice their distance as 4-vectors, LAPACK's SVD answers with a backward error of the same form and its
rotation is as sensitive to the same gap: 2 d / GAP for each side, 4 d / GAP in all.  Kabsch's fit starts from CENTRED positions, the row
from moments about the origin, so this comparison (and no other here) also sees what forming A costs: an entry A_ab = S (m x_a) q_b of p
terms is within (p + 2) u S |m x_a q_b| of the exact sum, and the dropped term (MX_a * S m q_b) / MASS is at most |COM_a| (p + 2) u
S |m q_b| (q = r - c0 rounded once per component, the sum of p terms).  N's entries combine at most three of A's, so ||dN||_F <= 12 dA,
dA the largest of those entry bounds, and the angle may differ by another 2 * 12 dA / GAP.  Far from the origin this is the larger part:
the price of raw moments, |COM| / |q| digits, which the header states.

THE PLACEMENT ROUND TRIP.  tests/place_ref.py moves a rest body by a row (Q, PIVOT, OFFSET, LINEAR, ANGULAR): the stored state is
    x_i = R q_i + g + d_i          v_i = LINEAR + w x (x_i - c - d_i) + e_i          (c = PIVOT + OFFSET, g = R (c0 - PIVOT) + c)
with q_i the table's, |d_i| <= delta_i = sqrt(3) * 2^-24 * max |coordinate of x_i| (the f32 store of three components, each within half
an ulp; the f64 roundings in front of it are 2^29 times smaller) and likewise |e_i| <= sqrt(3) * 2^-24 * max |coordinate of v_i|.
  * The pose row's Q minimises S m |R' q - (x - COM)|^2.  With R' = R exp([theta]x), to first order in theta and d the minimum is at
    H theta = tau, tau = S m q x R^T (d - dbar) = S m q x R^T d (S m q = 0), H = S m (|q|^2 I - q q^T) = tr(B) I - B, B = S m q q^T with
    eigenvalues mu_1 <= mu_2 <= mu_3; H's smallest eigenvalue is mu_1 + mu_2.  So |theta| <= (S |m| |q| delta) / (mu_1 + mu_2); the
    bound is twice that, which covers the second-order terms and the Jacobi margin (both smaller by many orders here; printed).
  * v_i - VCOM = w x (x_i - COM) + (eps_i - its mass-weighted mean), eps_i = e_i - w x d_i, |eps_i| <= |e_i| + |w| delta_i.  Hence
    L = Ic w + S m (x - COM) x eps and |OMEGA - w| <= (S |m| |x - COM| |eps|) / lambda_min(Ic); twice that is allowed.
  * VCOM - (LINEAR + w x (COM - c)) = (S m eps) / M: |.| <= (S |m| |eps|) / |M|; twice that is allowed.
These are derived, not measured; nothing is in tolerances.json.  Each test prints observed / bound."""
import os
import re

import numpy as np
import pytest

import place_ref
import pose_ref as R
from conftest import load_f32, load_mesh
from tetsim_amd import _capi as capi

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
U = 2.0 ** -53
DENSITY = 1000.0


def prep_table(verts, tets, first_vert=None, first_tet=None, density=DENSITY):
    """(records, centres) of tetsim_prep_pose_table."""
    C = capi.C
    v = np.ascontiguousarray(verts, dtype=np.float32)
    t = np.ascontiguousarray(tets, dtype=np.int32).reshape(-1, 4)
    fp, ip, up, dp = C.POINTER(C.c_float), C.POINTER(C.c_int32), C.POINTER(C.c_uint32), C.POINTER(C.c_double)
    nb = 1 if first_vert is None else len(first_vert) - 1
    fv = None if first_vert is None else np.ascontiguousarray(first_vert, dtype=np.uint32)
    ft = None if first_tet is None else np.ascontiguousarray(first_tet, dtype=np.uint32)
    rec, cen = np.zeros(len(v), dtype=R.REC), np.full((nb, 3), np.nan)
    rc = capi.lib().tetsim_prep_pose_table(v.ctypes.data_as(fp), len(v), t.ctypes.data_as(ip), len(t), fv.ctypes.data_as(up) if fv is not None else None,
                                           ft.ctypes.data_as(up) if ft is not None else None, nb, density, rec.ctypes.data, cen.ctypes.data_as(dp))
    assert rc == capi.OK, capi.lib().tetsim_last_error(None)
    return rec, cen


def batch_of(names, shifts):
    parts = [((load_mesh(n)[0] + np.asarray(s, np.float32)).astype(np.float32), load_mesh(n)[1]) for n, s in zip(names, shifts)]
    fv = np.concatenate([[0], np.cumsum([len(v) for v, _ in parts])])
    ft = np.concatenate([[0], np.cumsum([len(t) for _, t in parts])])
    return np.concatenate([v for v, _ in parts]), np.concatenate([t + int(o) for (_, t), o in zip(parts, fv)]), fv, ft


# ---- the table ------------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("mesh", ["dragon", "lat4", "mixed", "notets"])
def test_the_host_built_table_is_within_the_rounding_bound_of_its_definition(mesh):
    if mesh == "mixed":
        v, t, fv, ft = batch_of(["lat4", "dragon", "lat4"], [[-3, 0, 0], [0, 0, 0], [3, 0, 0.5]])
    else:
        v, t = load_mesh(mesh)
        t = t if mesh != "notets" else np.zeros((0, 4), np.int32)
        fv = ft = None
    rec, cen = prep_table(v, t, fv, ft)
    ref = R.table(v, t, DENSITY, fv)
    worst = 0.0
    for i in range(len(v)):
        err = abs(R.Fraction(float(rec["m"][i])) - ref["m"][i])
        assert err <= ref["b_m"][i], (i, float(err), float(ref["b_m"][i]))
        worst = max(worst, float(err / ref["b_m"][i]) if ref["b_m"][i] else 0.0)
        for k in range(3):
            err = abs(R.Fraction(float(rec["q"][i, k])) - ref["q"][i][k])
            assert err <= ref["b_q"][i][k], (i, k, float(err), float(ref["b_q"][i][k]))
            worst = max(worst, float(err / ref["b_q"][i][k]) if ref["b_q"][i][k] else 0.0)
    for b in range(len(cen)):
        for k in range(3):
            err = abs(R.Fraction(float(cen[b, k])) - ref["c0"][b][k])
            assert err <= ref["b_c0"][b][k], (b, k, float(err))
            if ref["c0"][b][k] != 0:                               # the second-order terms the bound leaves to its "+ 1"
                assert ref["b_c0"][b][k] / abs(ref["c0"][b][k]) < R.Fraction(1, 10 ** 6) or abs(ref["c0"][b][k]) < 1e-3
    print("%s: worst |error| / bound = %.3g" % (mesh, worst))
    if mesh == "notets":
        assert not rec["m"].any() and not cen.any() and np.array_equal(rec["q"], v.astype(np.float64))
    else:
        assert (rec["m"] > 0).all()
    # the same arithmetic in numpy gives the same bits; a body of a batch has the table it has alone
    tbl, centres = R.table_f64(v, t, DENSITY, fv)
    assert np.array_equal(tbl["m"].view(np.uint64), rec["m"].view(np.uint64)) and np.array_equal(tbl["q"].view(np.uint64), rec["q"].view(np.uint64))
    assert np.array_equal(centres.view(np.uint64), cen.view(np.uint64))
    if mesh == "mixed":
        for b in range(3):
            lo, hi = int(fv[b]), int(fv[b + 1])
            solo, solo_c = prep_table(v[lo:hi], t[int(ft[b]):int(ft[b + 1])] - lo)
            assert np.array_equal(solo.view(np.uint64), rec[lo:hi].view(np.uint64)) and np.array_equal(solo_c[0], cen[b])


# ---- derived() against LAPACK ---------------------------------------------------------------------------------------------------------------
def rotations(rng, k):
    q, r = np.linalg.qr(rng.standard_normal((k, 3, 3)))
    q = q * np.sign(np.diagonal(r, axis1=1, axis2=2))[:, None, :]
    return q * np.linalg.det(q)[:, None, None]


def moments(m, q, x, v):
    """[n, 26] raw moments of n point sets ([n, p] masses, [n, p, 3] q / x / v), plain f64 sums."""
    mx, mv = m[..., None] * x, m[..., None] * v
    cols = [m.sum(1)] + [mx[..., a].sum(1) for a in range(3)] + [mv[..., a].sum(1) for a in range(3)]
    cols += [(mx[..., a] * q[..., c]).sum(1) for a in range(3) for c in range(3)]
    cols += [(m * (x[..., i] * v[..., j] - x[..., j] * v[..., i])).sum(1) for i, j in ((1, 2), (2, 0), (0, 1))]
    cols += [(mx[..., i] * x[..., j]).sum(1) for i, j in ((0, 0), (1, 1), (2, 2), (0, 1), (0, 2), (1, 2))]
    cols += [(m * (q * q).sum(2)).sum(1)]
    return np.stack(cols, axis=1)


KINDS_OF_SET = (("generic", 1700), ("flat", 500), ("collinear", 150), ("mirrored", 450), ("half-turn", 400), ("far", 400), ("deformed", 400))


def seeded_sets(seed=20250):
    """(rows [4000, 26], kind [4000]): point sets of 12 weighted points moved by a rotation and a shift, stored as f32."""
    rng = np.random.default_rng(seed)
    n, p = sum(k for _, k in KINDS_OF_SET), 12
    kind = np.concatenate([[name] * k for name, k in KINDS_OF_SET])
    m = rng.uniform(0.1, 2.0, (n, p))
    r = rng.uniform(-0.5, 0.5, (n, p, 3)) * rng.uniform(0.2, 2.0, (n, 1, 3))
    r[kind == "flat", :, 2] = 0.0
    line = kind == "collinear"
    r[line] = rng.uniform(-1, 1, (line.sum(), p, 1)) * rng.standard_normal((line.sum(), 1, 3))
    half = np.flatnonzero(kind == "half-turn")
    exact = half[:len(half) // 2]                            # small dyadic numbers in +- pairs: c0 = 0 and every product and sum below is exact
    m[exact, :6] = rng.integers(1, 9, (len(exact), 6)) / 4.0
    m[exact, 6:] = m[exact, :6]
    r[exact, :6] = rng.integers(-8, 9, (len(exact), 6, 3)) / 16.0
    r[exact, 6:] = -r[exact, :6]
    q = r - (m[..., None] * r).sum(1, keepdims=True) / m.sum(1)[:, None, None]
    assert np.array_equal(q[exact], r[exact])
    rot = rotations(rng, n)
    axes = np.eye(3)[rng.integers(0, 3, len(half))]
    axes[len(half) // 2:] = rng.standard_normal((len(half) - len(half) // 2, 3))
    axes /= np.linalg.norm(axes, axis=1, keepdims=True)
    rot[half] = 2.0 * axes[:, :, None] * axes[:, None, :] - np.eye(3)
    shape = q.copy()
    shape[kind == "mirrored", :, 0] *= -1.0
    noise = np.where(kind == "deformed", 0.3, 0.02)[:, None, None]
    noise[half[:len(half) // 2]] = 0.0                       # exact half turns about an axis of the frame: w == 0
    shape = shape * (1.0 + noise * rng.standard_normal((n, 1, 3))) + noise * 0.1 * rng.standard_normal((n, p, 3))
    shift = rng.uniform(-2, 2, (n, 1, 3)) * np.where(kind == "far", 500.0, 1.0)[:, None, None]
    shift[half[:len(half) // 2]] = 0.0
    x = (np.einsum("nab,npb->npa", rot, shape) + shift).astype(np.float32).astype(np.float64)
    v = rng.standard_normal((n, p, 3)).astype(np.float32).astype(np.float64)
    return moments(m, q, x, v), kind, (m, q, x)


def dragon_sets():
    v, t = load_mesh("dragon")
    tbl, _ = R.table_f64(v, t, DENSITY)
    names = ("dragon_pos_100.f32", "dragon_grab_pos_60.f32", "dragon_soft_pos_80.f32")
    pos = [load_f32(n).reshape(-1, 3) for n in names]
    rows = np.stack([R.raw_f64(tbl, x, np.zeros_like(x)) for x in pos])
    m, q = tbl["m"], tbl["q"]
    return rows, np.array(["dragon"] * 3), (np.tile(m, (3, 1)), np.tile(q, (3, 1, 1)), np.stack(pos).astype(np.float64))


def rot_of(q):
    x, y, z, w = q[:, 0], q[:, 1], q[:, 2], q[:, 3]
    return np.stack([np.stack([1 - 2 * (y * y + z * z), 2 * (x * y - w * z), 2 * (x * z + w * y)], 1),
                     np.stack([2 * (x * y + w * z), 1 - 2 * (x * x + z * z), 2 * (y * z - w * x)], 1),
                     np.stack([2 * (x * z - w * y), 2 * (y * z + w * x), 1 - 2 * (x * x + y * y)], 1)], 1)


def against_lapack(rows, points, sweeps):
    """Per set: |lambda_max - eigh| / d, |GAP - eigh| / 2d, quaternion distance / (d / GAP), Kabsch angle / (4 d / GAP), ill-defined."""
    detail = {}
    out = R.derived(rows, sweeps, detail)
    N = R.dense(R.horn_matrix(rows))
    norm = np.sqrt((N ** 2).sum(axis=(1, 2)))
    d = (48 * sweeps + 16) * U * norm
    w, vec = np.linalg.eigh(N)
    lam, gap, q = detail["lam"], out[:, R.GAP - R.RAW], out[:, R.Q - R.RAW:R.Q - R.RAW + 4]
    with np.errstate(divide="ignore", invalid="ignore"):
        vec_margin = d / gap
        ill = ~(vec_margin <= 1e-3)
        ref = vec[:, [1, 2, 3, 0], 3]                          # eigh's (w,x,y,z) of the largest eigenvalue, as xyzw
        dist = np.minimum(np.linalg.norm(q - ref, axis=1), np.linalg.norm(q + ref, axis=1)) / vec_margin
        m, qq, x = points
        com = (m[..., None] * x).sum(1, keepdims=True) / m.sum(1)[:, None, None]
        H = np.einsum("np,npa,npb->nab", m, x - com, qq)
        Us, _, Vt = np.linalg.svd(H)
        fix = np.ones((len(H), 3))
        fix[:, 2] = np.sign(np.linalg.det(Us @ Vt))
        kabsch = np.einsum("nab,nb,nbc->nac", Us, fix, Vt)
        rel = np.einsum("nab,ncb->nac", rot_of(q), kabsch)
        cosang = np.clip((np.trace(rel, axis1=1, axis2=2) - 1.0) / 2.0, -1.0, 1.0)
        sinang = np.linalg.norm(np.stack([rel[:, 2, 1] - rel[:, 1, 2], rel[:, 0, 2] - rel[:, 2, 0], rel[:, 1, 0] - rel[:, 0, 1]], 1), axis=1) / 2.0
        p = m.shape[1]
        dA = (p + 2) * U * (np.einsum("np,npa,npb->nab", m, np.abs(x), np.abs(qq)) + np.abs(com[:, 0, :, None]) * np.einsum("np,npb->nb", m, np.abs(qq))[:, None, :]).max(axis=(1, 2))
        angle = np.arctan2(sinang, cosang) / (4.0 * vec_margin + 24.0 * dA / gap)
    return dict(lam=np.abs(lam - w[:, 3]) / d, gap=np.abs(gap - (w[:, 3] - w[:, 2])) / (2 * d), quat=dist, kabsch=angle, ill=ill, d=d, gap_value=gap,
                lapack_gap=w[:, 3] - w[:, 2], off=detail["off"] / norm, out=out, norm=norm)


_SETS = {}


def sets(name):
    if name not in _SETS:
        _SETS[name] = seeded_sets() if name == "seeded" else dragon_sets()
    return _SETS[name]


def worst_of(name, sweeps):
    rows, kind, points = sets(name)
    a = against_lapack(rows, points, sweeps)
    ok = ~a["ill"]
    return a, kind, dict(lam=float(a["lam"].max()), gap=float(a["gap"].max()), quat=float(a["quat"][ok].max()), kabsch=float(a["kabsch"][ok].max()),
                         off=float(a["off"].max()), ill=float(a["ill"].mean()))


@pytest.mark.parametrize("name", ["seeded", "dragon"])
def test_reference_agrees_with_lapack(name):
    rows, kind, _ = sets(name)
    assert np.isfinite(rows).all() and len(rows) == (4000 if name == "seeded" else 3)
    a, kind, worst = worst_of(name, R.SWEEPS)
    print("%s: %d sweeps, worst / margin: lambda_max %.3g, GAP %.3g, quaternion %.3g, Kabsch angle %.3g; off-diagonal left / ||N|| %.3g; ill-defined %.2f %%"
          % (name, R.SWEEPS, worst["lam"], worst["gap"], worst["quat"], worst["kabsch"], worst["off"], 100 * worst["ill"]))
    assert worst["lam"] <= 1.0 and worst["gap"] <= 1.0 and worst["quat"] <= 1.0 and worst["kabsch"] <= 1.0
    # the ill-defined ones say so, LAPACK agrees, and they are few -- the collinear sets, and only those
    ill = a["ill"]
    assert (a["gap_value"][ill] <= 1e3 * a["d"][ill]).all() and (a["lapack_gap"][ill] <= 1e3 * a["d"][ill] + 2 * a["d"][ill]).all()
    assert ill.mean() <= 0.05
    if name == "seeded":
        assert set(kind[ill]) == {"collinear"} and ill[kind == "collinear"].all()
    out = a["out"]
    q = out[:, R.Q - R.RAW:R.Q - R.RAW + 4]
    assert np.allclose(np.linalg.norm(q, axis=1), 1.0, rtol=0, atol=8 * U) and (q[:, 3] >= 0).all()
    flat_w = q[:, 3] == 0
    first = np.where(q[:, 0] != 0, q[:, 0], np.where(q[:, 1] != 0, q[:, 1], q[:, 2]))
    assert (first[flat_w] > 0).all()
    if name == "seeded":
        assert flat_w.sum() >= 100 and set(kind[flat_w]) == {"half-turn"}          # the exact half turns: w == 0 is exercised
        mirrored = kind == "mirrored"
        res = out[:, R.RESIDUAL - R.RAW]
        assert np.allclose(np.linalg.det(rot_of(q)), 1.0, atol=1e-12)             # a proper rotation, also for a mirrored body
        assert np.median(res[mirrored]) > 20 * np.median(res[kind == "generic"])
    assert not out[:, R.RESERVED - R.RAW:].any()


def test_the_sweep_count_is_the_smallest_that_meets_the_margin():
    assert R.SWEEPS == capi.POSE_SWEEPS
    worst = {}
    for s in (R.SWEEPS - 1, R.SWEEPS):
        w = [worst_of(name, s)[2] for name in ("seeded", "dragon")]
        worst[s] = max(max(x["lam"], x["gap"], x["quat"]) for x in w)
    print("worst error / margin by sweeps:", worst)
    assert worst[R.SWEEPS] <= 1.0 < worst[R.SWEEPS - 1]


def test_a_massless_row_and_a_nan_row():
    rows = np.zeros((2, R.RAW))
    rows[0, R.A:R.A + 9] = 3.0                                     # (moments without a mass: not looked at)
    rows[1] = np.nan
    out = R.derived(rows)
    want = np.zeros(R.WIDTH - R.RAW)
    want[R.Q - R.RAW + 3] = 1.0
    assert np.array_equal(out[0].view(np.uint64), want.view(np.uint64))
    assert np.isnan(out[1, :R.RESERVED - R.RAW]).all() and not out[1, R.RESERVED - R.RAW:].any()


# ---- the placement round trip -----------------------------------------------------------------------------------------------------------------
def seeded_place_rows(seed):
    """Three rows: a generic one with w < 0, an exact half turn about y, a generic one."""
    rng = np.random.default_rng(seed)
    q = rng.standard_normal((3, 4))
    q[0, 3] = -abs(q[0, 3])
    q[1] = [0.0, 1.0, 0.0, 0.0]
    q[2, 3] = abs(q[2, 3])
    return [place_ref.np.concatenate([q[k], rng.uniform(-1, 1, 3), rng.uniform(-2, 2, 3), rng.uniform(-3, 3, 3), rng.uniform(-4, 4, 3)]).astype(np.float32)
            for k in range(3)]


def check_placed(label, row, tbl, pos, vel, got):
    """One body's pose row `got` [48] against the motion of `row`; prints observed / bound."""
    M = place_ref.Motion(row)
    angle_b, omega_b, vcom_b, rms = R.placement_bounds(tbl, pos, vel, M.angular)
    angle = R.quat_angle(got[R.Q:R.Q + 4], M.q)
    omega = float(np.linalg.norm(got[R.OMEGA:R.OMEGA + 3] - M.angular))
    com = got[R.COM:R.COM + 3]
    vcom = float(np.linalg.norm(got[R.VCOM:R.VCOM + 3] - (M.linear + np.cross(M.angular, com - M.centre))))
    print("%s: angle %.3g / %.3g, |OMEGA - w| %.3g / %.3g, VCOM %.3g / %.3g, RESIDUAL %.3g (rms delta %.3g), GAP %.3g"
          % (label, angle, angle_b, omega, omega_b, vcom, vcom_b, got[R.RESIDUAL], rms, got[R.GAP]))
    assert angle <= angle_b and omega <= omega_b and vcom <= vcom_b, label
    assert got[R.Q + 3] >= 0
    return rms


@pytest.mark.parametrize("mesh", ["dragon", "lat4"])
def test_a_placed_rest_body_reports_its_placement(mesh):
    v, t = load_mesh(mesh)
    tbl, _ = prep_table(v, t)
    for k, row in enumerate(seeded_place_rows(77)):
        pos, vel = place_ref.place_particles(row, v, np.zeros_like(v))
        got = np.concatenate([R.raw_f64(tbl, pos, vel), np.zeros(R.WIDTH - R.RAW)])
        got[R.RAW:] = R.derived(got)[0]
        check_placed("%s row %d" % (mesh, k), row, tbl, pos, vel, got)
        if k == 1:
            assert abs(got[R.Q + 3]) < 1e-6 and got[R.Q + 1] > 0.999999          # the half turn: (0, 1, 0, ~0), sign fixed


# ---- the binding ------------------------------------------------------------------------------------------------------------------------------
def test_binding_matches_the_header():
    header = open(os.path.join(ROOT, "include", "tetsim.h")).read()
    assert int(re.search(r"#define TETSIM_POSE_WIDTH (\d+)", header).group(1)) == capi.POSE_WIDTH == R.WIDTH == 48
    assert int(re.search(r"#define TETSIM_POSE_SWEEPS (\d+)", header).group(1)) == capi.POSE_SWEEPS == R.SWEEPS
    assert "WHY %d SWEEPS" % R.SWEEPS in header
    names = dict((n, int(v)) for n, v in re.findall(r"TETSIM_(POSE_[A-Z0-9_]+) = (\d+)", header))
    assert names == dict(POSE_MASS=0, POSE_MX=1, POSE_MV=4, POSE_A=7, POSE_L0=16, POSE_G=19, POSE_Q0=25, POSE_COM=26, POSE_VCOM=29, POSE_Q=32,
                         POSE_OMEGA=36, POSE_L=39, POSE_RESIDUAL=42, POSE_GAP=43, POSE_RESERVED=44)
    for n, v in names.items():
        assert getattr(capi, n) == v == getattr(R, n[5:]), n
    L = capi.lib()
    for s in ("tetsim_body_poses_device", "tetsim_read_body_poses", "tetsim_prep_pose_table"):
        assert s in capi.SYMBOLS and s in capi.OPTIONAL_SYMBOLS and hasattr(L, s), s
    from tetsim_amd import SoftBodyHIP
    assert callable(SoftBodyHIP.observePoses) and callable(SoftBodyHIP.bodyPoses)


def test_entry_points_refuse_bad_arguments():
    L, C = capi.lib(), capi.C
    out = np.zeros(48)
    assert L.tetsim_body_poses_device(None, None, 0, None) == capi.EINVAL
    assert L.tetsim_body_poses_device(None, out.ctypes.data, 384, None) == capi.EINVAL
    assert L.tetsim_read_body_poses(None, out.ctypes.data_as(C.POINTER(C.c_double))) == capi.EINVAL
    assert not out.any()
    v, t = load_mesh("lat4")
    fp, ip, up = C.POINTER(C.c_float), C.POINTER(C.c_int32), C.POINTER(C.c_uint32)
    args = (v.ctypes.data_as(fp), len(v), t.ctypes.data_as(ip), len(t))
    rec = np.zeros(len(v), R.REC)
    assert L.tetsim_prep_pose_table(*args, None, None, 1, DENSITY, None, None) == capi.EINVAL
    fv = np.array([0, len(v)], np.uint32)
    assert L.tetsim_prep_pose_table(*args, fv.ctypes.data_as(up), None, 1, DENSITY, rec.ctypes.data, None) == capi.EINVAL
    ft = np.array([0, len(t) - 1], np.uint32)
    assert L.tetsim_prep_pose_table(*args, fv.ctypes.data_as(up), ft.ctypes.data_as(up), 1, DENSITY, rec.ctypes.data, None) == capi.EINVAL
    bad = t.copy()
    bad[3, 2] = len(v)
    assert L.tetsim_prep_pose_table(args[0], args[1], bad.ctypes.data_as(ip), len(bad), None, None, 1, DENSITY, rec.ctypes.data, None) == capi.EINVAL
    assert not rec["m"].any()
    assert L.tetsim_prep_pose_table(*args, None, None, 1, DENSITY, rec.ctypes.data, None) == capi.OK and (rec["m"] > 0).all()
