"""Per-tet strain without a GPU: the numpy reference (tests/strain_ref.py) against LAPACK and on geometry whose answer is known exactly,
the binding against the header, the entry points' refusal of a NULL handle, and the host-built table against tetsim_prep_rest.

THE MARGIN against numpy.linalg.svd, and why strain_ref.SWEEPS is 4.  The reference forms C = F^T F and diagonalises it with a fixed
number of cyclic Jacobi sweeps, all in f64 (u = 2^-53).  Forming C perturbs each entry by at most 3u |F|^T|F| <= 3u trace(C); a rotation
computes t, c, s with a handful of roundings and rewrites five entries with at most three roundings each, a backward error below
8u trace(C) (every entry of C is at most trace(C) in size, and stays so: rotations keep the Frobenius norm); the three square roots and
the reading of the diagonal take the rest of the "+ 8".  So the computed eigenvalues are those of C up to
    d = (24 * sweeps + 8) * u * trace(C)                                  (3 rotations per sweep, 8u each; Weyl's theorem)
PROVIDED the sweeps have converged: what they leave off the diagonal adds its norm to the error and is NOT in d.  A stretch is sqrt(e),
and |sqrt(a) - sqrt(b)| = |a - b| / (sqrt(a) + sqrt(b)) is at most both |a - b| / sqrt(b) and sqrt|a - b|; LAPACK's own sigma is within a
few u * sigma_max of the truth.  Hence the test allows, per stretch,
    min(d / sigma, sqrt(d)) + 4u * sigma_max.
SWEEPS is the smallest count that meets this on every input below: 3 sweeps miss it (22x on the seeded set, 1,000x on a Dragon state:
not converged), 4 meet it with the worst stretch at 0.11 of the margin and less than 3e-7 * u * trace(C) left off the diagonal; the test
checks both the count in use and that one sweep fewer fails, so the count cannot drift from its reason.  J is compared with
numpy.linalg.det within 32u * |F|_F^3: six products of three factors with at most five roundings each on our side (|each product| <=
|F|_F^3 / 3^1.5, so 6 * 5 / 5.2 < 6), and as much again five times over for LU with partial pivoting."""
import os
import re

import numpy as np
import pytest

import strain_ref as R
from conftest import load_f32, load_mesh
from tetsim_amd import _capi as capi
from tetsim_amd import make_lattice

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
U = 2.0 ** -53
REC = np.dtype([("ids", "<i4", (4,)), ("irp", "<f4", (9,)), ("degenerate", "<u4"), ("abs_v0", "<f8")])


def prep_rest(verts, tets, density=1000.0):
    """(invMass, invRestPose [nt, 9], invRestVolume) of the library's host preprocessing."""
    v = np.ascontiguousarray(verts, dtype=np.float32)
    t = np.ascontiguousarray(tets, dtype=np.int32)
    fp, ip = capi.C.POINTER(capi.C.c_float), capi.C.POINTER(capi.C.c_int32)
    im, irp, irv = np.zeros(len(v), np.float32), np.zeros((len(t), 9), np.float32), np.zeros(len(t), np.float32)
    rc = capi.lib().tetsim_prep_rest(v.ctypes.data_as(fp), len(v), t.ctypes.data_as(ip), len(t), density, im.ctypes.data_as(fp),
                                     irp.ctypes.data_as(fp), irv.ctypes.data_as(fp))
    assert rc == capi.OK
    return im, irp, irv


def strain_table(verts, tets, density=1000.0):
    v = np.ascontiguousarray(verts, dtype=np.float32)
    t = np.ascontiguousarray(tets, dtype=np.int32)
    fp, ip = capi.C.POINTER(capi.C.c_float), capi.C.POINTER(capi.C.c_int32)
    out = np.zeros(len(t), dtype=REC)
    assert capi.lib().tetsim_prep_strain_table(v.ctypes.data_as(fp), len(v), t.ctypes.data_as(ip), len(t), density, out.ctypes.data) == capi.OK
    return out


def seeded_F(n=4000, seed=20240):
    """[n, 9] column-major F = U diag(s) V^T, rounded to f32 values: singular values over six decades with condition numbers up to
    1e6, an eighth with a nearly equal pair, 200 of rank 2, 100 of rank 1, 100 rotations, every third with J < 0."""
    rng = np.random.default_rng(seed)

    def rotations(k):
        q, r = np.linalg.qr(rng.standard_normal((k, 3, 3)))
        return q * np.sign(np.diagonal(r, axis1=1, axis2=2))[:, None, :]

    Uu, V = rotations(n), rotations(n)
    s = np.sort(10.0 ** rng.uniform(-3, 3, (n, 3)), axis=1)[:, ::-1]
    s[:, 2] = np.maximum(s[:, 2], s[:, 0] * 1e-6)
    s[:, 1] = np.maximum(s[:, 1], s[:, 2])
    s[n // 8: n // 4, 1] = s[n // 8: n // 4, 0] * (1 + 1e-9 * rng.standard_normal(n // 4 - n // 8))
    s[n // 4: n // 4 + 200, 2] = 0.0
    s[n // 4 + 200: n // 4 + 300, 1:] = 0.0
    s[-100:] = 1.0
    s[::3, 2] *= -1.0
    F = np.einsum("nij,nj,nkj->nik", Uu, s, V).astype(np.float32).astype(np.float64)
    return F.transpose(0, 2, 1).reshape(n, 9)


def dragon_F(name):
    _, t = load_mesh("dragon")
    return R.deformation_gradient(load_f32(name).reshape(-1, 3), t, load_f32("dragon_invRestPose.f32"))


def against_lapack(F9, sweeps):
    """(worst |stretch - sigma| / margin, worst |J - det| / margin, worst off-diagonal norm left / (u trace C))."""
    off = []
    v = R.values_from_F(F9, sweeps, off)
    M = F9.reshape(-1, 3, 3).transpose(0, 2, 1)
    sigma = np.linalg.svd(M, compute_uv=False)
    trace = (M ** 2).sum(axis=(1, 2))
    d = (24 * sweeps + 8) * U * trace
    with np.errstate(divide="ignore"):
        allow = np.minimum(d[:, None] / sigma, np.sqrt(d)[:, None]) + 4 * U * sigma[:, :1]
    stretch = np.abs(v[:, R.STRETCH_AT:R.STRETCH_AT + 3] - sigma) / allow
    det = np.abs(v[:, R.J_AT] - np.linalg.det(M)) / (32 * U * trace ** 1.5)
    return float(stretch.max()), float(det.max()), float((off[0] / (U * trace)).max())


INPUTS = {"seeded": seeded_F, "dragon_pos_100": lambda: dragon_F("dragon_pos_100.f32"), "dragon_grab_pos_60": lambda: dragon_F("dragon_grab_pos_60.f32"),
          "dragon_soft_pos_80": lambda: dragon_F("dragon_soft_pos_80.f32")}


@pytest.mark.parametrize("name", list(INPUTS))
def test_reference_agrees_with_lapack(name):
    F9 = INPUTS[name]()
    assert len(F9) >= 3840 and np.isfinite(F9).all()
    stretch, det, off = against_lapack(F9, R.SWEEPS)
    print("%s: %d sweeps, worst stretch error / margin %.3g, worst J error / margin %.3g, off-diagonal left / (u trace C) %.3g" % (name, R.SWEEPS, stretch, det, off))
    assert stretch <= 1.0 and det <= 1.0
    v = R.values_from_F(F9)
    s = v[:, R.STRETCH_AT:R.STRETCH_AT + 3]
    assert (s[:, 0] >= s[:, 1]).all() and (s[:, 1] >= s[:, 2]).all() and (s[:, 2] >= 0).all()
    # DEV^2 = the sum of the squared stretches, GREEN^2 = the sum of ((stretch^2 - 1) / 2)^2: the same invariants of C by another route
    assert np.allclose(v[:, R.DEV_AT] ** 2, (s ** 2).sum(axis=1), rtol=1e-12)
    assert np.allclose(v[:, R.GREEN_AT] ** 2, (((s ** 2 - 1) / 2) ** 2).sum(axis=1), rtol=1e-9, atol=1e-18)


def test_the_sweep_count_is_the_smallest_that_meets_the_margin():
    assert R.SWEEPS == capi.STRAIN_SWEEPS == 4
    worst = {s: max(against_lapack(make(), s)[0] for make in INPUTS.values()) for s in (R.SWEEPS - 1, R.SWEEPS)}
    print("worst stretch error / margin by sweeps:", worst)
    assert worst[R.SWEEPS] <= 1.0 < worst[R.SWEEPS - 1]


def integer_lattice():
    """2 x 2 x 2 cells of side 2 from the origin: small integers, so every edge, every determinant (8) and B (entries 0, +-1/2) are exact."""
    v, t = make_lattice(2, y0=0.5)
    v = ((v - v.min(axis=0)).astype(np.float64) * 4.0).astype(np.float32)
    assert np.array_equal(v, np.round(v)) and v.min() == 0 and v.max() == 4
    return v, t


def test_an_exact_stretch_on_a_small_integer_lattice():
    v, t = integer_lattice()
    _, irp, _ = prep_rest(v, t)
    assert np.isin(irp, (0.0, 0.5, -0.5)).all() and not R.degenerate_tets(v, t, irp).any()
    pos = v * np.array([2.0, 1.0, 1.0], np.float32)
    val = R.tet_values(pos, t, irp)
    rows = R.tet_rows(val)
    want = np.zeros(16, np.float32)
    want[[0, 4, 8]] = (2, 1, 1)
    want[R.J_AT], want[R.DEV_AT], want[R.GREEN_AT] = 2, np.float32(np.sqrt(6.0)), 1.5
    want[R.STRETCH_AT:R.STRETCH_AT + 3] = (2, 1, 1)
    assert np.array_equal(rows.view(np.uint32), np.tile(want, (len(t), 1)).view(np.uint32))
    assert np.array_equal(val[:, R.GREEN_AT], np.full(len(t), 1.5)) and np.array_equal(val[:, R.J_AT], np.full(len(t), 2.0))
    body = R.body_rows(val, rows, R.rest_volume(v, t), np.zeros(len(t), bool))
    v0 = 8.0 / 6.0                                                   # every tet; the sums are those of 48 equal terms in the tree's order
    assert body.shape == (1, 8) and list(body[0, :5]) == [2.0, 1.0, 2.0, 2.0, 1.5] and body[0, 7] == 0
    assert abs(body[0, 6] - 48 * v0) <= 48 * U * 48 * v0 and abs(body[0, 5] - 48 * v0 * 2.25) <= 48 * U * 48 * v0 * 2.25


def test_a_rigid_motion_has_no_strain():
    v, t = integer_lattice()
    _, irp, _ = prep_rest(v, t)
    rot = np.array([[0, -1, 0], [1, 0, 0], [0, 0, 1]], np.float32)   # 90 degrees about z
    pos = (v @ rot.T + np.array([7.0, -3.0, 11.0], np.float32)).astype(np.float32)
    val = R.tet_values(pos, t, irp)
    assert np.array_equal(val[:, :9], np.tile(rot.T.reshape(-1).astype(np.float64), (len(t), 1)))   # column-major F = the rotation
    assert (val[:, R.GREEN_AT] == 0).all() and (val[:, R.STRETCH_AT:R.STRETCH_AT + 3] == 1).all() and (val[:, R.J_AT] == 1).all()
    assert (val[:, R.DEV_AT] == np.sqrt(3.0)).all()
    assert (R.tet_rows(val)[:, R.RESERVED_AT] == 0).all()


def test_degenerate_and_nonfinite_tets_are_left_out_of_the_body_row():
    v, t = integer_lattice()
    v = np.concatenate([v, [[9, 9, 9]]]).astype(np.float32)
    t = np.concatenate([[[0, 1, 2, 2]], t]).astype(np.int32)          # tet 0: two equal corners, volume 0 (tet 0 is also the one whose
    _, irp, _ = prep_rest(v, t)                                      # cleared invRestPose the reference's clearing bug leaves in place)
    deg = R.degenerate_tets(v, t, irp)
    assert deg[0] and not deg[1:].any()
    pos = v.copy()
    pos[int(t[5, 1])] = np.nan
    val = R.tet_values(pos, t, irp)
    rows = R.tet_rows(val, deg)
    hit = (t == t[5, 1]).any(axis=1)
    hit[0] = False
    assert np.isnan(rows[0, :15]).all() and rows[0, 15] == 0 and np.isnan(rows[hit, R.J_AT]).all() and np.isfinite(rows[~hit & ~deg]).all()
    body = R.body_rows(val, rows, R.rest_volume(v, t), deg)
    assert body[0, 7] == 1 + hit.sum() and list(body[0, :5]) == [1.0, 1.0, 1.0, 1.0, 0.0] and body[0, 5] == 0
    none = R.body_rows(val[:1], rows[:1], R.rest_volume(v, t[:1]), deg[:1])
    assert list(none[0]) == [-np.inf, np.inf, np.inf, -np.inf, -np.inf, 0.0, 0.0, 1.0]


@pytest.mark.parametrize("mesh", ["dragon", "lat2degen"])
def test_the_host_built_table_is_prep_rest_and_the_observations_volume(mesh):
    v, t = load_mesh(mesh)
    _, irp, _ = prep_rest(v, t)
    rec = strain_table(v, t)
    assert rec.dtype.itemsize == 64 and np.array_equal(rec["ids"], t)
    assert np.array_equal(rec["irp"].view(np.uint32), irp.view(np.uint32))
    v0 = R.rest_volume(v, t)
    assert np.array_equal(rec["abs_v0"], np.abs(v0))
    assert np.array_equal(rec["degenerate"].astype(bool), R.degenerate_tets(v, t, irp))
    assert rec["degenerate"].any() == (mesh == "lat2degen")


def test_binding_matches_the_header():
    header = open(os.path.join(ROOT, "include", "tetsim.h")).read()
    for name, value in (("WIDTH", 16), ("BODY_WIDTH", 8), ("SWEEPS", 4)):
        assert int(re.search(r"#define TETSIM_STRAIN_%s (\d+)" % name, header).group(1)) == getattr(capi, "STRAIN_" + name) == value
    names = dict((n, int(v)) for n, v in re.findall(r"TETSIM_(STRAIN_[A-Z0-9_]+) = (\d+)", header))
    assert names == dict(STRAIN_F=0, STRAIN_J=9, STRAIN_DEV=10, STRAIN_STRETCH=11, STRAIN_GREEN=14, STRAIN_RESERVED=15)
    for n, v in names.items():
        assert getattr(capi, n) == v, n
    assert (R.WIDTH, R.BODY_WIDTH, R.J_AT, R.DEV_AT, R.STRETCH_AT, R.GREEN_AT, R.RESERVED_AT) == (16, 8, 9, 10, 11, 14, 15)
    L = capi.lib()
    for s in ("tetsim_tet_strain_device", "tetsim_read_tet_strain", "tetsim_body_strain_device", "tetsim_visual_strain_device", "tetsim_prep_strain_table"):
        assert s in capi.SYMBOLS and s in capi.OPTIONAL_SYMBOLS and hasattr(L, s), s
    from tetsim_amd.softbody import _STRAIN_CHANNELS
    assert sorted(_STRAIN_CHANNELS.values()) == list(range(15)) and _STRAIN_CHANNELS["F01"] == 3 and _STRAIN_CHANNELS["green"] == 14


def test_entry_points_refuse_null_arguments():
    L = capi.lib()
    out = np.zeros(16, np.float32)
    p = out.ctypes.data
    assert L.tetsim_tet_strain_device(None, None, 0, None) == capi.EINVAL
    assert L.tetsim_tet_strain_device(None, p, 64, None) == capi.EINVAL
    assert L.tetsim_body_strain_device(None, p, 64, None) == capi.EINVAL
    assert L.tetsim_visual_strain_device(None, 0, p, 4, None) == capi.EINVAL
    assert L.tetsim_read_tet_strain(None, out.ctypes.data_as(capi.C.POINTER(capi.C.c_float))) == capi.EINVAL
    assert not out.any()
    v, t = load_mesh("lat4")
    fp, ip = capi.C.POINTER(capi.C.c_float), capi.C.POINTER(capi.C.c_int32)
    assert L.tetsim_prep_strain_table(v.ctypes.data_as(fp), len(v), t.ctypes.data_as(ip), len(t), 1000.0, None) == capi.EINVAL
    bad = t.copy()
    bad[3, 2] = len(v)
    assert L.tetsim_prep_strain_table(v.ctypes.data_as(fp), len(v), bad.ctypes.data_as(ip), len(bad), 1000.0, np.zeros(len(t), REC).ctypes.data) == capi.EINVAL
