"""The per-body pose of include/tetsim.h (tetsim_body_poses_device) three ways.

    table(rest, tets, density, first_vert)   THE TABLE in exact arithmetic (Fractions; the tets' determinants as Python integers over one
                                             power-of-two denominator, as observe_ref does): m, c0, q, and next to each the largest
                                             |f64 value - exact| that the header's f64 evaluation allows.  The roundings are counted as
                                             observe_ref.bounds counts them: c * 2^-53 * S, S the sum of the absolute values of all
                                             products that enter the value, c the roundings on the longest path + the terms added up.
    raw(tbl, pos, vel, ranges)               the raw moments [0..25] as exact sums over Fractions of the f64 table (taken as it is: what
                                             the device reads) and the f32 state, with S per value; raw_bounds(o) = c * 2^-53 * S with
                                             c = the roundings on the term's path (PATH) + the body's particle count.
    derived(rows)                            THE ROW, PART 2 in numpy f64, expression for expression: only + - * / sqrt, comparisons, fabs
                                             and negation, every operation rounded once (numpy never fuses a multiply with an add), which
                                             IEEE 754 rounds the same on the host and on the device: [26..47] BIT FOR BIT.
and the bounds of a placed rest body that tests/test_pose_cpu.py derives (placement_bounds)."""
import math
from fractions import Fraction

import numpy as np

import observe_ref
from observe_ref import SCALE, U, _det_and_s, _ints

SWEEPS = 5
WIDTH, RAW = 48, 26
MASS, MX, MV, A, L0, G, Q0, COM, VCOM, Q, OMEGA, L, RESIDUAL, GAP, RESERVED = 0, 1, 4, 7, 16, 19, 25, 26, 29, 32, 36, 39, 42, 43, 44
REC = np.dtype([("m", "<f8"), ("q", "<f8", (3,))])
PAIRS = ((0, 1), (0, 2), (0, 3), (1, 2), (1, 3), (2, 3))
# roundings on the longest path into one particle's term of each raw value (the f32 -> f64 conversions and the products of two f32
# values are exact): m | m*x | (m*x)*q | x.y*v.z - x.z*v.y, m * (..) | (m*x)*x | three squares' two sums after a product, m * (..)
PATH = [0] + [1] * 6 + [2] * 9 + [2] * 3 + [2] * 6 + [4]
R_W = observe_ref.R_W


# ---- the table, exactly -----------------------------------------------------------------------------------------------------------------
def table(rest, tets, density, first_vert=None):
    """dict(m [nv], c0 [bodies][3], q [nv][3]: Fractions; b_m, b_c0, b_q: the bounds of their f64 values, Fractions)."""
    nv = len(rest)
    first_vert = [0, nv] if first_vert is None else [int(x) for x in first_vert]
    rho = Fraction(float(density))
    R = _ints(rest)
    unit = rho / (24 * SCALE ** 3)                        # a rest determinant's integer -> w
    d_sum, s_sum, val = [0] * nv, [0] * nv, [0] * nv
    for ids in np.asarray(tets).reshape(-1, 4).tolist():
        d0, s0 = _det_and_s(*(R[i] for i in ids))
        for i in ids:                                     # corner by corner: a particle named twice by a tet gets w twice
            d_sum[i] += d0
            s_sum[i] += s0
            val[i] += 1
    m = [unit * d for d in d_sum]
    s_m = [abs(unit) * s for s in s_sum]
    b_m = [(R_W + v) * U * s for v, s in zip(val, s_m)]  # w's roundings (observe_ref) + the additions
    r = [[Fraction(c, SCALE) for c in row] for row in R]
    c0, b_c0, q, b_q = [], [], [None] * nv, [None] * nv
    for b in range(len(first_vert) - 1):
        lo, hi = first_vert[b], first_vert[b + 1]
        n, deep = hi - lo, max(val[lo:hi], default=0)
        m0, s_m0 = sum(m[lo:hi], Fraction(0)), sum(s_m[lo:hi], Fraction(0))
        cb, bb = [Fraction(0)] * 3, [Fraction(0)] * 3
        if m0 != 0:
            for k in range(3):
                num = sum((m[i] * r[i][k] for i in range(lo, hi)), Fraction(0))
                s_num = sum((s_m[i] * abs(r[i][k]) for i in range(lo, hi)), Fraction(0))
                cb[k] = num / m0
                # N / M off by a in N and b in M: a / M - (N / M) * b / M.  The numerator's path: m (R_W + its additions), the product, n
                # additions; + the division; + 1 for the second-order terms (checked to be tiny by the test, as observe_ref's is)
                bb[k] = (R_W + deep + 1 + n + 2) * U * (s_num + abs(cb[k]) * s_m0) / abs(m0)
        c0.append(cb)
        b_c0.append(bb)
        for i in range(lo, hi):
            q[i] = [r[i][k] - cb[k] for k in range(3)]
            b_q[i] = [bb[k] + U * (abs(r[i][k]) + abs(cb[k]) + bb[k]) for k in range(3)]   # c0's error + the subtraction's rounding
    return dict(m=m, b_m=b_m, s_m=s_m, c0=c0, b_c0=b_c0, q=q, b_q=b_q)


# ---- the raw moments, exactly -------------------------------------------------------------------------------------------------------------
def _int_array(a):
    """f64 array -> (object array of Python ints, K) with value = int / 2^K exactly."""
    a = np.asarray(a, dtype=np.float64)
    nz = a[a != 0]
    k = 0 if nz.size == 0 else int(53 - np.frexp(np.abs(nz).min())[1]) + 1
    k = max(k, 0)
    scaled = np.ldexp(a, k)
    assert np.isfinite(scaled).all() and np.array_equal(scaled, np.round(scaled))
    out = np.empty(a.shape, dtype=object)
    flat = out.reshape(-1)
    for j, v in enumerate(scaled.reshape(-1).tolist()):
        flat[j] = int(v)
    return out, k


def raw(tbl, pos, vel, first_vert=None):
    """Per body dict(value [26]: Fraction, or float NaN where a non-finite input enters; S [26]: Fractions; n: its particles).
    tbl: the f64 records (REC) the device reads; pos, vel: [nv, 3] f32."""
    tbl = np.asarray(tbl).view(REC).reshape(-1)
    nv = len(tbl)
    first_vert = [0, nv] if first_vert is None else [int(x) for x in first_vert]
    pos, vel = np.asarray(pos, np.float32).reshape(nv, 3), np.asarray(vel, np.float32).reshape(nv, 3)
    out = []
    for b in range(len(first_vert) - 1):
        lo, hi = first_vert[b], first_vert[b + 1]
        x_ok, v_ok = bool(np.isfinite(pos[lo:hi]).all()), bool(np.isfinite(vel[lo:hi]).all())
        m, km = _int_array(tbl["m"][lo:hi])
        q, kq = _int_array(tbl["q"][lo:hi])
        x, kx = _int_array(np.where(np.isfinite(pos[lo:hi]), pos[lo:hi], 0).astype(np.float64))
        v, kv = _int_array(np.where(np.isfinite(vel[lo:hi]), vel[lo:hi], 0).astype(np.float64))
        am, aq, ax, av = np.abs(m), np.abs(q), np.abs(x), np.abs(v)
        val, S = [None] * RAW, [None] * RAW

        def put(at, terms, abs_terms, k, ok):
            S[at] = Fraction(int(abs_terms.sum()) if len(abs_terms) else 0, 2 ** k)
            val[at] = Fraction(int(terms.sum()) if len(terms) else 0, 2 ** k) if ok else float("nan")

        put(MASS, m, am, km, True)
        for a in range(3):
            put(MX + a, m * x[:, a], am * ax[:, a], km + kx, x_ok)
            put(MV + a, m * v[:, a], am * av[:, a], km + kv, v_ok)
            for c in range(3):
                put(A + 3 * a + c, m * x[:, a] * q[:, c], am * ax[:, a] * aq[:, c], km + kx + kq, x_ok)
        for a, (i, j) in enumerate(((1, 2), (2, 0), (0, 1))):
            put(L0 + a, m * (x[:, i] * v[:, j] - x[:, j] * v[:, i]), am * (ax[:, i] * av[:, j] + ax[:, j] * av[:, i]), km + kx + kv, x_ok and v_ok)
        for a, (i, j) in enumerate(((0, 0), (1, 1), (2, 2), (0, 1), (0, 2), (1, 2))):
            put(G + a, m * x[:, i] * x[:, j], am * ax[:, i] * ax[:, j], km + 2 * kx, x_ok)
        qq = q[:, 0] * q[:, 0] + q[:, 1] * q[:, 1] + q[:, 2] * q[:, 2]
        put(Q0, m * qq, am * qq, km + 2 * kq, True)
        out.append(dict(value=val, S=S, n=hi - lo))
    return out


def raw_bounds(o):
    """[26] Fractions: (PATH[k] + the body's particle count) * 2^-53 * S[k] (the count: a generous stand-in for the tree's depth)."""
    return [(PATH[k] + o["n"]) * U * o["S"][k] for k in range(RAW)]


# ---- the derived values, bit for bit --------------------------------------------------------------------------------------------------------
def _rotate(N, V, p, q):
    """One Jacobi rotation of the pair (p, q) on N = {(i, j): [n] for i <= j} with the eigenvectors V[k][j] = [n]; N_pq == 0 skips."""
    key = lambda i, j: (i, j) if i < j else (j, i)
    pp, qq, pq = N[(p, p)], N[(q, q)], N[(p, q)]
    skip = pq == 0.0
    theta = (qq - pp) / (2.0 * pq)
    t = np.where(theta < 0.0, -1.0, 1.0) / (np.abs(theta) + np.sqrt(theta * theta + 1.0))
    c = 1.0 / np.sqrt(t * t + 1.0)
    s = t * c
    tpq = t * pq
    new = {(p, p): pp - tpq, (q, q): qq + tpq, (p, q): np.zeros_like(pq)}
    for r in range(4):
        if r != p and r != q:
            rp, rq = N[key(r, p)], N[key(r, q)]
            new[key(r, p)] = c * rp - s * rq
            new[key(r, q)] = s * rp + c * rq
    for k, v in new.items():
        N[k] = np.where(skip, N[k], v)
    for k in range(4):
        ep, eq = V[k][p], V[k][q]
        V[k][p] = np.where(skip, ep, c * ep - s * eq)
        V[k][q] = np.where(skip, eq, s * ep + c * eq)


def horn_matrix(rows):
    """N of the header as {(i, j): [n]} (i <= j) from rows' A."""
    r = np.asarray(rows, dtype=np.float64).reshape(-1, RAW if np.asarray(rows).shape[-1] == RAW else WIDTH)
    a = lambda i, j: r[:, A + 3 * i + j]
    sxx, syx, szx, sxy, syy, szy, sxz, syz, szz = a(0, 0), a(0, 1), a(0, 2), a(1, 0), a(1, 1), a(1, 2), a(2, 0), a(2, 1), a(2, 2)
    return {(0, 0): (sxx + syy) + szz, (1, 1): (sxx - syy) - szz, (2, 2): (syy - sxx) - szz, (3, 3): (szz - sxx) - syy,
            (0, 1): syz - szy, (0, 2): szx - sxz, (0, 3): sxy - syx, (1, 2): sxy + syx, (1, 3): szx + sxz, (2, 3): syz + szy}


def dense(N):
    """{(i, j): [n]} -> [n, 4, 4] symmetric."""
    n = len(N[(0, 0)])
    M = np.empty((n, 4, 4))
    for (i, j), v in N.items():
        M[:, i, j] = M[:, j, i] = v
    return M


def derived(rows, sweeps=SWEEPS, detail=None):
    """[n, 22] f64 = the values [26..47] of rows whose first 26 values are the raw moments.  detail: a dict that receives lambda_max,
    the norm left off the diagonal and the diagonal, [n] / [n, 4]."""
    rows = np.asarray(rows, dtype=np.float64)
    r = rows.reshape(-1, rows.shape[-1])[:, :RAW]
    n = len(r)
    out = np.zeros((n, WIDTH - RAW))
    at = lambda k: k - RAW
    with np.errstate(all="ignore"):
        mass = r[:, MASS]
        mx, mv = [r[:, MX + a] for a in range(3)], [r[:, MV + a] for a in range(3)]
        com = [mx[a] / mass for a in range(3)]
        for a in range(3):
            out[:, at(COM) + a] = com[a]
            out[:, at(VCOM) + a] = mv[a] / mass
        lx = r[:, L0] - (com[1] * mv[2] - com[2] * mv[1])
        ly = r[:, L0 + 1] - (com[2] * mv[0] - com[0] * mv[2])
        lz = r[:, L0 + 2] - (com[0] * mv[1] - com[1] * mv[0])
        out[:, at(L)], out[:, at(L) + 1], out[:, at(L) + 2] = lx, ly, lz
        gxx, gyy = r[:, G] - (mx[0] * mx[0]) / mass, r[:, G + 1] - (mx[1] * mx[1]) / mass
        gzz, gxy = r[:, G + 2] - (mx[2] * mx[2]) / mass, r[:, G + 3] - (mx[0] * mx[1]) / mass
        gxz, gyz = r[:, G + 4] - (mx[0] * mx[2]) / mass, r[:, G + 5] - (mx[1] * mx[2]) / mass
        tr = (gxx + gyy) + gzz
        ixx, iyy, izz, ixy, ixz, iyz = tr - gxx, tr - gyy, tr - gzz, -gxy, -gxz, -gyz
        a00, a01, a02 = iyy * izz - iyz * iyz, ixz * iyz - ixy * izz, ixy * iyz - ixz * iyy
        a11, a12, a22 = ixx * izz - ixz * ixz, ixy * ixz - ixx * iyz, ixx * iyy - ixy * ixy
        det = (ixx * a00 + ixy * a01) + ixz * a02
        solve = det != 0.0
        out[:, at(OMEGA)] = np.where(solve, ((a00 * lx + a01 * ly) + a02 * lz) / det, 0.0)
        out[:, at(OMEGA) + 1] = np.where(solve, ((a01 * lx + a11 * ly) + a12 * lz) / det, 0.0)
        out[:, at(OMEGA) + 2] = np.where(solve, ((a02 * lx + a12 * ly) + a22 * lz) / det, 0.0)
        N = horn_matrix(r)
        V = [[np.full(n, 1.0 if i == j else 0.0) for j in range(4)] for i in range(4)]
        for _ in range(sweeps):
            for p, q in PAIRS:
                _rotate(N, V, p, q)
        diag = [N[(k, k)] for k in range(4)]
        lam, kmax = diag[0], np.zeros(n, dtype=np.int64)
        for k in (1, 2, 3):
            better = diag[k] > lam
            lam = np.where(better, diag[k], lam)
            kmax = np.where(better, k, kmax)
        w, x, y, z = V[0][0], V[1][0], V[2][0], V[3][0]
        for k in (1, 2, 3):
            pick = kmax == k
            w, x, y, z = np.where(pick, V[0][k], w), np.where(pick, V[1][k], x), np.where(pick, V[2][k], y), np.where(pick, V[3][k], z)
        second = np.where(kmax == 0, diag[1], diag[0])
        for k in (1, 2, 3):
            second = np.where((kmax != k) & (diag[k] > second), diag[k], second)
        ln = np.sqrt(((w * w + x * x) + y * y) + z * z)
        w, x, y, z = w / ln, x / ln, y / ln, z / ln
        first = np.where(x != 0.0, x, np.where(y != 0.0, y, z))
        flip = (w < 0.0) | ((w == 0.0) & (first < 0.0))
        for k, c in enumerate((x, y, z, w)):
            out[:, at(Q) + k] = np.where(flip, -c, c)
        res = ((tr + r[:, Q0]) - 2.0 * lam) / mass
        out[:, at(RESIDUAL)] = np.sqrt(np.where(res < 0.0, 0.0, res))
        out[:, at(GAP)] = lam - second
        if detail is not None:
            detail.update(lam=lam, diag=np.stack(diag, axis=1), off=np.sqrt(2.0 * sum(N[k] ** 2 for k in PAIRS)))
    massless = mass == 0.0
    out[massless] = 0.0
    out[massless, at(Q) + 3] = 1.0
    return out


# ---- what a table gives in plain f64 (the CPU tests' moment sets; NOT the device's summation order) -------------------------------------------
def table_f64(rest, tets, density, first_vert=None):
    """The header's table in numpy f64, operation for operation (the host's own arithmetic: equal to tetsim_prep_pose_table bit for bit)."""
    rest = np.asarray(rest, np.float32).astype(np.float64)
    nv = len(rest)
    first_vert = [0, nv] if first_vert is None else [int(x) for x in first_vert]
    w = (float(density) * observe_v0(rest, tets)) / 4.0
    m = [0.0] * nv
    for ids, we in zip(np.asarray(tets).reshape(-1, 4).tolist(), w.tolist()):
        for i in ids:
            m[i] = m[i] + we
    tbl = np.zeros(nv, dtype=REC)
    tbl["m"] = m
    centres = np.zeros((len(first_vert) - 1, 3))
    for b in range(len(first_vert) - 1):
        lo, hi = first_vert[b], first_vert[b + 1]
        m0, s = 0.0, [0.0, 0.0, 0.0]
        for i in range(lo, hi):
            m0 = m0 + m[i]
            for k in range(3):
                s[k] = s[k] + m[i] * float(rest[i, k])
        if m0 != 0.0:
            centres[b] = [s[k] / m0 for k in range(3)]
        tbl["q"][lo:hi] = rest[lo:hi] - centres[b]
    return tbl, centres


def observe_v0(rest, tets):
    """The observation's V0, [nt] f64 (the expression of strain_ref.rest_volume)."""
    r = np.asarray(rest, dtype=np.float64)
    t = np.asarray(tets).reshape(-1, 4)
    a = r[t[:, 0]]
    e1, e2, e3 = r[t[:, 1]] - a, r[t[:, 2]] - a, r[t[:, 3]] - a
    cx = e2[:, 1] * e3[:, 2] - e2[:, 2] * e3[:, 1]
    cy = e2[:, 2] * e3[:, 0] - e2[:, 0] * e3[:, 2]
    cz = e2[:, 0] * e3[:, 1] - e2[:, 1] * e3[:, 0]
    return ((e1[:, 0] * cx + e1[:, 1] * cy) + e1[:, 2] * cz) / 6.0


def raw_f64(tbl, pos, vel):
    """One body's raw moments [26] in f64 with math.fsum (correctly rounded sums of the rounded terms): the CPU tests' input to derived()."""
    tbl = np.asarray(tbl).view(REC).reshape(-1)
    m, q = tbl["m"], tbl["q"]
    x, v = np.asarray(pos, np.float32).astype(np.float64), np.asarray(vel, np.float32).astype(np.float64)
    cols = [m] + [m * x[:, a] for a in range(3)] + [m * v[:, a] for a in range(3)]
    cols += [(m * x[:, a]) * q[:, c] for a in range(3) for c in range(3)]
    cols += [m * (x[:, i] * v[:, j] - x[:, j] * v[:, i]) for i, j in ((1, 2), (2, 0), (0, 1))]
    cols += [(m * x[:, i]) * x[:, j] for i, j in ((0, 0), (1, 1), (2, 2), (0, 1), (0, 2), (1, 2))]
    cols += [m * ((q[:, 0] * q[:, 0] + q[:, 1] * q[:, 1]) + q[:, 2] * q[:, 2])]
    return np.array([math.fsum(c.tolist()) for c in cols])


# ---- a placed rest body: what the pose row may differ by ----------------------------------------------------------------------------------
def quat_angle(qa, qb):
    """The angle of the rotation between two unit quaternions (xyzw), sign-blind."""
    qa, qb = np.asarray(qa, np.float64), np.asarray(qb, np.float64)
    chord = min(float(np.linalg.norm(qa - qb)), float(np.linalg.norm(qa + qb)))      # (no cancellation for small angles)
    return 4.0 * math.asin(min(1.0, chord / 2.0))


def residual_floor(o, row):
    """What rounding can add to e = ((T + Q0) - 2 lambda_max) / MASS of a row (RESIDUAL^2), as a float: o = raw()'s dict of the body
    (its bounds b), row = the body's 48 values.  T = (Gxx + Gyy) + Gzz - |MX|^2 / MASS is off by at most the G's bounds, 2 |COM_a| times
    MX_a's and COM_a^2 times MASS's; Q0 by its bound; lambda_max by the perturbation of N -- its entries combine at most three of A's, so
    ||dN||_F <= 12 max b(A_ab) -- plus the Jacobi margin d of tests/test_pose_cpu.py; the procedure's own dozen roundings act on values
    no larger than tr G + Q0 + 2 |lambda_max|."""
    b = [float(x) for x in raw_bounds(o)]
    row = np.asarray(row, np.float64)
    mass, com = abs(row[MASS]), np.abs(row[COM:COM + 3])
    e_t = sum(b[G:G + 3]) + sum(2.0 * com[a] * b[MX + a] + com[a] * com[a] * b[MASS] for a in range(3))
    n = dense(horn_matrix(row[None, :RAW]))[0]
    d = (48 * SWEEPS + 16) * float(U) * math.sqrt(float((n * n).sum()))
    e_lam = 12.0 * max(b[A:A + 9]) + d
    own = 16.0 * float(U) * (abs(row[G]) + abs(row[G + 1]) + abs(row[G + 2]) + abs(row[Q0]) + 2.0 * math.sqrt(float((n * n).sum())))
    return (e_t + b[Q0] + 2.0 * e_lam + own) / mass


def placement_bounds(tbl, pos, vel, angular):
    """(angle, omega, vcom, residual_rms) bounds of a body whose stored f32 state is a rigid motion of the table's rest shape with angular
    velocity `angular` (tests/test_pose_cpu.py derives them): delta_i = sqrt(3) * 2^-24 * max |coordinate| of the stored position,
    eps_i = the same of the stored velocity + |angular| * delta_i."""
    tbl = np.asarray(tbl).view(REC).reshape(-1)
    m, q = tbl["m"], tbl["q"]
    x, v = np.asarray(pos, np.float32).astype(np.float64), np.asarray(vel, np.float32).astype(np.float64)
    store = math.sqrt(3.0) * 2.0 ** -24
    delta = store * np.abs(x).max(axis=1)
    eps = store * np.abs(v).max(axis=1) + float(np.linalg.norm(angular)) * delta
    B = np.einsum("i,ia,ib->ab", m, q, q)
    mu = np.linalg.eigvalsh(B)
    M = m.sum()
    com = (m[:, None] * x).sum(axis=0) / M
    d = x - com
    Ic = np.einsum("i,i->", m, (d * d).sum(axis=1)) * np.eye(3) - np.einsum("i,ia,ib->ab", m, d, d)
    angle = 2.0 * float((np.abs(m) * np.linalg.norm(q, axis=1) * delta).sum()) / float(mu[0] + mu[1])
    omega = 2.0 * float((np.abs(m) * np.linalg.norm(d, axis=1) * eps).sum()) / float(np.linalg.eigvalsh(Ic)[0])
    vcom = 2.0 * float((np.abs(m) * eps).sum()) / abs(float(M))
    rms = math.sqrt(float((np.abs(m) * delta * delta).sum()) / abs(float(M)))
    return angle, omega, vcom, rms
