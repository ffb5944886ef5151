"""The per-tet strain of include/tetsim.h (tetsim_tet_strain_device / tetsim_body_strain_device) in numpy, operation for operation.

Everything is f64 arithmetic on the stored f32 values, every operation rounded on its own (numpy evaluates a * b + c as two ufuncs: no
fused multiply-add), sums left to right as the header writes them, and only + - * / sqrt, which IEEE 754 rounds correctly on the host and
on the device alike: the device's rows equal these BIT FOR BIT.

    tet_values(pos, tets, irp)            [nt, 15] f64: F (9, column-major), J, DEV, STRETCH (3, descending), GREEN
    tet_rows(values, degenerate)          [nt, 16] f32: the values rounded once, degenerate tets NaN in 0..14, RESERVED 0
    degenerate_tets(rest, tets, irp)      [nt] bool: rest volume 0 (the observation's V0) or a non-finite invRestPose entry
    body_rows(values, rows, v0, degenerate, first_tet)    [bodies, 8] f64: the reduction tree of the header

SWEEPS is the fixed number of cyclic Jacobi sweeps; tests/test_strain_cpu.py says why it is what it is."""
import numpy as np

SWEEPS = 4
CHUNK = 256
WIDTH, BODY_WIDTH = 16, 8
F_AT, J_AT, DEV_AT, STRETCH_AT, GREEN_AT, RESERVED_AT = 0, 9, 10, 11, 14, 15
INF = np.inf


def rest_volume(rest, tets):
    """The observation's V0 = dot(r1-r0, cross(r2-r0, r3-r0)) / 6 with its sign, [nt] f64 (include/tetsim.h, per-body observations)."""
    r = np.asarray(rest, dtype=np.float32).astype(np.float64)
    t = np.asarray(tets).reshape(-1, 4)
    a = r[t[:, 0]]
    e1, e2, e3 = r[t[:, 1]] - a, r[t[:, 2]] - a, r[t[:, 3]] - a
    cx = e2[:, 1] * e3[:, 2] - e2[:, 2] * e3[:, 1]
    cy = e2[:, 2] * e3[:, 0] - e2[:, 0] * e3[:, 2]
    cz = e2[:, 0] * e3[:, 1] - e2[:, 1] * e3[:, 0]
    return ((e1[:, 0] * cx + e1[:, 1] * cy) + e1[:, 2] * cz) / 6.0


def degenerate_tets(rest, tets, irp):
    irp = np.asarray(irp, dtype=np.float32).reshape(-1, 9)
    return (rest_volume(rest, tets) == 0.0) | ~np.isfinite(irp).all(axis=1)


def deformation_gradient(pos, tets, irp):
    """F = P * invRestPose per tet, [nt, 9] f64 column-major (F[:, 3 * j + i] = F_ij)."""
    x = np.asarray(pos, dtype=np.float32).astype(np.float64)
    t = np.asarray(tets).reshape(-1, 4)
    B = np.asarray(irp, dtype=np.float32).astype(np.float64).reshape(-1, 9)
    P = [x[t[:, k + 1]] - x[t[:, 0]] for k in range(3)]            # P[k][:, i] = P_ik
    F = np.empty((len(t), 9))
    for j in range(3):
        for i in range(3):
            F[:, 3 * j + i] = (P[0][:, i] * B[:, 3 * j] + P[1][:, i] * B[:, 3 * j + 1]) + P[2][:, i] * B[:, 3 * j + 2]
    return F


def _rotate(C, p, q, r):
    """One Jacobi rotation of the pair (p, q), r the third index, on C = {(i, j): [n] f64 for i <= j}.  A pair whose C_pq is 0 is left
    as it is; a NaN C_pq is not 0, so the rotation runs and the NaN spreads."""
    key = lambda i, j: (i, j) if i < j else (j, i)
    pp, qq, pq, rp, rq = C[(p, p)], C[(q, q)], C[key(p, q)], C[key(r, p)], C[key(r, q)]
    skip = pq == 0.0
    theta = (qq - pp) / (2.0 * pq)
    t = np.where(theta < 0.0, -1.0, 1.0) / (np.abs(theta) + np.sqrt(theta * theta + 1.0))
    c = 1.0 / np.sqrt(t * t + 1.0)
    s = t * c
    tpq = t * pq
    new = {(p, p): pp - tpq, (q, q): qq + tpq, key(p, q): np.zeros_like(pq), key(r, p): c * rp - s * rq, key(r, q): s * rp + c * rq}
    for k, v in new.items():
        C[k] = np.where(skip, C[k], v)


def values_from_F(F, sweeps=SWEEPS, off=None):
    """[n, 15] f64 of [n, 9] column-major F.  off: a list that receives the off-diagonal Frobenius norm Jacobi left behind, [n]."""
    F = np.asarray(F, dtype=np.float64).reshape(-1, 9)
    f = lambda i, j: F[:, 3 * j + i]
    out = np.empty((len(F), 15))
    out[:, :9] = F
    with np.errstate(all="ignore"):
        out[:, J_AT] = (f(0, 0) * (f(1, 1) * f(2, 2) - f(1, 2) * f(2, 1)) - f(0, 1) * (f(1, 0) * f(2, 2) - f(1, 2) * f(2, 0))) \
            + f(0, 2) * (f(1, 0) * f(2, 1) - f(1, 1) * f(2, 0))
        C = {(i, j): (f(0, i) * f(0, j) + f(1, i) * f(1, j)) + f(2, i) * f(2, j) for i in range(3) for j in range(i, 3)}
        out[:, DEV_AT] = np.sqrt((C[(0, 0)] + C[(1, 1)]) + C[(2, 2)])
        e = [(C[(i, i)] - 1.0) / 2.0 for i in range(3)] + [C[k] / 2.0 for k in ((0, 1), (0, 2), (1, 2))]
        g = e[0] * e[0]
        g = g + e[1] * e[1]
        g = g + e[2] * e[2]
        for k in (3, 4, 5):
            g = g + 2.0 * (e[k] * e[k])
        out[:, GREEN_AT] = np.sqrt(g)
        for _ in range(sweeps):
            _rotate(C, 0, 1, 2)
            _rotate(C, 0, 2, 1)
            _rotate(C, 1, 2, 0)
        if off is not None:
            off.append(np.sqrt(2.0 * (C[(0, 1)] ** 2 + C[(0, 2)] ** 2 + C[(1, 2)] ** 2)))
        s = [np.sqrt(np.where(C[(i, i)] < 0.0, 0.0, C[(i, i)])) for i in range(3)]
        for a, b in ((0, 1), (0, 2), (1, 2)):                        # descending: swap where the earlier one is smaller (a NaN stays)
            swap = s[a] < s[b]
            s[a], s[b] = np.where(swap, s[b], s[a]), np.where(swap, s[a], s[b])
        for k in range(3):
            out[:, STRETCH_AT + k] = s[k]
    return out


def tet_values(pos, tets, irp, sweeps=SWEEPS):
    with np.errstate(all="ignore"):
        F = deformation_gradient(pos, tets, irp)
    return values_from_F(F, sweeps)


def tet_rows(values, degenerate=None):
    rows = np.zeros((len(values), WIDTH), dtype=np.float32)
    with np.errstate(all="ignore"):
        rows[:, :15] = values.astype(np.float32)
    if degenerate is not None:
        rows[np.asarray(degenerate, dtype=bool), :15] = np.nan
    return rows


# ---- the body row -------------------------------------------------------------------------------------------------------------------
_OPS = (np.fmax, np.fmin, np.fmin, np.fmax, np.fmax, np.add, np.add, np.add)
_IDENTITY = (-INF, INF, INF, -INF, -INF, 0.0, 0.0, 0.0)


def _tree256(v):
    """[256, 8] -> [8]: within a wave of 64 lane l takes lane l + 32, 16, .. 1; the four waves as (w0 + w1) + (w2 + w3)."""
    w = v.reshape(4, 64, BODY_WIDTH)
    h = 32
    while h:
        w = np.stack([_OPS[k](w[:, :h, k], w[:, h:2 * h, k]) for k in range(BODY_WIDTH)], axis=-1)
        h //= 2
    w = w[:, 0, :]
    return np.array([_OPS[k](_OPS[k](w[0, k], w[1, k]), _OPS[k](w[2, k], w[3, k])) for k in range(BODY_WIDTH)])


def body_rows(values, rows, v0, degenerate, first_tet=None):
    """values: tet_values; rows: tet_rows of them (a tet whose f32 row is not finite in 0..14 is left out); v0: rest_volume;
    first_tet: [bodies + 1] of a batch, or None for one body."""
    nt = len(values)
    first_tet = [0, nt] if first_tet is None else [int(x) for x in first_tet]
    out_of = np.asarray(degenerate, dtype=bool) | ~np.isfinite(rows[:, :15]).all(axis=1)
    g = values[:, GREEN_AT]
    a = np.abs(np.asarray(v0, dtype=np.float64))
    per = np.stack([values[:, STRETCH_AT], values[:, STRETCH_AT + 2], values[:, J_AT], values[:, J_AT], g, a * (g * g), a,
                    np.zeros(nt)], axis=1)
    per[out_of] = _IDENTITY
    per[:, 7] = out_of
    ident = np.array(_IDENTITY)
    res = np.empty((len(first_tet) - 1, BODY_WIDTH))
    for b in range(len(first_tet) - 1):
        lo, hi = first_tet[b], first_tet[b + 1]
        partial = []
        for at in range(lo, hi, CHUNK):
            block = np.tile(ident, (CHUNK, 1))
            n = min(CHUNK, hi - at)
            block[:n] = per[at:at + n]
            partial.append(_tree256(block))
        lanes = np.tile(ident, (CHUNK, 1))
        for j, p in enumerate(partial):                              # thread t folds the partial rows t, t + 256, .. in that order
            lanes[j % CHUNK] = [_OPS[k](lanes[j % CHUNK, k], p[k]) for k in range(BODY_WIDTH)]
        res[b] = _tree256(lanes)
    return res
