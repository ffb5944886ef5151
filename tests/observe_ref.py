"""The per-body observations of include/tetsim.h (tetsim_observe_bodies_device) in exact arithmetic: plain Python over fractions.Fraction.

Every f32 input becomes the Fraction it is, so the sums, products and quotients below have no rounding error at all.  (The loops over the
tets carry those Fractions as Python integers over one power-of-two denominator, 2^149 per factor -- the same exact arithmetic, with the
gcd taken once at the end instead of in every operation: a Dragon takes a quarter of a second instead of four.)  Next to every sum
and quotient the reference returns S, the sum of the absolute values of all products that enter it once every difference and sum of inputs
is multiplied out: a floating-point evaluation that rounds each operation once, in whatever order it adds, is off by at most
c * 2^-53 * S (to first order), c = the roundings on the longest path from an input to the value + the number of terms added up.
bounds() below counts c for the evaluation the header defines.

What the header defines as bit-exact is computed the way it is defined: the box from the f32 values, max_speed2 in Python floats (IEEE
doubles: (vx*vx + vy*vy) + vz*vz, each operation rounded once), the two counts as integers.

observe(...) returns one dict per body:
    mass, com[3], vcom[3], volume, rest_volume, min_volume_ratio     Fractions (min_volume_ratio: float +inf without a tet of V0 != 0;
                                                                     com / vcom / volume: float NaN where a non-finite input enters)
    inverted_tets, nonfinite                                         ints
    aabb_min[3], aabb_max[3], max_speed2                             floats
    S                                                                {name: S of that value} (com / vcom: a list of 3)
    tets, min_abs_ratio                                              the body's tet count; min |V/V0| over its tets (how far every sign is
                                                                     from flipping)
"""
import math
from fractions import Fraction

import numpy as np

INF = float("inf")
U = Fraction(1, 2 ** 53)

# roundings on the longest path into one tet's term (include/tetsim.h, DEFINITIONS)
R_VOLUME = 7        # x_k - x_0 | a product of the cross | its difference | a product of the dot | its two sums | / 6
R_W = R_VOLUME + 2  # density * V0 | / 4
R_MOMENT = R_W + 4  # three sums of the corners | w * (...)


SCALE = 2 ** 149   # every finite f32 is an integer multiple of 2^-149


def _ints(a):
    """[n, 3] float32 -> per row three Python integers m with value = m / SCALE (exact: the product is exact in f64), or None for a row
    with a non-finite component.  The hot loops below work on these integers -- numerators over a common power-of-two denominator -- and
    every value leaves as the Fraction it is; the arithmetic is Fraction arithmetic with the gcd taken once at the end."""
    rows = (np.asarray(a, dtype=np.float32).astype(np.float64) * 2.0 ** 149).tolist()
    return [[int(c) for c in r] if all(math.isfinite(c) for c in r) else None for r in rows]


def _det_and_s(p0, p1, p2, p3):
    """(6 * SCALE^3 * dot(p1-p0, cross(p2-p0, p3-p0)) / 6, the same multiple of that expression's S): corners as 3 integers each."""
    e = [[p[k] - p0[k] for k in range(3)] for p in (p1, p2, p3)]
    a = [[abs(p[k]) + abs(p0[k]) for k in range(3)] for p in (p1, p2, p3)]
    det = s = 0
    for (i, j, k), sign in (((0, 1, 2), 1), ((1, 2, 0), 1), ((2, 0, 1), 1), ((0, 2, 1), -1), ((2, 1, 0), -1), ((1, 0, 2), -1)):
        det += sign * e[0][i] * e[1][j] * e[2][k]
        s += a[0][i] * a[1][j] * a[2][k]
    return det, s


def observe(rest, tets, pos, vel, density, first_vert=None, first_tet=None):
    """rest / pos / vel: [nv, 3] float32 arrays (a batch: the concatenation); tets: [nt, 4] ids into them; first_vert / first_tet:
    [bodies + 1] ranges of a batch, or None for one body."""
    nv, nt = len(rest), len(tets)
    first_vert = [0, nv] if first_vert is None else [int(x) for x in first_vert]
    first_tet = [0, nt] if first_tet is None else [int(x) for x in first_tet]
    rho = Fraction(float(density))
    R, X, Vl = _ints(rest), _ints(pos), _ints(vel)
    ok_p, ok_v = [x is not None for x in X], [x is not None for x in Vl]
    tet_ids = np.asarray(tets).reshape(-1, 4).tolist()
    vol_unit = Fraction(1, 6 * SCALE ** 3)             # a determinant's integer -> a volume
    w_unit = abs(rho) * vol_unit / 4                   # a rest determinant's integer -> w (its sign is the determinant's)
    out = []
    for b in range(len(first_vert) - 1):
        d0_sum = s0_sum = d_sum = s_sum = 0            # sums of determinants and of their S, rest and current
        mom, s_mom = [[0] * 3, [0] * 3], [[0] * 3, [0] * 3]   # [positions, velocities][xyz]: sums of rest determinant * corner sum
        nan_x = nan_v = False
        min_ratio, s_ratio, min_abs, inverted = INF, Fraction(0), INF, 0
        for e in range(first_tet[b], first_tet[b + 1]):
            ids = tet_ids[e]
            d0, s0 = _det_and_s(*(R[i] for i in ids))
            d0_sum += d0
            s0_sum += s0
            for which, A in enumerate((X, Vl)):
                if any(A[i] is None for i in ids):
                    if which == 0:
                        nan_x = True
                    else:
                        nan_v = True
                    continue
                for k in range(3):
                    mom[which][k] += d0 * sum(A[i][k] for i in ids)
                    s_mom[which][k] += s0 * sum(abs(A[i][k]) for i in ids)
            if any(X[i] is None for i in ids):
                continue                                   # (a NaN volume: left out of the minimum and of the count; nan_x is set)
            d, s = _det_and_s(*(X[i] for i in ids))
            d_sum += d
            s_sum += s
            if d0 != 0:
                r = Fraction(d, d0)
                s_r = (s + abs(r) * s0) / abs(d0)          # V / V0 off by a in V and b in V0: a / V0 - (V / V0) * b / V0
                if r < min_ratio:
                    min_ratio = r
                s_ratio = max(s_ratio, s_r)
                min_abs = min(min_abs, abs(r))
                inverted += r <= 0
        sign = -1 if rho < 0 else 1
        mass, s_mass = 4 * sign * w_unit * d0_sum, 4 * w_unit * s0_sum
        rest_volume, s_rest, volume, s_volume = vol_unit * d0_sum, vol_unit * s0_sum, vol_unit * d_sum, vol_unit * s_sum
        mom = [[sign * w_unit * m / SCALE for m in row] for row in mom]
        s_mom = [[w_unit * m / SCALE for m in row] for row in s_mom]
        o = dict(tets=first_tet[b + 1] - first_tet[b], mass=mass, rest_volume=rest_volume, min_volume_ratio=min_ratio, inverted_tets=int(inverted),
                 volume=float("nan") if nan_x else volume, min_abs_ratio=min_abs)
        S = dict(mass=s_mass, rest_volume=s_rest, volume=s_volume, min_volume_ratio=s_ratio)
        for which, name, nan in ((0, "com", nan_x), (1, "vcom", nan_v)):
            if mass == 0:
                o[name], S[name] = [Fraction(0)] * 3, [Fraction(0)] * 3
            elif nan:
                o[name], S[name] = [float("nan")] * 3, [Fraction(0)] * 3
            else:
                o[name] = [mom[which][k] / mass for k in range(3)]
                # N / M off by a in N and b in M: a / M - (N / M) * b / M, and the quotient's own rounding (|q| <= |q| S_M / |M|)
                S[name] = [(s_mom[which][k] + abs(o[name][k]) * s_mass) / abs(mass) for k in range(3)]
        lo, hi, speed2, nonfinite = [INF] * 3, [-INF] * 3, 0.0, 0
        for i in range(first_vert[b], first_vert[b + 1]):
            if not (ok_p[i] and ok_v[i]):
                nonfinite += 1
                continue
            x, u = [float(c) for c in pos[i]], [float(c) for c in vel[i]]
            lo, hi = [min(a, c) for a, c in zip(lo, x)], [max(a, c) for a, c in zip(hi, x)]
            speed2 = max(speed2, (u[0] * u[0] + u[1] * u[1]) + u[2] * u[2])
        o.update(aabb_min=lo, aabb_max=hi, max_speed2=speed2, nonfinite=nonfinite, S=S)
        out.append(o)
    return out


def bounds(o):
    """{name: the largest |computed - exact| the header's evaluation allows} for the sums and quotients of one body's dict (com / vcom: a
    list of 3), as Fractions: c * 2^-53 * S with
        mass         c = R_W + tets                     volume, rest_volume   c = R_VOLUME + tets
        com, vcom    c = R_MOMENT + tets + 2            (the numerator's path is the longer one; + the division's rounding; + 1 that covers
                                                        the second-order terms, which are c * 2^-53 * S_mass / |mass| of the bound: tiny)
        min_volume_ratio   c = R_VOLUME + 2             (V and V0 have the same path; + the division; + 1 as above; nothing is added up, and
                                                        the minimum of values that are each within the bound is within the largest bound)"""
    n, S = o["tets"], o["S"]
    c = dict(mass=R_W + n, volume=R_VOLUME + n, rest_volume=R_VOLUME + n, min_volume_ratio=R_VOLUME + 2, com=R_MOMENT + n + 2, vcom=R_MOMENT + n + 2)
    return {k: [c[k] * U * s for s in S[k]] if isinstance(S[k], list) else c[k] * U * S[k] for k in c}
