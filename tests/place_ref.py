"""The definition of tetsim_place_bodies / _device (include/tetsim.h, "placement") in numpy: f64 on the stored f32 values, every operation
rounded on its own and written in the header's order (numpy never fuses a multiply with an add), results rounded once to f32.  One row =
one body's rigid motion; the functions take that body's rows of the state.  No GPU, no library: tests/test_place_cpu.py checks its
properties, tests/test_gpu_place.py holds the device kernel to it value for value."""
import numpy as np

Q, PIVOT, OFFSET, LINEAR, ANGULAR, WIDTH = 0, 4, 7, 10, 13, 16


def row_ok(row):
    """What the device kernel asks of a row before it touches the body: every float finite, |q| != 0."""
    r = np.asarray(row, dtype=np.float32).astype(np.float64)
    return bool(np.isfinite(r).all()) and _norm(r[Q:Q + 4]) != 0.0


def _norm(q):
    return np.sqrt(((q[0] * q[0] + q[1] * q[1]) + q[2] * q[2]) + q[3] * q[3])


class Motion:
    """Unit quaternion, matrix, pivot, centre, linear and angular velocity of one row, all f64."""

    def __init__(self, row):
        r = np.asarray(row, dtype=np.float32).reshape(WIDTH).astype(np.float64)
        n = _norm(r[Q:Q + 4])
        x, y, z, w = r[Q] / n, r[Q + 1] / n, r[Q + 2] / n, r[Q + 3] / n
        xx, yy, zz, xy, xz, yz, wx, wy, wz = x * x, y * y, z * z, x * y, x * z, y * z, w * x, w * y, w * z
        self.q = np.array([x, y, z, w])
        self.m = np.array([[1.0 - 2.0 * (yy + zz), 2.0 * (xy - wz), 2.0 * (xz + wy)],
                           [2.0 * (xy + wz), 1.0 - 2.0 * (xx + zz), 2.0 * (yz - wx)],
                           [2.0 * (xz - wy), 2.0 * (yz + wx), 1.0 - 2.0 * (xx + yy)]])
        self.pivot = r[PIVOT:PIVOT + 3]
        self.centre = r[PIVOT:PIVOT + 3] + r[OFFSET:OFFSET + 3]
        self.linear, self.angular = r[LINEAR:LINEAR + 3], r[ANGULAR:ANGULAR + 3]

    def rot(self, d):
        """Rot(d)_i = (m_i0*d.x + m_i1*d.y) + m_i2*d.z for rows d [n, 3] (f64)."""
        m = self.m
        return np.stack([(m[i, 0] * d[:, 0] + m[i, 1] * d[:, 1]) + m[i, 2] * d[:, 2] for i in range(3)], axis=1)


def _f64(a, cols):
    return np.asarray(a, dtype=np.float32).reshape(-1, cols).astype(np.float64)


def place_points(row, p):
    """World-space points (positions, Neo-Hookean previous positions, corners of an absolute shape layout): f32(Rot(p - pivot) + c)."""
    M = Motion(row)
    return (M.rot(_f64(p, 3) - M.pivot) + M.centre).astype(np.float32)


def place_particles(row, pos, vel, keep_velocity=False):
    """(pos', vel') [n, 3] f32."""
    M = Motion(row)
    r = M.rot(_f64(pos, 3) - M.pivot)
    a = M.angular
    cross = np.stack([a[1] * r[:, 2] - a[2] * r[:, 1], a[2] * r[:, 0] - a[0] * r[:, 2], a[0] * r[:, 1] - a[1] * r[:, 0]], axis=1)
    u = M.linear + cross
    if keep_velocity:
        u = M.rot(_f64(vel, 3)) + u
    return (r + M.centre).astype(np.float32), u.astype(np.float32)


def place_quats(row, quats):
    """q' = f32(qR (x) q) [n, 4] xyzw, in the reference's quat_mult term order (SoftbodyGPU.js:114-121); not renormalised."""
    ax, ay, az, aw = Motion(row).q
    b = _f64(quats, 4)
    bx, by, bz, bw = b[:, 0], b[:, 1], b[:, 2], b[:, 3]
    return np.stack([((aw * bx + ax * bw) + ay * bz) - az * by, ((aw * by - ax * bz) + ay * bw) + az * bx,
                     ((aw * bz + ax * by) - ay * bx) + az * bw, ((aw * bw - ax * bx) - ay * by) - az * bz], axis=1).astype(np.float32)


def place_shape_absolute(row, corners):
    """Corners [..., 3] of a layout that stores world-space corners (the reference's textureElem): f32(Rot(e - pivot) + c)."""
    c = np.asarray(corners, dtype=np.float32)
    return place_points(row, c.reshape(-1, 3)).reshape(c.shape)


def place_shape_centred(row, corners):
    """Corners [..., 3] of a layout that stores corners relative to their own centroid: f32(Rot(e))."""
    c = np.asarray(corners, dtype=np.float32)
    return Motion(row).rot(_f64(c, 3)).astype(np.float32).reshape(c.shape)


def predict(pos, vel, dt):
    """The re-prediction kernel's arithmetic on the placed rows: f32 product, then f32 sum."""
    p, v = np.asarray(pos, dtype=np.float32), np.asarray(vel, dtype=np.float32)
    return p + v * np.float32(dt)
