"""What kinematic colliders (tetsim_set_colliders) cost: tetsim_time_step_n per frame with 0, 1 and 8 colliders, on the 1 M-tet lattice
(FAST, the benchmark's body) and on the Dragon frame (FAST: the four-lane frame kernel; PRECISE).  The colliders sit in the body's fall
path so that the contact branch is taken by some particles, as in use.
    python tools/collider_cost.py [--reps 10]"""
import argparse
import os
import sys

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import numpy as np  # noqa: E402

from tetsim_amd import SoftBodyHIP, make_lattice  # noqa: E402

PP = dict(gravity=-9.81, friction=1000.0, density=1000.0, devCompliance=1e-5, volCompliance=0.0, worldBounds=[-2.5, -1.0, -2.5, 2.5, 10.0, 2.5])
G = os.path.join(os.path.dirname(os.path.dirname(os.path.abspath(__file__))), "tests", "golden")


def colliders(v, k):
    lo, hi = v.min(0).astype(float), v.max(0).astype(float)
    c, w = (lo + hi) / 2, hi - lo
    y = lo[1] + 0.05 * w[1]   # through the body's lowest twentieth: particles in contact every substep
    pool = [dict(kind="sphere", a=[c[0], y - 0.2 * w[0], c[2]], radius=0.2 * w[0] + 0.01, friction=100.0),
            dict(kind="plane", a=[0, y - 0.03 * w[1], 0], b=[0.1, 1.0, 0.0], friction=10.0),
            dict(kind="capsule", a=[lo[0], y, c[2]], b=[hi[0], y, c[2]], radius=0.02 * w[0], friction=10.0),
            dict(kind="box", a=[c[0], y - 0.05 * w[1], c[2]], b=[0.3 * w[0], 0.05 * w[1], 0.3 * w[2]], friction=10.0)]
    return [pool[i % 4] for i in range(k)]


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--reps", type=int, default=10)
    ap.add_argument("--cells", type=int, default=55)   # 55^3 * 6 = 998,250 tets
    a = ap.parse_args()
    dv = np.fromfile(os.path.join(G, "dragon_verts.f32"), dtype="<f4").reshape(-1, 3)
    dt_ = np.fromfile(os.path.join(G, "dragon_tets.i32"), dtype="<i4").reshape(-1, 4)
    lv, lt = make_lattice(a.cells, y0=0.02)
    cases = [("lattice %d tets fast" % len(lt), lv, lt, dict(solver="polar", precision="fast")),
             ("dragon fast", dv, dt_, dict(solver="polar", precision="fast")),
             ("dragon precise", dv, dt_, dict(solver="polar", precision="precise")),
             ("dragon neohookean fast", dv, dt_, dict(solver="neohookean", precision="fast"))]
    n, dt = 20, (1.0 / 60.0) / 20
    for name, v, t, kw in cases:
        res = {}
        for k in (0, 1, 8):
            b = SoftBodyHIP(v, t, None, dict(PP), **kw)
            if k:
                b.setColliders(colliders(v, k))
            b.simulateSubsteps(n, dt, PP)
            b.sync()
            ms = sorted(b.timeSubsteps(n, dt, PP) for _ in range(a.reps))
            res[k] = ms[len(ms) // 2]
            path = b.info.fused_particle_pass
            b.close()
        print("%-34s path %d  ms per call of %d substeps (median of %d): 0 colliders %.4f  1: %.4f (%+.1f%%)  8: %.4f (%+.1f%%)" % (
            name, path, n, a.reps, res[0], res[1], 100 * (res[1] / res[0] - 1), res[8], 100 * (res[8] / res[0] - 1)), flush=True)


if __name__ == "__main__":
    main()
