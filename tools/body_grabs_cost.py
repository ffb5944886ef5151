"""What body grabs cost when they are ON: 64 Dragons in one batch, one call of 20 substeps (timeSubsteps), every body held against
none held -- median of 20 calls after 5 warm-up calls, polar FAST and Neo-Hookean FAST.  Prints one line per solver and the ratio.

    python tools/body_grabs_cost.py [--bodies 64] [--out profiles/body_grabs_cost.txt]
"""
import argparse
import os
import statistics
import sys

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

from tetsim_amd import SoftBodyHIP  # noqa: E402

PP = dict(gravity=-9.81, friction=1000.0, density=1000.0, devCompliance=1e-5, volCompliance=0.0,
          worldBounds=[-2.5, -1.0, -2.5, 2.5, 10.0, 2.5])
DT = (1.0 / 60.0) / 20
SUB, WARM, CALLS = 20, 5, 20


def dragon(y0):
    gold = os.path.join(ROOT, "tests", "golden")
    v = np.fromfile(os.path.join(gold, "dragon_verts.f32"), dtype="<f4").reshape(-1, 3).copy()
    t = np.fromfile(os.path.join(gold, "dragon_tets.i32"), dtype="<i4").reshape(-1, 4)
    v[:, 1] += np.float32(y0) - v[:, 1].min()
    return v, t


def median_ms(body):
    for _ in range(WARM):
        body.timeSubsteps(SUB, DT, PP)
    return statistics.median(body.timeSubsteps(SUB, DT, PP) for _ in range(CALLS))


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--bodies", type=int, default=64)
    ap.add_argument("--out", default=None)
    a = ap.parse_args()
    meshes = [dragon(0.3)] * a.bodies
    lines = []
    for name, kw in (("polar FAST", dict(solver="polar", precision="fast")), ("Neo-Hookean FAST", dict(solver="neohookean", precision="fast"))):
        free, held = (SoftBodyHIP.batch(meshes, dict(PP), **kw) for _ in range(2))
        v = meshes[0][0]
        held.setBodyGrabs(np.full(a.bodies, 5, np.int32), np.tile(v[5] - np.float32([0.0, 0.15, 0.0]), (a.bodies, 1)))
        off, on = median_ms(free), median_ms(held)
        lines.append("%-17s %d Dragons, path %d, %d substeps per call, median of %d calls: none held %.4f ms, every body held %.4f ms, ratio %.4f"
                     % (name, a.bodies, held.info.fused_particle_pass, SUB, CALLS, off, on, on / off))
        free.close()
        held.close()
    text = "\n".join(lines)
    print(text)
    if a.out:
        with open(a.out, "w") as f:
            f.write(text + "\n")


if __name__ == "__main__":
    main()
