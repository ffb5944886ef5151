"""What a pose row costs next to an observation row, on the same handles: 64 Dragons in one batch, and the 1 M-tet lattice (one body).
Each figure: device time between two events on torch's stream around 20 calls enqueued back to back, per call, median of 9 such
measurements after 3 warm-up rounds.  Polar FAST and Neo-Hookean FAST.  The number to read is the ratio pose / observation.

    python tools/pose_cost.py [--bodies 64] [--cells 55] [--out profiles/pose_cost.txt]
"""
import argparse
import os
import statistics
import sys

import numpy as np
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

from tetsim_amd import SoftBodyHIP, make_lattice  # noqa: E402

PP = dict(gravity=-9.81, friction=1000.0, density=1000.0, devCompliance=1e-5, volCompliance=0.0,
          worldBounds=[-2.5, -1.0, -2.5, 2.5, 10.0, 2.5])
DT = (1.0 / 60.0) / 20
CALLS, WARM, ROUNDS = 20, 3, 9


def dragon(y0):
    gold = os.path.join(ROOT, "tests", "golden")
    v = np.fromfile(os.path.join(gold, "dragon_verts.f32"), dtype="<f4").reshape(-1, 3).copy()
    t = np.fromfile(os.path.join(gold, "dragon_tets.i32"), dtype="<i4").reshape(-1, 4)
    v[:, 1] += np.float32(y0) - v[:, 1].min()
    return v, t


def per_call_us(fn):
    """Device microseconds per call of fn, CALLS calls between two events, median of ROUNDS."""
    got = []
    for r in range(WARM + ROUNDS):
        e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        e0.record()
        for _ in range(CALLS):
            fn()
        e1.record()
        e1.synchronize()
        if r >= WARM:
            got.append(1000.0 * e0.elapsed_time(e1) / CALLS)
    return statistics.median(got)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--bodies", type=int, default=64)
    ap.add_argument("--cells", type=int, default=55)
    ap.add_argument("--out", default=None)
    a = ap.parse_args()
    lines = []
    for name, kw in (("polar FAST", dict(solver="polar", precision="fast")), ("Neo-Hookean FAST", dict(solver="neohookean", precision="fast", order="clustered"))):
        for what, make in (("%d Dragons" % a.bodies, lambda: SoftBodyHIP.batch([dragon(0.3)] * a.bodies, dict(PP), **kw)),
                           ("lattice of %d cells" % a.cells, lambda: SoftBodyHIP(*make_lattice(a.cells), None, dict(PP), **kw))):
            body = make()
            body.simulateSubsteps(20, DT, PP)
            body.observeBodies()   # (the first calls build and upload the tables)
            body.observePoses()
            torch.cuda.synchronize()
            obs, pose = per_call_us(body.observeBodies), per_call_us(body.observePoses)
            lines.append("%-17s %-22s %8d particles %8d tets: observation %.2f us, pose %.2f us per call, pose / observation %.2f"
                         % (name, what, body.info.num_particles, body.info.num_elems, obs, pose, pose / obs))
            body.close()
    lines.append("(device us per call: %d calls between two events, median of %d)" % (CALLS, ROUNDS))
    text = "\n".join(lines)
    print(text)
    if a.out:
        with open(a.out, "w") as f:
            f.write(text + "\n")


if __name__ == "__main__":
    main()
