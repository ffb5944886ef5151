"""What the touch rows cost next to an observation row, on the same handle: 64 Dragons in one batch, with 0, 4 and 8 collider slots per
body (the body-collider table; 0 = never switched on).  Each figure: device time between two events on torch's stream around 20 calls
enqueued back to back, per call, median of 9 such measurements after 3 warm-up rounds.  Polar FAST.  The numbers to read are the ratios
to the observation.

    python tools/touch_cost.py [--bodies 64] [--out profiles/touch_cost.txt]
"""
import argparse
import os
import sys

import numpy as np
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tools"))

from pose_cost import CALLS, DT, PP, ROUNDS, dragon, per_call_us  # noqa: E402
from tetsim_amd import SoftBodyHIP  # noqa: E402

MARGIN = 1e-3


def slots(v, count):
    """`count` colliders around a Dragon with vertices v: the floor it rests on, then spheres, boxes and capsules along its sides"""
    lo, hi = v.min(axis=0).astype(float), v.max(axis=0).astype(float)
    c, s = (lo + hi) / 2, hi - lo
    every = [dict(kind="plane", a=(0.0, lo[1] + 0.02 * s[1], 0.0), b=(0.0, 1.0, 0.0), friction=0.3),
             dict(kind="sphere", a=(hi[0], c[1], c[2]), radius=0.25 * s[0]),
             dict(kind="box", a=(lo[0], c[1], c[2]), b=tuple(0.2 * s)),
             dict(kind="capsule", a=(lo[0], hi[1], c[2]), b=(hi[0], hi[1], c[2]), radius=0.05 * s[1]),
             dict(kind="sphere", a=(c[0], c[1], hi[2]), radius=0.2 * s[2]),
             dict(kind="box", a=(c[0], c[1], lo[2]), b=tuple(0.15 * s)),
             dict(kind="capsule", a=(c[0], lo[1], lo[2]), b=(c[0], lo[1], hi[2]), radius=0.05 * s[1]),
             dict(kind="plane", a=(lo[0] + 0.02 * s[0], 0.0, 0.0), b=(1.0, 0.0, 0.0))]
    return every[:count]


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--bodies", type=int, default=64)
    ap.add_argument("--out", default=None)
    a = ap.parse_args()
    v, t = dragon(0.3)
    lines = []
    for count in (0, 4, 8):
        body = SoftBodyHIP.batch([(v, t)] * a.bodies, dict(PP), solver="polar", precision="fast")
        if count:
            body.setBodyColliders([slots(v, count)] * a.bodies)
        body.simulateSubsteps(20, DT, PP)
        body.observeBodies()   # (the first calls build and upload the tables)
        body.touchBodies(MARGIN)
        body.touchParticlesDevice(MARGIN)
        torch.cuda.synchronize()
        obs = per_call_us(body.observeBodies)
        rows = per_call_us(lambda: body.touchBodies(MARGIN))
        prt = per_call_us(lambda: body.touchParticlesDevice(MARGIN))
        touching = body.bodyTouch(MARGIN)[:, 0]
        lines.append("%d Dragons, %d slots per body, %d particles (%d touching in body 0): observation %.2f us, touch rows %.2f us (x%.2f), "
                     "particle rows %.2f us (x%.2f) per call" % (a.bodies, count, body.info.num_particles, touching[0], obs, rows, rows / obs, prt, prt / obs))
        body.close()
    lines.append("(polar FAST, margin %g; device us per call: %d calls between two events, median of %d)" % (MARGIN, CALLS, ROUNDS))
    text = "\n".join(lines)
    print(text)
    if a.out:
        with open(a.out, "w") as f:
            f.write(text + "\n")


if __name__ == "__main__":
    main()
