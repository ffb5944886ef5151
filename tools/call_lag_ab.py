#!/usr/bin/env python3
"""In-run A/B of the one-launch polar call's dispatch order on the 1 M-tet lattice (polar Jacobi FAST): TETSIM_PJ_CALL_LAG = how many tile
blocks per XCD a particle block sits behind the last tile it waits for (0 = behind every tile of the substep; host_prep.cpp:
build_call_schedule).  One body per lag, all driven to the floor, then timed in turn, round after round; every body must end bit-equal.

With --fall the falling body is timed instead (what bench.py's `value` runs: frames 6-25 from rest, fewer rotation iterations per tet): a
fresh body per lag and round, lags in turn inside a round.

    python tools/call_lag_ab.py [--fall] [cells] [rounds] [lag ...]      ->  profiles/r07_call_schedule_ab.txt
"""
import os
import sys
import time

import numpy as np

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
from tetsim_amd import SoftBodyHIP, make_lattice  # noqa: E402

PP = dict(gravity=-9.81, friction=1000.0, density=1000.0, devCompliance=1e-5, volCompliance=0.0, worldBounds=[-2.5, -1.0, -2.5, 2.5, 10.0, 2.5])
DT = (1.0 / 60.0) / 20
SUB = 20


def frames(body, n):
    body.sync()
    t0 = time.perf_counter()
    for _ in range(n):
        body.simulateSubsteps(SUB, DT, PP)
    body.sync()
    return (time.perf_counter() - t0) / (n * SUB) * 1e6


def body_with_lag(v, t, lag):
    os.environ["TETSIM_PJ_CALL_LAG"] = str(lag)
    try:
        b = SoftBodyHIP(v, t, None, dict(PP), solver="polar", precision="fast")
    finally:
        del os.environ["TETSIM_PJ_CALL_LAG"]
    assert b.info.fused_particle_pass == 5
    return b


def falling(v, t, lags, rounds):
    fall = {lag: [] for lag in lags}
    end = {}
    for _ in range(rounds):
        for lag in lags:
            b = body_with_lag(v, t, lag)
            frames(b, 5)
            fall[lag].append(frames(b, 20))
            end[lag] = b.pos
            b.close()
    print("%6s | %9s %9s %9s | falling, us per substep over frames 6-25, round by round" % ("lag", "min", "median", "max"))
    for lag in lags:
        f = fall[lag]
        print("%6d | %9.2f %9.2f %9.2f | %s" % (lag, min(f), float(np.median(f)), max(f), " ".join("%.2f" % x for x in f)), flush=True)
    same = all(np.array_equal(p.view(np.uint32), end[lags[0]].view(np.uint32)) for p in end.values())
    print("every body bit-equal to lag %d after %d substeps: %s" % (lags[0], 25 * SUB, same))
    return 0 if same else 1


def main():
    argv = [a for a in sys.argv[1:] if a != "--fall"]
    cells = int(argv[0]) if len(argv) > 0 else 55
    rounds = int(argv[1]) if len(argv) > 1 else 7
    lags = [int(x) for x in argv[2:]] or [0, 1, 2, 4, 8, 16, 32, 64, 128, 256]
    v, t = make_lattice(cells)
    print("lattice %d^3 cells, %d tets, %d particles; calls of %d substeps; %d rounds, lags alternate inside a round" % (cells, len(t), len(v), SUB, rounds))
    if "--fall" in sys.argv[1:]:
        return falling(v, t, lags, rounds)
    bodies = {lag: body_with_lag(v, t, lag) for lag in lags}
    fall = {lag: (frames(b, 5), frames(b, 20))[1] for lag, b in bodies.items()}
    for b in bodies.values():
        frames(b, 15)               # the body reaches the floor around frame 19 and settles
    floor = {lag: [] for lag in lags}
    for _ in range(rounds):
        for lag, b in bodies.items():
            floor[lag].append(frames(b, 10))
    print("%6s %9s | %9s %9s %9s | floor us per substep, round by round" % ("lag", "fall us", "min", "median", "max"))
    for lag in lags:
        f = floor[lag]
        print("%6d %9.2f | %9.2f %9.2f %9.2f | %s" % (lag, fall[lag], min(f), float(np.median(f)), max(f), " ".join("%.2f" % x for x in f)), flush=True)
    ref = bodies[lags[0]]
    same = all(np.array_equal(b.pos.view(np.uint32), ref.pos.view(np.uint32)) and np.array_equal(b.quats.view(np.uint32), ref.quats.view(np.uint32))
               for b in bodies.values())
    print("every body bit-equal to lag %d after %d substeps: %s" % (lags[0], (40 + 10 * rounds) * SUB, same))
    return 0 if same else 1


if __name__ == "__main__":
    sys.exit(main())
