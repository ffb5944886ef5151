"""What a device snapshot costs (include/tetsim.h: tetsim_snapshot_*), on the headline lattice (55 cells: 1 M tets; polar FAST, default and
lean tet record) and on a batch of 64 Dragons (polar FAST), each on an idle handle:
  restore with a NULL mask, restore of one body of the batch (mask on the device), capture with a NULL mask -- device time between two
  events recorded on torch's stream around the call, so the window holds the one kernel and the contract's two cross-stream event waits
  and no host synchronisation; median of --reps calls after 5 warm-ups;
  beside them the host wall time of saveState + loadState of the same body (the only complete restore without a snapshot), and what the
  chip's own float4 copy (tetsim_measure_stream_bandwidth, kind = copy) needs for the bytes a NULL-mask call moves (the payload read
  once and written once) -- the ratio of the two is the figure DESIGN.md quotes.
    python tools/snapshot_cost.py [--reps 20] [--cells 55] [--bodies 64] [--out profiles/snapshot_cost.txt]"""
import argparse
import os
import sys
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
import numpy as np  # noqa: E402
import torch  # noqa: E402

from tetsim_amd import SoftBodyHIP, library_info, make_lattice  # noqa: E402
from tetsim_amd.softbody import measure_stream_bandwidth  # noqa: E402

PP = dict(gravity=-9.81, friction=1000.0, density=1000.0, devCompliance=1e-5, volCompliance=0.0, worldBounds=[-2.5, -1.0, -2.5, 2.5, 10.0, 2.5])
G = os.path.join(ROOT, "tests", "golden")
DT = (1.0 / 60.0) / 20
HEADER = 64   # bytes of a state blob in front of its payload


def spread(ts):
    ts = sorted(ts)
    return ts[len(ts) // 2], ts[len(ts) // 10], ts[(9 * len(ts)) // 10]


def device_us(body, fn, reps):
    body.sync()
    torch.cuda.synchronize()
    ts = []
    for _ in range(reps + 5):
        e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        e0.record()
        fn()
        e1.record()
        torch.cuda.synchronize()
        ts.append(1e3 * e0.elapsed_time(e1))
    return spread(ts[5:])


def host_us(fn, reps):
    ts = []
    for _ in range(reps + 5):
        t0 = time.perf_counter()
        fn()
        ts.append(1e6 * (time.perf_counter() - t0))
    return spread(ts[5:])


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--reps", type=int, default=20)
    ap.add_argument("--cells", type=int, default=55)
    ap.add_argument("--bodies", type=int, default=64)
    ap.add_argument("--out", default=None)
    a = ap.parse_args()
    lines = []

    def say(s):
        print(s, flush=True)
        lines.append(s)

    say("library source_sha %s torch %s; medians of %d after 5 warm-ups (10%%, 90%%)" % (library_info()["source_sha"], torch.__version__, a.reps))
    torch.zeros(1, device="cuda")
    lv, lt = make_lattice(a.cells)
    dv = np.fromfile(os.path.join(G, "dragon_verts.f32"), dtype="<f4").reshape(-1, 3)
    dt_ = np.fromfile(os.path.join(G, "dragon_tets.i32"), dtype="<i4").reshape(-1, 4)
    side = int(np.ceil(np.sqrt(a.bodies)))
    dragons = [((dv + np.array([3.0 * (b % side), 0.0, 2.0 * (b // side)], np.float32)).astype(np.float32), dt_) for b in range(a.bodies)]
    wide = dict(PP, worldBounds=[-5.0, -1.0, -5.0, 3.0 * side + 5.0, 10.0, 2.0 * side + 5.0])
    works = [("lattice %d cells" % a.cells, lambda: SoftBodyHIP(lv, lt, None, dict(PP), solver="polar", precision="fast"), PP),
             ("lattice %d cells, lean" % a.cells, lambda: SoftBodyHIP(lv, lt, None, dict(PP), solver="polar", precision="fast", lean_state=True), PP),
             ("%d dragons" % a.bodies, lambda: SoftBodyHIP.batch(dragons, dict(wide), ref_fixed_bounds=False, solver="polar", precision="fast"), wide)]
    for name, make, pp in works:
        body = make()
        body.simulateSubsteps(20, DT, pp)
        snap = body.snapshot()
        blob = body.saveState()
        payload = len(blob) - HEADER
        nb = body.info.num_bodies
        one = torch.zeros(nb, dtype=torch.bool, device="cuda")
        one[nb // 2] = True
        say("%s: %d bodies, %d particles, %d tets, fused_particle_pass %d, payload %d bytes" %
            (name, nb, body.info.owned_particles, body.info.num_elems, body.info.fused_particle_pass, payload))
        got = {}
        for label, fn in (("restore, NULL mask", lambda: body.restore(snap)), ("restore, one body of %d" % nb, lambda: body.restore(snap, bodies=one)),
                          ("capture, NULL mask", lambda: body.capture(snap))):
            got[label] = device_us(body, fn, a.reps)
            say("  %-28s %9.1f us device (%.1f, %.1f)" % ((label,) + got[label]))
        body.restore(snap)
        body.sync()
        assert body.saveState() == blob
        m = host_us(lambda: body.loadState(body.saveState()), a.reps)
        say("  %-28s %9.1f us host wall (%.1f, %.1f)" % (("saveState + loadState",) + m))
        gbps = measure_stream_bandwidth(payload, "copy", reps=20)
        probe_us = 2.0 * payload / (gbps * 1e3)
        r = got["restore, NULL mask"][0]
        say("  copy probe at %d bytes: %.0f GB/s (read + write) = %.1f us for the payload; NULL-mask restore / probe = %.2f, i.e. %.0f GB/s" %
            (payload, gbps, probe_us, r / probe_us, 2.0 * payload / (r * 1e3)))
        snap.close()
        body.close()
    if a.out:
        with open(a.out, "w") as f:
            f.write("\n".join(lines) + "\n")


if __name__ == "__main__":
    main()
