"""What the per-tet strain costs (include/tetsim.h: tetsim_tet_strain_device / tetsim_body_strain_device) on the headline lattice (55
cells: 998,250 tets, one body; polar FAST), on an idle handle:
  (a) tetStrainDevice() into packed rows (the LDS-staged stores), into rows 80 bytes apart (dword stores per row), and bodyStrainDevice():
      device time between two events recorded on torch's stream around the call -- the window holds the launches and the contract's two
      cross-stream event waits, no host synchronisation; median of --reps calls after 5 warm-ups;
  (b) the same calls back to back, --burst of them inside one pair of events, per call: the event waits overlap, so this is nearer the
      kernel's own time;
  (c) what the chip's own streaming copy (tetsim_measure_stream_bandwidth, kind = copy) needs for the same bytes: the 64-byte record read
      plus the 64-byte row written per tet -- the gathered particle rows are expected to stay in cache.
    python tools/strain_cost.py [--reps 20] [--burst 20] [--cells 55] [--out profiles/strain_cost.txt]"""
import argparse
import os
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
import torch  # noqa: E402

from tetsim_amd import SoftBodyHIP, library_info, make_lattice  # noqa: E402
from tetsim_amd import _capi as c  # noqa: E402
from tetsim_amd.softbody import measure_stream_bandwidth  # noqa: E402

PP = dict(gravity=-9.81, friction=1000.0, density=1000.0, devCompliance=1e-5, volCompliance=0.0, worldBounds=[-2.5, -1.0, -2.5, 2.5, 10.0, 2.5])
DT = (1.0 / 60.0) / 20


def spread(ts):
    ts = sorted(ts)
    return ts[len(ts) // 2], ts[len(ts) // 10], ts[(9 * len(ts)) // 10]


def device_us(body, fn, reps, burst=1):
    body.sync()
    torch.cuda.synchronize()
    ts = []
    for _ in range(reps + 5):
        e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        e0.record()
        for _ in range(burst):
            fn()
        e1.record()
        torch.cuda.synchronize()
        ts.append(1e3 * e0.elapsed_time(e1) / burst)
    return spread(ts[5:])


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--reps", type=int, default=20)
    ap.add_argument("--burst", type=int, default=20)
    ap.add_argument("--cells", type=int, default=55)
    ap.add_argument("--out", default=None)
    a = ap.parse_args()
    lines = []

    def say(s):
        print(s, flush=True)
        lines.append(s)

    lib = library_info()
    say("library source_sha %s kernel_sha %s torch %s; medians of %d after 5 warm-ups (10%%, 90%%)" % (lib["source_sha"], lib["kernel_sha"], torch.__version__, a.reps))
    torch.zeros(1, device="cuda")
    v, t = make_lattice(a.cells)
    body = SoftBodyHIP(v, t, None, dict(PP), solver="polar", precision="fast")
    body.simulateSubsteps(20, DT, PP)
    nt = body.info.num_elems
    say("lattice %d cells: %d particles, %d tets, %d Jacobi sweeps" % (a.cells, body.info.owned_particles, nt, c.STRAIN_SWEEPS))
    packed = body.tetStrainDevice()
    wide = torch.empty((nt, 20), dtype=torch.float32, device="cuda")[:, :c.STRAIN_WIDTH]
    body.tetStrainDevice(out=wide)
    torch.cuda.synchronize()
    assert torch.equal(packed.view(torch.int32), wide.contiguous().view(torch.int32))
    calls = (("tetStrainDevice, packed rows (staged in LDS)", body.tetStrainDevice), ("tetStrainDevice, rows 80 bytes apart (dword stores)", lambda: body.tetStrainDevice(out=wide)),
             ("bodyStrainDevice (no rows written)", body.bodyStrainDevice))
    single = {}
    for name, fn in calls:
        single[name] = device_us(body, fn, a.reps)
        per = device_us(body, fn, a.reps, a.burst)
        say("  %-52s %8.1f us device (%.1f, %.1f); %d back to back: %.1f us each (%.1f, %.1f)" % ((name,) + single[name] + (a.burst,) + per))
        single[name + "/burst"] = per
    moved = 128 * nt
    gbps = measure_stream_bandwidth(64 * nt, "copy", reps=20)
    probe_us = moved / (gbps * 1e3)
    say("  copy probe at %d bytes read + %d written (64 + 64 per tet): %.0f GB/s = %.1f us" % (64 * nt, 64 * nt, gbps, probe_us))
    name = calls[0][0]
    say("  packed rows / copy probe = %.2f (one call), %.2f (back to back)" % (single[name][0] / probe_us, single[name + "/burst"][0] / probe_us))
    body.close()
    if a.out:
        with open(a.out, "w") as f:
            f.write("\n".join(lines) + "\n")


if __name__ == "__main__":
    main()
