"""What a per-body observation costs (include/tetsim.h: tetsim_observe_bodies_device), on the headline lattice (55 cells: 1 M tets, one
body; polar FAST) and on a batch of 64 Dragons (polar FAST), each on an idle handle:
  (a) observeBodies(): device time between two events recorded on torch's stream around the call, so the window holds the two launches and
      the contract's two cross-stream event waits and no host synchronisation; median of --reps calls after 5 warm-ups;
  (b) what a caller can do without it, for the PARTICLE quantities only (box, fastest particle, non-finite count; the tet quantities need the
      tet list): exportTensors(("pos", "vel")) + torch segment reductions (torch.segment_reduce over the bodies' lengths), timed the same way;
  (c) what the chip's own streaming read (tetsim_measure_stream_bandwidth, kind = read) needs for the bytes of the constant table the kernel
      streams, 24 per tet -- the gathered particle rows are expected to stay in cache.
The ratios (a) / (b) and (a) / (c) are the figures DESIGN.md 9.3 quotes.
    python tools/observe_cost.py [--reps 20] [--cells 55] [--bodies 64] [--out profiles/observe_cost.txt]"""
import argparse
import os
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
import numpy as np  # noqa: E402
import torch  # noqa: E402

from tetsim_amd import SoftBodyHIP, library_info, make_lattice  # noqa: E402
from tetsim_amd import _capi as c  # noqa: E402
from tetsim_amd.softbody import measure_stream_bandwidth  # noqa: E402

PP = dict(gravity=-9.81, friction=1000.0, density=1000.0, devCompliance=1e-5, volCompliance=0.0, worldBounds=[-2.5, -1.0, -2.5, 2.5, 10.0, 2.5])
G = os.path.join(ROOT, "tests", "golden")
DT = (1.0 / 60.0) / 20


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


def torch_particle_quantities(body, lengths):
    """Box, max speed^2 and non-finite count per body from an export, with torch's segment reductions."""
    out = body.exportTensors(("pos", "vel"))
    pos, vel = out["pos"].double(), out["vel"].double()
    ok = torch.isfinite(pos).all(dim=1) & torch.isfinite(vel).all(dim=1)
    inf = torch.full_like(pos, float("inf"))
    lo = torch.segment_reduce(torch.where(ok[:, None], pos, inf), "min", lengths=lengths, axis=0)
    hi = torch.segment_reduce(torch.where(ok[:, None], pos, -inf), "max", lengths=lengths, axis=0)
    speed2 = torch.segment_reduce(torch.where(ok, (vel * vel).sum(dim=1), torch.zeros_like(ok, dtype=torch.float64)), "max", lengths=lengths, axis=0)
    bad = torch.segment_reduce((~ok).double(), "sum", lengths=lengths, axis=0)
    return lo, hi, speed2, bad


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
             ("%d dragons" % a.bodies, lambda: SoftBodyHIP.batch(dragons, dict(wide), ref_fixed_bounds=False, solver="polar", precision="fast"), wide)]
    for name, make, pp in works:
        body = make()
        body.simulateSubsteps(20, DT, pp)
        nb, nt = body.info.num_bodies, body.info.num_elems
        lengths = torch.tensor([hi - lo for (lo, hi), _ in body.bodyRanges], device="cuda")
        say("%s: %d bodies, %d particles, %d tets" % (name, nb, body.info.owned_particles, nt))
        obs = body.observeBodies()
        lo, hi, speed2, bad = torch_particle_quantities(body, lengths)
        torch.cuda.synchronize()
        assert torch.equal(obs[:, c.OBS_AABB_MIN:c.OBS_AABB_MIN + 3], lo) and torch.equal(obs[:, c.OBS_AABB_MAX:c.OBS_AABB_MAX + 3], hi)
        assert torch.equal(obs[:, c.OBS_NONFINITE], bad)
        t_obs = device_us(body, body.observeBodies, a.reps)
        t_torch = device_us(body, lambda: torch_particle_quantities(body, lengths), a.reps)
        table = 24 * nt
        gbps = measure_stream_bandwidth(table, "read", reps=20)
        probe_us = table / (gbps * 1e3)
        say("  %-46s %9.1f us device (%.1f, %.1f)" % (("observeBodies (all 20 columns)",) + t_obs))
        say("  %-46s %9.1f us device (%.1f, %.1f)" % (("export pos, vel + torch segment reductions",) + t_torch))
        say("  read probe at %d bytes (the table, 24 per tet): %.0f GB/s = %.1f us" % (table, gbps, probe_us))
        say("  observeBodies / torch (particle columns only) = %.4f; observeBodies / table read = %.1f" % (t_obs[0] / t_torch[0], t_obs[0] / probe_us))
        body.close()
    if a.out:
        with open(a.out, "w") as f:
            f.write("\n".join(lines) + "\n")


if __name__ == "__main__":
    main()
