"""What a frame costs a PyTorch consumer of the positions, per frame of 20 substeps, on the headline lattice (55 cells: 1 M tets,
175,616 particles) and on the Dragon, polar FAST -- host wall time around work that ends in a synchronisation, median of repeated
frames after warm-up:
  (s) the substeps alone: tetsim_step_n + tetsim_sync -- what every route below contains;
  (a) today's route without the device hand-over: tetsim_step_n, tetsim_read_positions_pinned (a stream drain, a pack kernel, a copy
      to pinned host memory), then torch.from_numpy(...).cuda() (the copy back);
  (b) tetsim_step_n, exportTensors(("pos",)), torch.cuda.synchronize();
  (c) the export alone on an idle handle, by device events recorded on torch's stream around the call: the gather kernel and the two
      cross-stream event waits of the contract (no substep in flight, no host synchronisation inside the window).
(a) - (s) and (b) - (s) are what the hand-over itself adds to a frame.  Route (a) uses only entry points that exist without
tetsim_export_device, so its figure is the baseline whichever build runs it.
Then the entry points that move rows, one by one on an idle handle with a visual mesh (the Dragon's own; the lattice's boundary):
host wall time of a single call through the Python binding, median of --calls calls after warm-up -- the copying and the pinned
reads, tetsim_write_state of the body's own state, and tetsim_export_device of positions + quaternions followed by
torch.cuda.synchronize().  Lines that start with "call" are meant to be compared across builds (TETSIM_HIP_LIB selects the library;
profiles/state_io_cost.txt).
    python tools/device_io_cost.py [--reps 50] [--cells 55] [--calls 200]"""
import argparse
import os
import sys
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
import numpy as np  # noqa: E402
import torch  # noqa: E402

from tetsim_amd import SoftBodyHIP, boundary_surface, library_info, make_lattice  # noqa: E402

PP = dict(gravity=-9.81, friction=1000.0, density=1000.0, devCompliance=1e-5, volCompliance=0.0, worldBounds=[-2.5, -1.0, -2.5, 2.5, 10.0, 2.5])
G = os.path.join(ROOT, "tests", "golden")
DT = (1.0 / 60.0) / 20


def median_us(fn, reps):
    for _ in range(5):
        fn()
    ts = []
    for _ in range(reps):
        t0 = time.perf_counter()
        fn()
        ts.append(1e6 * (time.perf_counter() - t0))
    ts.sort()
    return ts[len(ts) // 2], ts[len(ts) // 10], ts[(9 * len(ts)) // 10]


def per_call(name, body, calls):
    pos, vel = body.pos, body.vel

    def export():
        body.exportTensors(("pos", "quats"))
        torch.cuda.synchronize()

    rows = [("tetsim_read_positions", lambda: body.pos), ("tetsim_read_positions_pinned", lambda: body.posPinned),
            ("tetsim_read_quats_pinned", lambda: body.quatsPinned), ("tetsim_read_visual_mesh", body.visualPositions),
            ("tetsim_write_state", lambda: body.writeState(pos, vel)), ("tetsim_export_device(pos+quats)", export)]
    for label, fn in rows:
        body.sync()
        m, lo, hi = median_us(fn, calls)
        print("call %-8s %-34s %9.1f us median of %d (10%% %.1f, 90%% %.1f)" % (name.split()[0], label, m, calls, lo, hi), flush=True)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--reps", type=int, default=50)
    ap.add_argument("--cells", type=int, default=55)
    ap.add_argument("--calls", type=int, default=200)
    a = ap.parse_args()
    print("library source_sha", library_info()["source_sha"], "torch", torch.__version__, flush=True)
    dv = np.fromfile(os.path.join(G, "dragon_verts.f32"), dtype="<f4").reshape(-1, 3)
    dt_ = np.fromfile(os.path.join(G, "dragon_tets.i32"), dtype="<i4").reshape(-1, 4)
    lv, lt = make_lattice(a.cells)
    torch.zeros(1, device="cuda")
    for name, v, t in (("lattice %d cells" % a.cells, lv, lt), ("dragon", dv, dt_)):
        body = SoftBodyHIP(v, t, None, dict(PP), solver="polar", precision="fast")
        n = body.info.owned_particles

        def steps():
            body.simulateSubsteps(20, DT, PP)
            body.sync()

        def host_route():
            body.simulateSubsteps(20, DT, PP)
            return torch.from_numpy(body.posPinned).cuda()

        def device_route():
            body.simulateSubsteps(20, DT, PP)
            out = body.exportTensors(("pos",))["pos"]
            torch.cuda.synchronize()
            return out

        rows = [("(s) 20 substeps + sync", steps), ("(a) + read_positions_pinned + from_numpy().cuda()", host_route),
                ("(b) + exportTensors + torch.cuda.synchronize()", device_route)]
        got = {}
        for _ in range(2):   # the three routes alternate: two passes, the second is reported
            for label, fn in rows:
                got[label] = median_us(fn, a.reps)
        same = np.array_equal(host_route().cpu().numpy().view(np.uint32), body.pos.view(np.uint32)) and \
            np.array_equal(device_route().cpu().numpy().view(np.uint32), body.pos.view(np.uint32))
        print("%s: %d particles, %d tets; both routes equal tetsim_read_positions bit for bit: %s" % (name, n, body.info.num_elems, same), flush=True)
        for label, _ in rows:
            m, lo, hi = got[label]
            print("  %-52s %9.1f us per frame (10%% %.1f, 90%% %.1f)" % (label, m, lo, hi), flush=True)
        s = got[rows[0][0]][0]
        print("  the hand-over's share of a frame: host route (a) - (s) = %.1f us, device route (b) - (s) = %.1f us" % (got[rows[1][0]][0] - s, got[rows[2][0]][0] - s), flush=True)
        body.sync()
        torch.cuda.synchronize()
        ev = []
        for _ in range(a.reps + 5):
            e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
            e0.record()
            body.exportTensors(("pos",))
            e1.record()
            torch.cuda.synchronize()
            ev.append(1e3 * e0.elapsed_time(e1))
        ev = sorted(ev[5:])
        bytes_moved = n * (16 + 4 + 12)   # a float4 through a 4-byte index, 12 bytes out
        print("  (c) the export alone (gather kernel + the contract's two event waits), device events: %.1f us median (10%% %.1f, 90%% %.1f); "
              "%d bytes moved" % (ev[len(ev) // 2], ev[len(ev) // 10], ev[(9 * len(ev)) // 10], bytes_moved), flush=True)
        vis = np.fromfile(os.path.join(G, "dragon_vis.f32"), dtype="<f4").reshape(-1, 4) if name == "dragon" else boundary_surface(t, len(v), v)[0]
        body.setVisualMesh(vis)
        per_call(name, body, a.calls)
        body.close()


if __name__ == "__main__":
    main()
