"""What the sensor call costs (tetsim_raycast_visual_device), between HIP events on the caller's stream, median of repeated calls after
warm-up, on the Dragon (59,657 triangles):
  * 1,024 and 65,536 rays on one Dragon through the new call (ray_body NULL: the whole mesh, what tetsim_raycast_visual casts against);
  * the same rays through tetsim_raycast_visual, whose kernels the caller cannot bracket with events: the wall time of the synchronous
    Python call minus the wall time of its two host copies (count * 64 bytes in, count * 48 bytes out, timed on their own as copies of
    pageable memory).  What is left is MORE than the old kernels: it still holds make_rays and the numpy conversions, the ctypes call,
    the launches' latency and one synchronisation -- host overhead that the event-bracketed figure of the new call does not carry.  At
    65,536 rays that overhead is small against the kernels; at 1,024 rays it is of the size of the difference, so that line compares
    the two calls, not the two kernels.  Therefore also:
  * both calls as a Python caller with host arrays sees them, wall time: raycastVisual against rays_tensor + raycastVisualDevice + a
    synchronisation + the copy of the records to the host -- the same host work on both sides;
  * new and old alternate, `--runs` times each; the old path's own spread over its runs is the allowance of the comparison;
  * 64 x 1,024 rays on a batch of 64 Dragons with ray_body (every ray against its own body), grouped by body and shuffled: ray-triangle
    tests per second, next to the f64 rate of tools/micro/f64_fma_rate.hip.
    python tools/raycast_device_cost.py [--reps 20] [--runs 5] [--bodies 64]"""
import argparse
import os
import sys
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tests"))
sys.path.insert(0, os.path.join(ROOT, "tools"))
import numpy as np  # noqa: E402
import torch  # noqa: E402

import raycast_ref  # noqa: E402
from raycast_cost import PP, G, f64_fma_loop  # noqa: E402
from tetsim_amd import SoftBodyHIP, library_info, rays_tensor  # noqa: E402


def median(xs):
    return sorted(xs)[len(xs) // 2]


def event_ms(fn, reps):
    """median over reps of the time between two events around fn() on torch's current stream"""
    for _ in range(3):
        fn()
    torch.cuda.synchronize()
    ts = []
    for _ in range(reps):
        e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        e0.record()
        fn()
        e1.record()
        e1.synchronize()
        ts.append(e0.elapsed_time(e1))
    return median(ts)


def wall_ms(fn, reps):
    for _ in range(3):
        fn()
    ts = []
    for _ in range(reps):
        t0 = time.perf_counter()
        fn()
        ts.append(1e3 * (time.perf_counter() - t0))
    return median(ts)


def sphere_rays(c, r, n, seed):
    rng = np.random.default_rng(seed)
    u = rng.standard_normal((n, 3))
    u /= np.linalg.norm(u, axis=1, keepdims=True)
    w = rng.standard_normal((n, 3))
    w *= (rng.random(n) ** (1.0 / 3.0) / np.linalg.norm(w, axis=1))[:, None]
    o = c + 3.0 * r * u
    d = (c + r * w) - o
    return o, d / np.linalg.norm(d, axis=1, keepdims=True)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--reps", type=int, default=20)
    ap.add_argument("--runs", type=int, default=5)
    ap.add_argument("--bodies", type=int, default=64)
    a = ap.parse_args()
    print("library source_sha", library_info()["source_sha"])
    fma = f64_fma_loop()
    for line in fma:
        print(line, flush=True)
    dv = np.fromfile(os.path.join(G, "dragon_verts.f32"), dtype="<f4").reshape(-1, 3)
    dt_ = np.fromfile(os.path.join(G, "dragon_tets.i32"), dtype="<i4").reshape(-1, 4)
    dvis = np.fromfile(os.path.join(G, "dragon_vis.f32"), dtype="<f4").reshape(-1, 4)
    dtri = np.fromfile(os.path.join(G, "dragon_vistris.u16"), dtype="<u2").astype(np.int32).reshape(-1, 3)
    ntri = len(dtri)
    body = SoftBodyHIP(dv, dt_, None, dict(PP), dvis, dtri, solver="polar", precision="fast")
    body.simulateSubsteps(20, (1.0 / 60.0) / 20, PP)
    body.sync()
    c, r = raycast_ref.bounding_sphere(body.visualPositions())
    for n in (1024, 65536):
        o, d = sphere_rays(c, r, n, 1)
        rays = rays_tensor(o, d)
        host_in, host_out = np.zeros(n * 64, np.uint8), np.zeros(n * 48, np.uint8)
        dev_in, dev_out = torch.zeros(n * 64, dtype=torch.uint8, device="cuda"), torch.zeros(n * 48, dtype=torch.uint8, device="cuda")
        tin, tout = torch.from_numpy(host_in), torch.from_numpy(host_out)

        def copies():
            dev_in.copy_(tin)
            torch.cuda.synchronize()
            tout.copy_(dev_out)

        def new_from_host():
            res = body.raycastVisualDevice(rays_tensor(o, d))
            torch.cuda.synchronize()
            return res["raw"].cpu()

        new, old, cop, new_wall, old_wall = [], [], [], [], []
        for _ in range(a.runs):
            new.append(event_ms(lambda: body.raycastVisualDevice(rays), a.reps))
            whole, cp = wall_ms(lambda: body.raycastVisual(o, d), a.reps), wall_ms(copies, a.reps)
            old.append(whole - cp)
            cop.append(cp)
            old_wall.append(whole)
            new_wall.append(wall_ms(new_from_host, a.reps))
        fmt = lambda xs: " ".join("%.3f" % x for x in xs)  # noqa: E731
        print("dragon %6d rays, new call, events on the caller's stream (ms per run): %s  median %.3f" % (n, fmt(new), median(new)), flush=True)
        print("dragon %6d rays, tetsim_raycast_visual, wall minus its two host copies (ms per run): %s  median %.3f  spread %.3f  (the copies: %s)"
              % (n, fmt(old), median(old), max(old) - min(old), fmt(cop)), flush=True)
        print("dragon %6d rays, both calls from host arrays to host records, wall (ms per run): new %s  median %.3f; old %s  median %.3f  spread %.3f"
              % (n, fmt(new_wall), median(new_wall), fmt(old_wall), median(old_wall), max(old_wall) - min(old_wall)), flush=True)
        print("dragon %6d rays: new %.3f ms vs old %.3f ms (+ spread %.3f): %s; %.3g ray-triangle tests per second" %
              (n, median(new), median(old), max(old) - min(old), "not above" if median(new) <= median(old) + (max(old) - min(old)) else "ABOVE",
               n * ntri / (median(new) * 1e-3)), flush=True)
    body.close()
    nb, per = a.bodies, 1024
    batch = SoftBodyHIP.batch([(dv, dt_)] * nb, dict(PP), solver="polar", precision="fast")
    batch.setVisualMesh(np.concatenate([dvis + np.array([k * len(dt_), 0, 0, 0], np.float32) for k in range(nb)]))
    batch.setVisualTriangles(np.concatenate([dtri + k * len(dvis) for k in range(nb)]))
    batch.simulateSubsteps(20, (1.0 / 60.0) / 20, PP)
    batch.sync()
    o, d = sphere_rays(c, r, nb * per, 2)
    ids = np.repeat(np.arange(nb, dtype=np.int32), per)
    perm = np.random.default_rng(3).permutation(nb * per)
    for name, order in (("grouped by body", np.arange(nb * per)), ("shuffled", perm)):
        rays, bodies = rays_tensor(o[order], d[order]), torch.from_numpy(ids[order]).cuda()
        few = name == "shuffled"   # (a workgroup goes through every body its rays name: about `bodies` times the grouped call)
        ms = [event_ms(lambda: batch.raycastVisualDevice(rays, bodies), max(3, a.reps // 6) if few else a.reps) for _ in range(1 if few else a.runs)]
        print("batch of %d dragons, %d x %d rays with ray_body, %s (ms per run): %s  median %.3f; %.3g ray-triangle tests per second" %
              (nb, nb, per, name, " ".join("%.3f" % x for x in ms), median(ms), nb * per * ntri / (median(ms) * 1e-3)), flush=True)
    ms = event_ms(lambda: batch.visualBoundingSpheresDevice(), a.reps)
    print("batch of %d dragons, visualBoundingSpheresDevice (skinning included): %.3f ms" % (nb, ms), flush=True)


if __name__ == "__main__":
    main()
