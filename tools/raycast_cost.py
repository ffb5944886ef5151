"""What picking costs (tetsim_raycast_visual / tetsim_start_grab_ray), host wall time around the synchronous calls, median of repeated
calls after warm-up, on the Dragon (59,657 triangles) and on the 55-cell lattice's boundary surface (36,300 triangles):
  * one pick: tetsim_start_grab_ray against the only way without it -- tetsim_read_visual_mesh + the ray cast on the host
    (tests/raycast_ref.py, numpy) + tetsim_start_grab -- timed in the same run;
  * 1,024 and 65,536 rays per call: time per call and ray-triangle tests per second.  The time is the whole call as a Python caller
    sees it: packing the rays, the copy in, skinning, the sphere, the kernels, one synchronisation, the copy out (and the host's
    per-hit body lookup on a batch) -- not the kernels alone;
  * the chip's f64 vector rate from a measured f64 FMA loop of our own (tools/micro/f64_fma_rate.hip, run as a child process), to
    set the brute-force arithmetic against: a ray-triangle test that leaves at the back-face check is about 25 f64 operations, a
    full one about 70.
    python tools/raycast_cost.py [--reps 20]"""
import argparse
import os
import subprocess
import sys
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tests"))
import numpy as np  # noqa: E402

import raycast_ref  # noqa: E402
from tetsim_amd import SoftBodyHIP, boundary_surface, library_info, make_lattice  # noqa: E402

PP = dict(gravity=-9.81, friction=1000.0, density=1000.0, devCompliance=1e-5, volCompliance=0.0, worldBounds=[-2.5, -1.0, -2.5, 2.5, 10.0, 2.5])
G = os.path.join(ROOT, "tests", "golden")


def median_ms(fn, reps):
    fn()
    fn()
    ts = []
    for _ in range(reps):
        t0 = time.perf_counter()
        fn()
        ts.append(1e3 * (time.perf_counter() - t0))
    return sorted(ts)[len(ts) // 2]


def f64_fma_loop():
    """Build (if need be) and run tools/micro/f64_fma_rate.hip in a child process; its output lines."""
    src = os.path.join(ROOT, "tools", "micro", "f64_fma_rate.hip")
    exe = os.path.join(ROOT, "tools", "micro", "bin", "f64_fma_rate")
    if not os.path.exists(exe) or os.path.getmtime(exe) < os.path.getmtime(src):
        os.makedirs(os.path.dirname(exe), exist_ok=True)
        subprocess.run([os.environ.get("HIPCC", "/opt/rocm/bin/hipcc"), "--offload-arch=gfx950", "-O3", src, "-o", exe], check=True, capture_output=True)
    return subprocess.run([exe], check=True, capture_output=True, text=True, timeout=120).stdout.strip().splitlines()


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--reps", type=int, default=20)
    ap.add_argument("--cells", type=int, default=55)
    a = ap.parse_args()
    print("library source_sha", library_info()["source_sha"])
    for line in f64_fma_loop():
        print(line, flush=True)
    dv = np.fromfile(os.path.join(G, "dragon_verts.f32"), dtype="<f4").reshape(-1, 3)
    dt_ = np.fromfile(os.path.join(G, "dragon_tets.i32"), dtype="<i4").reshape(-1, 4)
    dvis = np.fromfile(os.path.join(G, "dragon_vis.f32"), dtype="<f4").reshape(-1, 4)
    dtri = np.fromfile(os.path.join(G, "dragon_vistris.u16"), dtype="<u2").astype(np.int32).reshape(-1, 3)
    lv, lt = make_lattice(a.cells)
    lvis, ltri = boundary_surface(lt, len(lv), lv)
    for name, v, t, vis, tri in (("dragon", dv, dt_, dvis, dtri), ("lattice %d cells" % a.cells, lv, lt, lvis, ltri)):
        body = SoftBodyHIP(v, t, None, dict(PP), vis, tri, solver="polar", precision="fast")
        body.simulateSubsteps(20, (1.0 / 60.0) / 20, PP)
        body.sync()
        pos = body.visualPositions()
        c, r = raycast_ref.bounding_sphere(pos)
        o, d = c + [0.0, 3.0 * r, 0.0], np.array([0.0, -1.0, 0.0])

        def host_pick():
            p = body.visualPositions()
            h = raycast_ref.raycast(p, tri, [o], [d])[0]
            if h["hit"]:
                body.startGrab((o + d * h["distance"]).astype(np.float32))

        dev = median_ms(lambda: body.startGrabRay(o, d), a.reps)
        host = median_ms(host_pick, a.reps)
        read = median_ms(lambda: body.visualPositions(), a.reps)
        print("%-18s %6d triangles  one pick: device %.3f ms, host path %.3f ms (of which the mesh read-back %.3f ms)" % (name, len(tri), dev, host, read), flush=True)
        rng = np.random.default_rng(1)
        for n in (1024, 65536):
            u = rng.standard_normal((n, 3))
            u /= np.linalg.norm(u, axis=1, keepdims=True)
            w = rng.standard_normal((n, 3))
            w *= (rng.random(n) ** (1.0 / 3.0) / np.linalg.norm(w, axis=1))[:, None]
            oo = c + 3.0 * r * u
            dd = (c + r * w) - oo
            dd /= np.linalg.norm(dd, axis=1, keepdims=True)
            ms = median_ms(lambda: body.raycastVisual(oo, dd), max(5, a.reps // 2))
            print("%-18s %6d rays per call (whole call, host side included): %.3f ms, %.3g ray-triangle tests per second" % (name, n, ms, n * len(tri) / (ms * 1e-3)), flush=True)
        body.close()


if __name__ == "__main__":
    main()
