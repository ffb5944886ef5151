"""What the sensor call through the refitted tree costs (tetsim_raycast_visual_bvh_device) next to the brute-force call
(tetsim_raycast_visual_device: unchanged code, the baseline) in the same build and session, on the Dragon (59,657 triangles).  Time
between HIP events on the caller's stream, median of `--reps` calls after warm-up; the two calls alternate, `--runs` rounds; the
brute-force call's own spread over its rounds is the allowance of the comparison.  Shapes, both calls each:
  1. one Dragon, 1,024 rays;  2. one Dragon, 65,536 rays;  5. one Dragon, 16 rays (where the refit dominates);
  3. 64 Dragons, 64 x 1,024 rays with ray_body, grouped by body;  4. the same rays shuffled.
(Calls of more than 50 ms are timed a sixth as often.)  Also: the first call's host build (wall), the tree's bytes per triangle, and --
in a child process on a development build of the library (-DTETSIM_BVH_STATS: libtetsim_hip_bvhstats.so, built here if it is missing) --
the refit alone and the traversal's statistics: boxes and triangles tested per ray, and the slowest lane's boxes per wave of 64 rays.
    python tools/raycast_bvh_cost.py [--reps 20] [--runs 5] [--bodies 64] [--out profiles/raycast_bvh_cost.txt]"""
import argparse
import ctypes as C
import os
import subprocess
import sys
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tests"))
sys.path.insert(0, os.path.join(ROOT, "tools"))
import numpy as np  # noqa: E402
import torch  # noqa: E402

import raycast_ref  # noqa: E402
from raycast_cost import PP, G  # noqa: E402
from raycast_device_cost import median, sphere_rays  # noqa: E402
from tetsim_amd import SoftBodyHIP, library_info, rays_tensor  # noqa: E402
from tetsim_amd import _capi as capi  # noqa: E402

STATS_LIB = os.path.join(ROOT, "tetsim_amd", "libtetsim_hip_bvhstats.so")
LINES = []


def say(text):
    print(text, flush=True)
    LINES.append(text)


def event_ms(fn, reps):
    """median over reps of the time between two events around fn() on torch's current stream; a slow call is repeated less often"""
    fn()
    torch.cuda.synchronize()
    ts = []
    for k in range(3 + reps):
        e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        e0.record()
        fn()
        e1.record()
        e1.synchronize()
        ts.append(e0.elapsed_time(e1))
        if k == 0 and ts[0] > 50.0:
            reps = max(3, reps // 6)
        if len(ts) >= 3 + reps:
            break
    return median(ts[3:])


def dragon():
    dv = np.fromfile(os.path.join(G, "dragon_verts.f32"), dtype="<f4").reshape(-1, 3)
    dt_ = np.fromfile(os.path.join(G, "dragon_tets.i32"), dtype="<i4").reshape(-1, 4)
    dvis = np.fromfile(os.path.join(G, "dragon_vis.f32"), dtype="<f4").reshape(-1, 4)
    dtri = np.fromfile(os.path.join(G, "dragon_vistris.u16"), dtype="<u2").astype(np.int32).reshape(-1, 3)
    return dv, dt_, dvis, dtri


def one_dragon():
    dv, dt_, dvis, dtri = dragon()
    body = SoftBodyHIP(dv, dt_, None, dict(PP), dvis, dtri, solver="polar", precision="fast")
    body.simulateSubsteps(20, (1.0 / 60.0) / 20, PP)
    body.sync()
    return body, len(dtri)


def many_dragons(nb):
    dv, dt_, dvis, dtri = dragon()
    batch = SoftBodyHIP.batch([(dv, dt_)] * nb, dict(PP), solver="polar", precision="fast")
    batch.setVisualMesh(np.concatenate([dvis + np.array([k * len(dt_), 0, 0, 0], np.float32) for k in range(nb)]))
    batch.setVisualTriangles(np.concatenate([dtri + k * len(dvis) for k in range(nb)]))
    batch.simulateSubsteps(20, (1.0 / 60.0) / 20, PP)
    batch.sync()
    return batch


def device_bytes(body):
    info = capi.TetSimInfo()
    capi.check(body._L.tetsim_get_info(body._h, C.byref(info)), body._h)
    return info.device_bytes


def same_records(a, b):
    return bool(torch.equal(a["raw"], b["raw"]))


def compare(name, body, rays, bodies, a):
    """both calls alternating, a.runs rounds; the verdict against the brute-force call's own spread"""
    tree, brute = [], []
    same = same_records(body.raycastVisualBvhDevice(rays, bodies, out=torch.empty((len(rays), 48), dtype=torch.uint8, device="cuda")),
                        body.raycastVisualDevice(rays, bodies, out=torch.empty((len(rays), 48), dtype=torch.uint8, device="cuda")))
    for _ in range(a.runs):
        tree.append(event_ms(lambda: body.raycastVisualBvhDevice(rays, bodies), a.reps))
        brute.append(event_ms(lambda: body.raycastVisualDevice(rays, bodies), a.reps))
    fmt = lambda xs: " ".join("%.3f" % x for x in xs)  # noqa: E731
    spread = max(brute) - min(brute)
    verdict = "BELOW by more than the spread" if median(tree) < median(brute) - spread else "not below by more than the spread"
    say("%s (ms per round): tree %s  median %.3f | brute force %s  median %.3f  spread %.3f | %.1fx, %s; records %s" %
        (name, fmt(tree), median(tree), fmt(brute), median(brute), spread, median(brute) / median(tree), verdict, "equal" if same else "DIFFER"))
    return median(tree), median(brute)


def stats_child(a):
    """in a process of its own, on the development build: the refit alone and what the traversal tests"""
    L = capi.lib()
    L.tetsim_debug_bvh_stats.argtypes = [C.c_void_p, C.c_void_p]
    L.tetsim_debug_bvh_refit.argtypes = [C.c_void_p, C.c_void_p]
    body, ntri = one_dragon()
    c, r = raycast_ref.bounding_sphere(body.visualPositions())
    shapes = []
    for n in (16, 1024, 65536):
        o, d = sphere_rays(c, r, n, 1)
        shapes.append(("one dragon, %d rays" % n, body, rays_tensor(o, d), None))
    batch = many_dragons(a.bodies)
    nb, per = a.bodies, 1024
    o, d = sphere_rays(c, r, nb * per, 2)
    ids = np.repeat(np.arange(nb, dtype=np.int32), per)
    perm = np.random.default_rng(3).permutation(nb * per)
    for name, order in (("grouped by body", np.arange(nb * per)), ("shuffled", perm)):
        shapes.append(("%d dragons, %d x %d rays, %s" % (nb, nb, per, name), batch, rays_tensor(o[order], d[order]), torch.from_numpy(ids[order]).cuda()))
    for name, h, rays, bodies in shapes:
        stats = torch.zeros((len(rays), 2), dtype=torch.int32, device="cuda")
        capi.check(L.tetsim_debug_bvh_stats(h._h, stats.data_ptr()), h._h)
        res = h.raycastVisualBvhDevice(rays, bodies)
        torch.cuda.synchronize()
        capi.check(L.tetsim_debug_bvh_stats(h._h, None), h._h)
        s = stats.cpu().numpy().astype(np.int64)
        boxes, tris = s[:, 0], s[:, 1]
        full = len(boxes) // 64 * 64
        wave = boxes[:full].reshape(-1, 64) if full else boxes.reshape(1, -1)
        say("%s: hits %d; per ray boxes tested mean %.1f max %d, triangles tested mean %.1f max %d (of %d); per wave of 64 rays the slowest lane's boxes "
            "mean %.1f, %.2fx the wave's mean lane" % (name, int((res["hit"] == 1).sum()), boxes.mean(), boxes.max(), tris.mean(), tris.max(), ntri,
                                                         wave.max(axis=1).mean(), wave.max(axis=1).mean() / max(wave.mean(), 1e-9)))
    for name, h in (("one dragon", body), ("%d dragons" % a.bodies, batch)):
        s = torch.cuda.current_stream().cuda_stream
        ms = [event_ms(lambda: capi.check(L.tetsim_debug_bvh_refit(h._h, s), h._h), a.reps) for _ in range(a.runs)]
        say("the refit alone with the call's stream handshake, %s (ms per round): %s  median %.4f" % (name, " ".join("%.4f" % x for x in ms), median(ms)))


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--reps", type=int, default=20)
    ap.add_argument("--runs", type=int, default=5)
    ap.add_argument("--bodies", type=int, default=64)
    ap.add_argument("--out", default=None)
    ap.add_argument("--stats-child", action="store_true", help=argparse.SUPPRESS)
    a = ap.parse_args()
    if a.stats_child:
        stats_child(a)
        return
    say("library source_sha %s" % library_info()["source_sha"])
    body, ntri = one_dragon()
    c, r = raycast_ref.bounding_sphere(body.visualPositions())
    o, d = sphere_rays(c, r, 1024, 1)
    rays = rays_tensor(o, d)
    body.raycastVisualDevice(rays)                                                # (the brute-force call's tables exist: what follows is the tree's alone)
    torch.cuda.synchronize()
    d0, t0 = device_bytes(body), time.perf_counter()
    body.raycastVisualBvhDevice(rays)
    torch.cuda.synchronize()
    first = 1e3 * (time.perf_counter() - t0)
    t0 = time.perf_counter()
    body.raycastVisualBvhDevice(rays)
    torch.cuda.synchronize()
    again = 1e3 * (time.perf_counter() - t0)
    say("one dragon: the first call %.2f ms wall (it builds the topology on the host: skin, wait, read back, sort, upload), the second %.3f ms wall; "
        "the tree takes %d bytes = %.1f bytes per triangle" % (first, again, device_bytes(body) - d0, (device_bytes(body) - d0) / ntri))
    times = {}
    for n in (1024, 65536, 16):
        o, d = sphere_rays(c, r, n, 1)
        times[n] = compare("one dragon, %6d rays" % n, body, rays_tensor(o, d), None, a)
    body.close()
    nb, per = a.bodies, 1024
    batch = many_dragons(nb)
    o, d = sphere_rays(c, r, nb * per, 2)
    ids = np.repeat(np.arange(nb, dtype=np.int32), per)
    perm = np.random.default_rng(3).permutation(nb * per)
    t0 = time.perf_counter()
    batch.raycastVisualBvhDevice(rays_tensor(o[:16], d[:16]), torch.from_numpy(ids[:16].copy()).cuda())
    torch.cuda.synchronize()
    say("%d dragons: the first call %.1f ms wall" % (nb, 1e3 * (time.perf_counter() - t0)))
    for name, order in (("grouped by body", np.arange(nb * per)), ("shuffled", perm)):
        times[name] = compare("%d dragons, %d x %d rays, %s" % (nb, nb, per, name), batch, rays_tensor(o[order], d[order]),
                              torch.from_numpy(ids[order]).cuda(), a)
    say("the tree call, shuffled over grouped: %.2fx" % (times["shuffled"][0] / times["grouped by body"][0]))
    batch.close()
    if not os.path.exists(STATS_LIB):
        from tetsim_amd.build import build_variant
        build_variant("bvhstats", ["-DTETSIM_BVH_STATS"])
    env = dict(os.environ, TETSIM_HIP_LIB=STATS_LIB)
    child = subprocess.run([sys.executable, os.path.abspath(__file__), "--stats-child", "--reps", str(a.reps), "--runs", str(a.runs), "--bodies", str(a.bodies)],
                           env=env, capture_output=True, text=True, timeout=900)
    for line in child.stdout.splitlines():
        say(line)
    if child.returncode != 0:
        say("the statistics run failed (exit %d): %s" % (child.returncode, child.stderr[-2000:]))
    if a.out:
        with open(a.out, "w") as f:
            f.write("\n".join(LINES) + "\n")
    sys.exit(child.returncode)


if __name__ == "__main__":
    main()
