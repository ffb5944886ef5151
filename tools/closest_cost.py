"""What a closest-point call through the refitted tree costs (tetsim_closest_visual_device) beside the ray cast through the same tree
(tetsim_raycast_visual_bvh_device: unchanged code) for the same number of rays, in the same build and session: `--bodies` Dragons in one
batch (59,657 triangles each), 1,024 queries per body scattered within one bounding radius of that body's surface, shuffled over the
bodies, no max_distance.  Time between HIP events on the caller's stream, median of `--reps` calls after warm-up; the two calls alternate,
`--runs` rounds; the ray call's own spread over its rounds is the allowance of any comparison.  Also, in a child process on a development
build of the library (-DTETSIM_BVH_STATS: libtetsim_hip_bvhstats.so, built here if it is missing): the refit alone with the call's stream
handshake, hence its share of the call, and the boxes and triangles tested per query.
    python tools/closest_cost.py [--reps 20] [--runs 5] [--bodies 64] [--out profiles/closest_cost.txt]"""
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

import closest_ref  # noqa: E402
import raycast_ref  # noqa: E402
from raycast_bvh_cost import STATS_LIB, LINES, device_bytes, event_ms, many_dragons, say  # noqa: E402
from raycast_device_cost import median, sphere_rays  # noqa: E402
from tetsim_amd import library_info, point_queries_tensor, rays_tensor  # noqa: E402
from tetsim_amd import _capi as capi  # noqa: E402

PER_BODY = 1024


def workload(batch, nb):
    """(queries, rays, bodies) on the device: per body PER_BODY points around its own surface and as many rays at its sphere, shuffled"""
    pos = batch.visualPositions().reshape(nb, -1, 3)
    points, o, d = [], [], []
    for k in range(nb):
        pk, _ = closest_ref.seeded_points(pos[k], PER_BODY, 300 + k)
        c, r = raycast_ref.bounding_sphere(pos[k])
        ok, dk = sphere_rays(c, r, PER_BODY, 400 + k)
        points.append(pk), o.append(ok), d.append(dk)
    ids = np.repeat(np.arange(nb, dtype=np.int32), PER_BODY)
    perm = np.random.default_rng(5).permutation(nb * PER_BODY)
    return (point_queries_tensor(np.concatenate(points)[perm]), rays_tensor(np.concatenate(o)[perm], np.concatenate(d)[perm]),
            torch.from_numpy(ids[perm]).cuda())


def stats_child(a):
    """in a process of its own, on the development build: the refit alone and what the traversal tests"""
    L = capi.lib()
    L.tetsim_debug_bvh_stats.argtypes = [C.c_void_p, C.c_void_p]
    L.tetsim_debug_bvh_refit.argtypes = [C.c_void_p, C.c_void_p]
    batch = many_dragons(a.bodies)
    queries, rays, bodies = workload(batch, a.bodies)
    ntri = 59657
    stats = torch.zeros((len(queries), 2), dtype=torch.int32, device="cuda")
    capi.check(L.tetsim_debug_bvh_stats(batch._h, stats.data_ptr()), batch._h)
    res = batch.closestPointsDevice(queries, bodies)
    torch.cuda.synchronize()
    capi.check(L.tetsim_debug_bvh_stats(batch._h, None), batch._h)
    s = stats.cpu().numpy().astype(np.int64)
    boxes, tris = s[:, 0], s[:, 1]
    wave = boxes.reshape(-1, 64)
    say("%d dragons, %d queries: found %d; per query boxes tested mean %.1f max %d, triangles tested mean %.1f max %d (of %d); per wave of 64 queries the "
        "slowest lane's boxes mean %.1f, %.2fx the wave's mean lane" % (a.bodies, len(queries), int((res["found"] == 1).sum()), boxes.mean(), boxes.max(),
                                                                      tris.mean(), tris.max(), ntri, wave.max(axis=1).mean(), wave.max(axis=1).mean() / max(wave.mean(), 1e-9)))
    st = torch.cuda.current_stream().cuda_stream
    ms = [event_ms(lambda: capi.check(L.tetsim_debug_bvh_refit(batch._h, st), batch._h), a.reps) for _ in range(a.runs)]
    say("the refit alone with the call's stream handshake, %d dragons (ms per round): %s  median %.4f" % (a.bodies, " ".join("%.4f" % x for x in ms), median(ms)))
    print("REFIT_MS %.6f" % median(ms), flush=True)


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
    nb = a.bodies
    batch = many_dragons(nb)
    queries, rays, bodies = workload(batch, nb)
    d0, t0 = device_bytes(batch), time.perf_counter()
    batch.closestPointsDevice(queries[:16], bodies[:16].contiguous())
    torch.cuda.synchronize()
    say("%d dragons: the first call %.1f ms wall (it builds the topology on the host), %d bytes of tables and tree" %
        (nb, 1e3 * (time.perf_counter() - t0), device_bytes(batch) - d0))
    d1 = device_bytes(batch)
    closest, cast = [], []
    for _ in range(a.runs):
        closest.append(event_ms(lambda: batch.closestPointsDevice(queries, bodies), a.reps))
        cast.append(event_ms(lambda: batch.raycastVisualBvhDevice(rays, bodies), a.reps))
    res = batch.closestPointsDevice(queries, bodies)
    torch.cuda.synchronize()
    fmt = lambda xs: " ".join("%.3f" % x for x in xs)  # noqa: E731
    say("%d dragons, %d x %d shuffled (ms per call, per round): closest point %s  median %.3f | ray cast through the tree %s  median %.3f  spread %.3f | "
        "closest / ray %.2fx; found %d of %d; device_bytes moved by %d" %
        (nb, nb, PER_BODY, fmt(closest), median(closest), fmt(cast), median(cast), max(cast) - min(cast), median(closest) / median(cast),
         int((res["found"] == 1).sum()), len(queries), device_bytes(batch) - d1))
    batch.close()
    if not os.path.exists(STATS_LIB):
        from tetsim_amd.build import build_variant
        build_variant("bvhstats", ["-DTETSIM_BVH_STATS"])
    env = dict(os.environ, TETSIM_HIP_LIB=STATS_LIB)
    child = subprocess.run([sys.executable, os.path.abspath(__file__), "--stats-child", "--reps", str(a.reps), "--runs", str(a.runs), "--bodies", str(a.bodies)],
                           env=env, capture_output=True, text=True, timeout=900)
    for line in child.stdout.splitlines():
        if line.startswith("REFIT_MS "):
            refit = float(line.split()[1])
            say("the refit's share of a closest-point call: %.4f of %.3f ms = %.1f %%" % (refit, median(closest), 100.0 * refit / median(closest)))
        else:
            say(line)
    if child.returncode != 0:
        say("the statistics run failed (exit %d): %s" % (child.returncode, child.stderr[-2000:]))
    if a.out:
        with open(a.out, "w") as f:
            f.write("\n".join(LINES) + "\n")
    sys.exit(child.returncode)


if __name__ == "__main__":
    main()
