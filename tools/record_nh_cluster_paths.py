"""The bits of the four-lane Neo-Hookean cluster kernels (nh_kernels.inc) on every path that executes a cluster, recorded as hex strings: what
tests/test_gpu_nh_cluster_paths_golden.py holds every later build to.  solver="neohookean", order="clustered"; a seeded state (writeState),
one sphere collider and one grab, 25 substeps in calls of 7, 6 and 12, then one more through tetsim_step (simulate).

    paths    colour   FAST, one launch per colour (TETSIM_NH_ONE_LAUNCH=0): nh_cluster4_kernel_fast, first sweep of a call without
                      the folded particle pass, the others with it
             sweep    FAST, every substep a call of its own (simulate): nh_sweep1_kernel<false>, one launch per substep
             call     FAST, simulateSubsteps: nh_call_kernel, one launch per call -- on the mesh with free particles the body keeps
                      the sweep, nh_sweep1_kernel<false> then <true> x (n - 1) inside one graph
             precise  PRECISE, simulateSubsteps: nh_cluster4_kernel_precise per colour; nh_cluster_kernel_precise (one lane per
                      cluster) for the colours of more than 2,048 clusters, which lat30's are
    meshes   lat5     750 tets: full and ragged clusters, every particle touched
             ragged   a Delaunay body (tests/test_gpu_random_meshes.py: random_mesh(2, 400)): clusters of fewer than 8 tets and fewer
                      than 8 particles -- the `i < L.count[j]` guard and the empty slots
             free     the same body and three particles no tet references: the untouched list of the particle pass, no call kernel
             lat30    162,000 tets, 8 colours of more than 2,048 clusters each (asserted from levelOffsets)

The three FAST paths promise each other's bits, so ONE entry per (mesh, precision) is kept and the tool refuses to write a file if two of
them differ.  Every wait of the one-launch kernels is bounded: a wait that gave up makes tetsim_sync fail and the body fall back to one
launch per colour, whose bits are the same -- so every call is followed by sync(), which must succeed.  lat30 is kept as SHA-256 of the
arrays' bytes (a committed file stays under 1 MiB), the others as hex rows.

    python tools/record_nh_cluster_paths.py [--out tests/golden/nh_cluster_paths_bits.json]

Only the public Python API is used: the same file runs on the build that recorded the golden file and on every later one.
"""
import argparse
import hashlib
import importlib.util
import json
import os
import struct
import sys

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

GOLDEN = os.path.join(ROOT, "tests", "golden", "nh_cluster_paths_bits.json")
PP = dict(gravity=-9.81, friction=1000.0, density=1000.0, devCompliance=1e-5, volCompliance=0.0,
          worldBounds=[-2.5, -1.0, -2.5, 2.5, 10.0, 2.5])
DT = (1.0 / 60.0) / 20
CALLS = (7, 6, 12)
MESHES = ["lat5", "ragged", "free", "lat30"]
SEEDS = {"lat5": 31, "ragged": 32, "free": 33, "lat30": 34}
PATHS = {"colour": "fast", "sweep": "fast", "call": "fast", "precise": "precise"}   # path -> the precision whose entry it must equal
FREE = [[0.1, 2.0, 0.1], [-0.3, 1.2, 0.2], [0.25, 0.9, -0.3]]   # particles no tet references
WHAT = ("pos", "vel", "prevPos", "volError")
ONE_LANE_CLUSTERS = 2048   # nh_launch_cluster_precise: more clusters than this in a launch take one lane per cluster
CLUSTER_TETS = 8           # a cluster holds at most this many tets
HEX_ROWS_MAX = 2048        # longer arrays are kept as a digest


def _random_mesh(seed, npts):
    tests = os.path.join(ROOT, "tests")
    if tests not in sys.path:
        sys.path.insert(0, tests)
    spec = importlib.util.spec_from_file_location("test_gpu_random_meshes", os.path.join(tests, "test_gpu_random_meshes.py"))
    mod = importlib.util.module_from_spec(spec)
    spec.loader.exec_module(mod)
    return mod.random_mesh(seed, npts)


def mesh(name):
    from tetsim_amd import make_lattice
    if name == "lat5":
        return make_lattice(5, y0=0.02)
    if name == "lat30":
        return make_lattice(30, y0=0.02)
    v, t = _random_mesh(2, 400)
    if name == "free":
        v = np.concatenate([v, FREE]).astype(np.float32)
    return v, t


_CASES = {}


def case(name):
    """(vertices, tets, pos, vel, collider, grab id, grab target): the mesh, its seeded state, a sphere that cuts into it, a held particle"""
    if name not in _CASES:
        v, t = mesh(name)
        rng = np.random.default_rng(SEEDS[name])
        size = float((v.max(axis=0) - v.min(axis=0)).max())
        pos = (v + rng.normal(0.0, 0.002 * size, v.shape)).astype(np.float32)
        vel = rng.normal(0.0, 0.5, v.shape).astype(np.float32)
        tv = v[np.unique(t)]   # (the sphere and the grab sit at the tets, wherever the free particles are)
        sphere = dict(kind="sphere", a=[float(x) for x in tv.max(axis=0)], radius=0.45 * float((tv.max(axis=0) - tv.min(axis=0)).max()), friction=0.5)
        gid = int(np.unique(t)[np.unique(t).size // 2])
        target = (v[gid] + np.float32([0.03, 0.05, -0.02]) * size).astype(np.float32)
        _CASES[name] = (v, t, pos, vel, sphere, gid, target)
    return _CASES[name]


def encode(a):
    """hex rows (one string per row, the row's words in order), or the digest of a long array's bytes"""
    a = np.ascontiguousarray(a, dtype=np.float32)
    a = a.reshape(len(a), -1)
    if len(a) > HEX_ROWS_MAX:
        return {"rows": len(a), "sha256": hashlib.sha256(a.astype("<f4").tobytes()).hexdigest()}
    return ["".join("%08x" % int(w) for w in row) for row in a.view(np.uint32)]


def record(name, path):
    """{pos, vel, prevPos, volError}: the encoded state after the calls on `path`"""
    from tetsim_amd import SoftBodyHIP
    v, t, pos, vel, sphere, gid, target = case(name)
    if path == "colour":
        os.environ["TETSIM_NH_ONE_LAUNCH"] = "0"   # (read at every creation)
    try:
        body = SoftBodyHIP(v, t, None, dict(PP), solver="neohookean", precision=PATHS[path], order="clustered")
    finally:
        if path == "colour":
            del os.environ["TETSIM_NH_ONE_LAUNCH"]
    # What makes a clustered FAST body take the one-launch kernels (tetsim_create.hip): 2..255 colours for nh_sweep1_kernel, and for
    # nh_call_kernel at most 127 colours and no particle that no tet references.  TetSimInfo does not say which path a body took, so
    # the conditions are asserted here: the three meshes without free particles are call-kernel bodies, `free` is a sweep body.
    levels, loose = body.info.num_levels, len(v) - int(np.unique(t).size)
    assert 2 <= levels <= 127 and loose == (len(FREE) if name == "free" else 0), (name, levels, loose)
    if name == "lat30":
        widest = int(np.diff(body.levelOffsets).max())
        assert widest > CLUSTER_TETS * ONE_LANE_CLUSTERS, (name, widest)   # (so its colour has more than 2,048 clusters)
    body.writeState(pos, vel)
    body.setColliders([sphere])
    body.setGrab(gid, target)
    for n in CALLS:
        if path == "sweep":
            for _ in range(n):
                body.simulate(DT, PP)
        else:
            body.simulateSubsteps(n, DT, PP)
        body.sync()   # (raises if a cluster waited in vain: the fall-back's bits are not accepted in the one-launch paths' place)
    body.simulate(DT, PP)
    body.sync()
    out = {"pos": encode(body.pos), "vel": encode(body.vel), "prevPos": encode(body.prevPos), "volError": struct.pack(">d", body.volError).hex()}
    body.close()
    return out


def record_all():
    """{path: {mesh: entry}} of all four paths"""
    return {p: {name: record(name, p) for name in MESHES} for p in PATHS}


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--out", default=GOLDEN)
    a = ap.parse_args()
    from tetsim_amd import _capi as capi
    got = record_all()
    cases = {}
    for name in MESHES:
        cases[name] = {}
        for p, precision in PATHS.items():
            first = cases[name].setdefault(precision, got[p][name])
            bad = [k for k in WHAT if got[p][name][k] != first[k]]
            if bad:
                sys.exit("%s: %s gives other bits than the first %s path in %s" % (name, p, precision, bad))
        print("%s: %d paths agree" % (name, len(PATHS)))
    doc = {"source_sha": capi.library_info()["source_sha"], "paths": PATHS, "calls": list(CALLS), "seeds": SEEDS, "cases": cases}
    with open(a.out, "w") as f:
        json.dump(doc, f, indent=1, sort_keys=True)
        f.write("\n")
    print("wrote %s (library %s)" % (a.out, doc["source_sha"]))


if __name__ == "__main__":
    main()
