"""The bits of the blocked polar kernels (pj_blocked.hip) on every unpartitioned path, recorded as hex strings: what
tests/test_gpu_blocked_paths_golden.py holds every later build to.  FAST precision; a seeded state (writeState), one sphere collider and one
grab, then 25 substeps in calls of 7, 6 and 12 (odd and even counts: the frame kernel's buffers alternate by parity).

    records  default | TETSIM_FLAG_CONSTANT_REST_SHAPE | TETSIM_FLAG_LEAN_STATE
    paths    pair    the tet kernel and the particle kernel per substep   (TETSIM_FUSED_PARTICLE_PASS=0, TETSIM_PJ_ONE_LAUNCH=0)
             call    a call as one launch, pjb_call_kernel                 (TETSIM_FUSED_PARTICLE_PASS=0)
             fused   the particle update fused into the tiles' staging     (tetsim_profile: tet | fused x (n - 1) | particle)
             frame   the persistent frame kernel, one launch per call      (tetsim_step_n of a body whose tiles are all resident)
             all with TETSIM_QUAD=0: 256-tet tiles also for the bodies that would take the four-lane kernels
    meshes   lat5    750 tets, 3 tiles: particles shared between tiles, runs of 1..24 entries (not multiples of four)
             hub     the committed Delaunay ball, 2 tiles: valence 44, so the incidence table DROPS corners (the +0 entries of the scatter)
             wheel   2,400 tets around one axis, 10 tiles: the axis particles are on ten tiles' lists -- the entry-by-entry tail behind the
                     eight-and-a-ninth gather of the fused and frame kernels (the hub, at two tiles, does not get there)
             lat16   24,576 tets, 96 tiles: too many for one XCD's share of resident workgroups, so the frame kernel takes the any-XCD
                     placement (memory-side exchange) where the three above take the one-XCD placement if the device has it

The four paths promise each other's bits, so ONE entry per (mesh, record) is kept and the tool refuses to write a file if two paths differ.
The two large meshes are kept as SHA-256 of the arrays' bytes (a committed file stays under 1 MiB), the two small ones as hex rows.
The switches are read once per process (tetsim_create.hip), so each pair of paths is recorded in a child process of its own.

    python tools/record_blocked_paths.py [--out tests/golden/blocked_paths_bits.json]

Only the public Python API is used: the same file runs on the build that recorded the golden file and on every later one.
"""
import argparse
import hashlib
import json
import os
import subprocess
import sys

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

GOLDEN = os.path.join(ROOT, "tests", "golden", "blocked_paths_bits.json")
PP = dict(gravity=-9.81, friction=1000.0, density=1000.0, devCompliance=1e-5, volCompliance=0.0,
          worldBounds=[-2.5, -1.0, -2.5, 2.5, 10.0, 2.5])
DT = (1.0 / 60.0) / 20
CALLS = (7, 6, 12)
MODES = {"default": dict(), "constant-rest": dict(constant_rest_shape=True), "lean-state": dict(lean_state=True)}
MESHES = ["lat5", "hub", "wheel", "lat16"]
SEEDS = {"lat5": 21, "hub": 22, "wheel": 23, "lat16": 24}
# the child processes: their switches, and the two paths each records
PROCESSES = {"two-kernel": (dict(TETSIM_QUAD="0", TETSIM_FUSED_PARTICLE_PASS="0"), ("pair", "call")),
             "fused": (dict(TETSIM_QUAD="0"), ("fused", "frame"))}
PATHS = [p for _, paths in PROCESSES.values() for p in paths]
PATH_CODE = {"pair": 0, "call": 5, "fused": 2, "frame": 2}   # TetSimInfo::fused_particle_pass (fused: the same body as frame, stepped by tetsim_profile)
HEX_ROWS_MAX = 2048   # longer arrays are kept as a digest


def mesh(name):
    from tetsim_amd import make_lattice
    if name == "lat5":
        return make_lattice(5, y0=0.02)
    if name == "lat16":
        return make_lattice(16, y0=0.02)
    if name == "hub":
        g = os.path.join(ROOT, "tests", "golden")
        return (np.fromfile(os.path.join(g, "hub_verts.f32"), dtype="<f4").reshape(-1, 3), np.fromfile(os.path.join(g, "hub_tets.i32"), dtype="<i4").reshape(-1, 4))
    spokes = 2400     # tests/test_gpu_frame_kernel.py: _wheel
    ang = np.linspace(0.0, 2.0 * np.pi, spokes, endpoint=False)
    ring = np.stack([0.5 * np.cos(ang), np.full(spokes, 1.0), 0.5 * np.sin(ang)], axis=1)
    v = np.concatenate([[[0.0, 1.3, 0.0], [0.0, 0.7, 0.0]], ring]).astype(np.float32)
    i = np.arange(spokes)
    return v, np.stack([np.zeros(spokes, int), np.ones(spokes, int), 2 + i, 2 + (i + 1) % spokes], axis=1).astype(np.int32)


def case(name):
    """(vertices, tets, pos, vel, collider, grab id, grab target): the mesh, its seeded state, a sphere that cuts into it, a held particle"""
    v, t = mesh(name)
    rng = np.random.default_rng(SEEDS[name])
    size = float((v.max(axis=0) - v.min(axis=0)).max())
    pos = (v + rng.normal(0.0, 0.002 * size, v.shape)).astype(np.float32)
    vel = rng.normal(0.0, 0.5, v.shape).astype(np.float32)
    sphere = dict(kind="sphere", a=[float(x) for x in v.max(axis=0)], radius=0.45 * size, friction=0.5)
    gid = len(v) // 2
    target = (v[gid] + np.float32([0.03, 0.05, -0.02]) * size).astype(np.float32)
    return v, t, pos, vel, sphere, gid, target


def encode(a):
    """hex rows (one string per row, the row's words in order), or the digest of a long array's bytes"""
    a = np.ascontiguousarray(a, dtype=np.float32)
    a = a.reshape(len(a), -1)
    if len(a) > HEX_ROWS_MAX:
        return {"rows": len(a), "sha256": hashlib.sha256(a.astype("<f4").tobytes()).hexdigest()}
    return ["".join("%08x" % int(w) for w in row) for row in a.view(np.uint32)]


def record(name, mode, path):
    """{pos, vel, quats, info}: the encoded state after the calls on `path` -- which must be one of THIS process's paths"""
    from tetsim_amd import SoftBodyHIP
    v, t, pos, vel, sphere, gid, target = case(name)
    pair = path == "pair"
    if pair:
        os.environ["TETSIM_PJ_ONE_LAUNCH"] = "0"   # (read at every creation)
    try:
        body = SoftBodyHIP(v, t, None, dict(PP), solver="polar", precision="fast", ref_slot_table=name != "wheel", **MODES[mode])
    finally:
        if pair:
            del os.environ["TETSIM_PJ_ONE_LAUNCH"]
    body.writeState(pos, vel)
    body.setColliders([sphere])
    body.setGrab(gid, target)
    for n in CALLS:
        if path == "fused":
            pr = body.profile(n, DT, PP)
            assert pr["substeps"] == n
        else:
            body.simulateSubsteps(n, DT, PP)
    body.sync()
    out = {"pos": encode(body.pos), "vel": encode(body.vel), "quats": encode(body.quats), "info": int(body.info.fused_particle_pass)}
    body.close()
    return out


def record_process(paths):
    """every (mesh, record) on the given paths of this process: {path: {mesh: {record: entry}}}"""
    return {p: {name: {mode: record(name, mode, p) for mode in MODES} for name in MESHES} for p in paths}


def record_all():
    """{path: {mesh: {record: entry}}} of all four paths, each pair of paths in a fresh process with its switches"""
    out = {}
    for key, (env, paths) in PROCESSES.items():
        keep = {k: v for k, v in os.environ.items() if k not in ("TETSIM_QUAD", "TETSIM_FUSED_PARTICLE_PASS", "TETSIM_PJ_ONE_LAUNCH", "TETSIM_FRAME_KERNEL")}
        r = subprocess.run([sys.executable, os.path.abspath(__file__), "--child", key], env=dict(keep, **env), capture_output=True, text=True, timeout=600)
        if r.returncode != 0:
            raise RuntimeError("recording the %s paths failed:\n%s" % (key, r.stderr[-3000:]))
        out.update(json.loads(r.stdout.splitlines()[-1]))
    return out


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--out", default=GOLDEN)
    ap.add_argument("--child", choices=list(PROCESSES))
    a = ap.parse_args()
    if a.child:
        print(json.dumps(record_process(PROCESSES[a.child][1])))
        return
    from tetsim_amd import _capi as capi
    got = record_all()
    cases = {}
    for name in MESHES:
        cases[name] = {}
        for mode in MODES:
            first = got[PATHS[0]][name][mode]
            for p in PATHS:
                e = got[p][name][mode]
                if e["info"] != PATH_CODE[p]:
                    sys.exit("%s / %s: the %s path reports %d, not %d" % (name, mode, p, e["info"], PATH_CODE[p]))
                bad = [k for k in ("pos", "vel", "quats") if e[k] != first[k]]
                if bad:
                    sys.exit("%s / %s: %s gives other bits than %s in %s" % (name, mode, p, PATHS[0], bad))
            cases[name][mode] = {k: first[k] for k in ("pos", "vel", "quats")}
        print("%s: %d records x %d paths agree" % (name, len(MODES), len(PATHS)))
    doc = {"source_sha": capi.library_info()["source_sha"], "modes": list(MODES), "paths": PATHS, "calls": list(CALLS), "seeds": SEEDS, "cases": cases}
    with open(a.out, "w") as f:
        json.dump(doc, f, indent=1, sort_keys=True)
        f.write("\n")
    print("wrote %s (library %s)" % (a.out, doc["source_sha"]))


if __name__ == "__main__":
    main()
