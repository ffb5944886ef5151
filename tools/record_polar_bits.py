"""The bits of the blocked polar solve (FAST) after 40 substeps on a few small bodies, recorded as float32 .npy files under
tests/golden/polar_bits/: what tests/test_gpu_tile_tables.py holds every later build to.  The tile tables of the blocked kernels
(host_prep.cpp: build_blocks) decide the ORDER in which a tile adds up its corner goals; a change of their layout must leave every
result bit for bit where it was.  The bodies are the smallest at which the tiles' reduction can go wrong:

    irregular  a Delaunay mesh of 700 points, 4,375 tets in 18 tiles: a last tile of 23 tets over 17 particles (ntb < 256, nu < 64),
               runs of every length mod 4 and of up to 37 entries, valences of up to 54 (the reference's 36-slot table drops the rest:
               corners without a place in the reduction).  It takes the persistent frame kernel of 256-tet tiles (tetsim_step_n,
               path 2 -- not the four-lane kernels of small bodies) and the fused kernel (tetsim_step)
    loose      the same mesh and a particle no tet references: the body keeps the kernel pair (tetsim_step) and runs a call as one
               launch (tetsim_step_n: pjb_call_kernel) at any size
    lattice    45 cells, 546,750 tets in 2,136 tiles: the smallest lattice that takes the one-launch call by its size, a last tile of
               190 tets, particles on the lists of 9 tiles

each with the carried record, TETSIM_FLAG_LEAN_STATE and TETSIM_FLAG_CONSTANT_REST_SHAPE.  Arrays of more than 1,024 rows keep a
fixed seeded sample of 1,024 rows in ascending order (positions, velocities, and the quaternions in the caller's tet order).

    python tools/record_polar_bits.py [--out tests/golden/polar_bits]

Only the public Python API is used: the same file runs on the build that recorded the files and on every later one.
"""
import argparse
import os
import sys

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

from tetsim_amd import SoftBodyHIP, make_lattice  # noqa: E402
from tetsim_amd import _capi as capi  # noqa: E402

GOLDEN = os.path.join(ROOT, "tests", "golden", "polar_bits")
PP = dict(gravity=-9.81, friction=1000.0, density=1000.0, devCompliance=1e-5, volCompliance=0.0,
          worldBounds=[-2.5, -1.0, -2.5, 2.5, 10.0, 2.5])
DT = (1.0 / 60.0) / 20
SUBSTEPS = 40
CALLS = (13, 1, 26)            # tetsim_step_n: a call's first substep and its later ones, a call of one substep
ROWS = 1024
CASES = ["irregular", "loose", "lattice"]
FLAGS = {"carried": dict(), "lean": dict(lean_state=True), "constant": dict(constant_rest_shape=True)}
FIELDS = ["pos", "vel", "quats"]
LOOSE = [0.1, 2.0, 0.1]
LATTICE_CELLS = 45


def delaunay_mesh(seed, npts, min_vol=2e-6):
    """tests/test_gpu_random_meshes.py: random_mesh -- seeded points in a box, their Delaunay tets with positive volume, slivers dropped"""
    from scipy.spatial import Delaunay
    rng = np.random.default_rng(seed)
    pts = (rng.random((npts, 3)) * [0.8, 0.6, 0.7] + [-0.4, 0.15, -0.35]).astype(np.float32)
    tets = Delaunay(pts.astype(np.float64)).simplices.astype(np.int32)
    d = pts[tets[:, 1:]].astype(np.float64) - pts[tets[:, :1]].astype(np.float64)
    vol = np.linalg.det(d) / 6.0
    flip = vol < 0
    tets[flip] = tets[flip][:, [0, 1, 3, 2]]
    tets = tets[np.abs(vol) > min_vol]
    used = np.unique(tets)
    remap = np.full(npts, -1, dtype=np.int32)
    remap[used] = np.arange(len(used), dtype=np.int32)
    return np.ascontiguousarray(pts[used]), np.ascontiguousarray(remap[tets])


def mesh(case):
    if case == "lattice":
        return make_lattice(LATTICE_CELLS, y0=0.004)
    v, t = delaunay_mesh(52, 700)
    v = v.copy()
    v[:, 1] -= v[:, 1].min() - np.float32(0.004)          # 4 mm above the floor: contact within the 40 substeps
    if case == "loose":
        v = np.concatenate([v, [LOOSE]]).astype(np.float32)
    return v, t


def sample(a):
    a = np.ascontiguousarray(a, dtype=np.float32)
    if len(a) > ROWS:
        a = a[np.sort(np.random.RandomState(12345).choice(len(a), ROWS, replace=False))]
    return a


def run(case, flag, stepper="step_n", one_launch=True):
    """{field: rows} after SUBSTEPS substeps -- stepper "step_n": calls of CALLS substeps, "step": one tetsim_step each; the whole arrays
    (the loose particle's row left out: 0 / 0, no evidence), quaternions in the caller's tet order; and the body's path"""
    v, t = mesh(case)
    if not one_launch:
        os.environ["TETSIM_PJ_ONE_LAUNCH"] = "0"
    try:
        body = SoftBodyHIP(v, t, None, dict(PP), solver="polar", precision="fast", **FLAGS[flag])
    finally:
        os.environ.pop("TETSIM_PJ_ONE_LAUNCH", None)
    if stepper == "step_n":
        for n in CALLS:
            body.simulateSubsteps(n, DT, PP)
    else:
        for _ in range(SUBSTEPS):
            body.simulate(DT, PP)
    rows = len(v) - (1 if case == "loose" else 0)
    quats = np.zeros((len(t), 4), dtype=np.float32)
    quats[body.localTets] = body.quats
    out = {"pos": body.pos.reshape(-1, 3)[:rows].copy(), "vel": body.vel.reshape(-1, 3)[:rows].copy(), "quats": quats}
    path = int(body.info.fused_particle_pass)
    body.close()
    return out, path


def path_of(name):
    return os.path.join(GOLDEN, name + ".npy")


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--out", default=GOLDEN)
    a = ap.parse_args()
    assert sum(CALLS) == SUBSTEPS
    os.makedirs(a.out, exist_ok=True)
    total = 0
    for case in CASES:
        for flag in FLAGS:
            got, path = run(case, flag)
            assert all(np.isfinite(x).all() for x in got.values()), (case, flag)
            for field in FIELDS:
                f = os.path.join(a.out, "%s_%s_%s.npy" % (case, flag, field))
                np.save(f, sample(got[field]))
                total += os.path.getsize(f)
            print("%s %s: path %d, %d particles, %d tets, min y %.6f" % (case, flag, path, len(got["pos"]), len(got["quats"]), got["pos"][:, 1].min()))
    with open(os.path.join(a.out, "SOURCE"), "w") as f:
        f.write("recorded by tools/record_polar_bits.py from the library with source_sha %s\n" % capi.library_info()["source_sha"])
    print("wrote %d bytes under %s (library %s)" % (total, a.out, capi.library_info()["source_sha"]))


if __name__ == "__main__":
    main()
