"""The bits of the per-body rows -- bodyObservations(), bodyPoses(), bodyStrainDevice(), nearestParticlesDevice() -- on a few seeded states,
recorded as hex strings: what tests/test_gpu_body_rows_golden.py holds every later build to.  The states are set with writeState (no
stepping, so no solver's bits enter) and the rows are computed from the rows in the caller's numbering, so every kind of body gives the
same bits: the tool records polar FAST and Neo-Hookean FAST and refuses to write a file if they differ.  The cases are the smallest
shapes at which a part of the reduction can go wrong:

    mixed    lat4, dragon, lat4 behind one handle: bodies below one chunk of 256, a body of several chunks with a ragged last one
    one-tet  a single tet, lattice(4), lattice(3): a chunk with one live lane (tets) and four (particles)
    lat23    73,002 tets in one body: 286 tet chunks, the finish kernels' strided fold wraps
    lat40    68,921 particles in one body: 270 particle chunks, likewise on the particle side

    python tools/record_body_rows.py [--out tests/golden/body_rows_bits.json]

Only the public Python API is used: the same file runs on the build that recorded the golden file and on every later one.
"""
import argparse
import json
import os
import sys

import numpy as np
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

from tetsim_amd import SoftBodyHIP, make_lattice  # noqa: E402
from tetsim_amd import _capi as capi  # noqa: E402

GOLDEN = os.path.join(ROOT, "tests", "golden", "body_rows_bits.json")
PP = dict(gravity=-9.81, friction=1000.0, density=1000.0, devCompliance=1e-5, volCompliance=0.0,
          worldBounds=[-10.0, -1.0, -10.0, 10.0, 10.0, 10.0])
KINDS = {"polar-fast": dict(solver="polar", precision="fast"), "nh-fast": dict(solver="neohookean", precision="fast", order="clustered")}
SHIFTS = [np.array(s, np.float32) for s in ([-3.0, 0.0, 0.0], [0.0, 0.0, 0.0], [3.0, 0.0, 0.5])]
ONE_TET = (np.array([[0, 0.5, 0], [0.5, 0.5, 0], [0, 1.0, 0], [0, 0.5, 0.5]], np.float32), np.array([[0, 1, 2, 3]], np.int32))
SEEDS = {"mixed": 11, "one-tet": 12, "lat23": 3, "lat40": 14, "points": 15}
CASES = ["mixed", "one-tet", "lat23", "lat40"]


def load_mesh(name):
    g = os.path.join(ROOT, "tests", "golden")
    return (np.fromfile(os.path.join(g, name + "_verts.f32"), dtype="<f4").reshape(-1, 3),
            np.fromfile(os.path.join(g, name + "_tets.i32"), dtype="<i4").reshape(-1, 4))


def shifted(parts):
    return [((v + s).astype(np.float32), t) for (v, t), s in zip(parts, SHIFTS)]


def case(name):
    """(parts, pos, vel, points): the bodies [(vertices, tets)], the seeded state of their concatenation, one seeded point per body"""
    rng = np.random.default_rng(SEEDS[name])
    if name == "mixed":        # tests/test_gpu_observe.py: parts_of("mixed")
        parts = shifted([load_mesh("lat4"), load_mesh("dragon"), load_mesh("lat4")])
    elif name == "one-tet":    # tests/test_gpu_strain.py: test_a_body_of_a_batch_gives_the_bits_it_gives_alone
        parts = shifted([ONE_TET, make_lattice(4), make_lattice(3)])
    else:
        parts = [make_lattice(23 if name == "lat23" else 40)]
    rest = np.concatenate([v for v, _ in parts])
    if name == "lat23":        # tests/test_gpu_crowd.py: lat23()
        pos = (rest + rng.normal(0.0, 0.03 / 23, rest.shape)).astype(np.float32)
    else:
        pos = (rest + rng.normal(0.0, 0.002, rest.shape)).astype(np.float32)
    vel = rng.normal(0.0, 1.5, rest.shape).astype(np.float32)
    prng = np.random.default_rng(SEEDS["points"])
    points = np.stack([v.mean(axis=0) + prng.normal(0.0, 0.2, 3) for v, _ in parts]).astype(np.float32)
    return parts, pos, vel, points


def make(parts, kind):
    if len(parts) == 1:
        return SoftBodyHIP(parts[0][0], parts[0][1], None, dict(PP), ref_fixed_bounds=False, **KINDS[kind])
    return SoftBodyHIP.batch(parts, dict(PP), ref_fixed_bounds=False, **KINDS[kind])


def hex_rows(a, dtype):
    """one string per row: the row's words as fixed-width hex, in order"""
    a = np.ascontiguousarray(a).reshape(len(a), -1)
    words = a.view({8: np.uint64, 4: np.uint32}[np.dtype(dtype).itemsize])
    fmt = "%016x" if words.dtype == np.uint64 else "%08x"
    return ["".join(fmt % int(w) for w in row) for row in words]


def rows_of(body, points):
    """{name: hex rows} of the four per-body calls in the body's present state"""
    ids, d2 = body.nearestParticlesDevice(torch.from_numpy(points).cuda())
    strain = body.bodyStrainDevice()
    torch.cuda.synchronize()
    return {"observations": hex_rows(body.bodyObservations(), np.float64), "poses": hex_rows(body.bodyPoses(), np.float64),
            "strain": hex_rows(strain.cpu().numpy(), np.float64), "nearest_ids": hex_rows(ids.cpu().numpy().astype(np.int32), np.int32),
            "nearest_dist2": hex_rows(d2.cpu().numpy(), np.float64)}


def record(name, kind):
    parts, pos, vel, points = case(name)
    body = make(parts, kind)
    body.writeState(pos, vel)
    assert np.array_equal(body.pos.view(np.uint32), pos.view(np.uint32)) and np.array_equal(body.vel.view(np.uint32), vel.view(np.uint32))
    out = rows_of(body, points)
    body.close()
    return out


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--out", default=GOLDEN)
    a = ap.parse_args()
    cases = {}
    for name in CASES:
        got = {kind: record(name, kind) for kind in KINDS}
        first = got[list(KINDS)[0]]
        for kind, rows in got.items():
            bad = [k for k in first if rows[k] != first[k]]
            if bad:
                sys.exit("%s: %s gives other bits than %s in %s -- record per kind" % (name, kind, list(KINDS)[0], bad))
        cases[name] = first
        print("%s: %d bodies, both kinds agree" % (name, len(first["poses"])))
    widths = {"observations": capi.OBS_WIDTH, "poses": capi.POSE_WIDTH, "strain": capi.STRAIN_BODY_WIDTH}
    doc = {"source_sha": capi.library_info()["source_sha"], "kinds": list(KINDS), "seeds": SEEDS, "widths": widths, "cases": cases}
    with open(a.out, "w") as f:
        json.dump(doc, f, indent=1, sort_keys=True)
        f.write("\n")
    print("wrote %s (library %s)" % (a.out, doc["source_sha"]))


if __name__ == "__main__":
    main()
