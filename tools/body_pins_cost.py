"""What body pins cost when they are ON: 64 Dragons in one batch, one call of 20 substeps (timeSubsteps), 1, 16 and 256 pins per body
against none held -- median of 20 calls after 5 warm-up calls, polar FAST and Neo-Hookean FAST, and one body of the persistent 256-tet
frame kernel (a 28-cell lattice), which steps through its fused kernels while pins are on.  Prints one line per case with the ratio.
With --parent-lib, first the cost of pins never switched on: `python bench.py`, three runs on the parent commit's library and three on
this one, alternating, each in a process of its own, and whether this commit's runs lie inside the parent's own spread.

    python tools/body_pins_cost.py [--bodies 64] [--parent-lib libtetsim_hip_parent.so] [--out profiles/body_pins_cost.txt]
"""
import argparse
import os
import json
import statistics
import subprocess
import sys

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

from tetsim_amd import SoftBodyHIP  # noqa: E402

PP = dict(gravity=-9.81, friction=1000.0, density=1000.0, devCompliance=1e-5, volCompliance=0.0,
          worldBounds=[-2.5, -1.0, -2.5, 2.5, 10.0, 2.5])
DT = (1.0 / 60.0) / 20
SUB, WARM, CALLS = 20, 5, 20
PINS = (1, 16, 256)


def dragon(y0):
    gold = os.path.join(ROOT, "tests", "golden")
    v = np.fromfile(os.path.join(gold, "dragon_verts.f32"), dtype="<f4").reshape(-1, 3).copy()
    t = np.fromfile(os.path.join(gold, "dragon_tets.i32"), dtype="<i4").reshape(-1, 4)
    v[:, 1] += np.float32(y0) - v[:, 1].min()
    return v, t


def median_ms(body):
    for _ in range(WARM):
        body.timeSubsteps(SUB, DT, PP)
    return statistics.median(body.timeSubsteps(SUB, DT, PP) for _ in range(CALLS))


def bench_value(lib):
    """the headline figure of one `python bench.py`, with `lib` (None: this tree's) as the library"""
    env = dict(os.environ)
    env.pop("TETSIM_HIP_LIB", None)
    if lib:
        env["TETSIM_HIP_LIB"] = os.path.abspath(lib)
    r = subprocess.run([sys.executable, os.path.join(ROOT, "bench.py")], env=env, capture_output=True, text=True, timeout=300)
    if r.returncode != 0:
        raise RuntimeError("bench.py failed:\n" + r.stderr[-2000:])
    out = json.loads(r.stdout.strip().splitlines()[-1])
    return float(out["value"]), out.get("unit", "")


def never_on(parent_lib):
    runs = {"parent": [], "this": []}
    unit = ""
    for _ in range(3):
        for name, lib in (("parent", parent_lib), ("this", None)):
            value, unit = bench_value(lib)
            runs[name].append(value)
            print("bench.py", name, value, unit, flush=True)
    lo, hi = min(runs["parent"]), max(runs["parent"])
    below, above = sum(x < lo for x in runs["this"]), sum(x > hi for x in runs["this"])
    verdict = "every run inside the parent's spread" if below + above == 0 else "%d run(s) below the parent's lowest, %d above its highest" % (below, above)
    fmt = lambda xs: ", ".join("%.4f" % x for x in xs)
    return ["pins never switched on, python bench.py (%s), alternating: parent %s; this commit %s" % (unit, fmt(runs["parent"]), fmt(runs["this"])),
            "    parent's spread %.4f-%.4f (median %.4f), this commit's median %.4f: %s" % (lo, hi, statistics.median(runs["parent"]), statistics.median(runs["this"]),
                                                                                          verdict)]


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--bodies", type=int, default=64)
    ap.add_argument("--out", default=None)
    ap.add_argument("--parent-lib", default=None)
    a = ap.parse_args()
    lines = never_on(a.parent_lib) if a.parent_lib else []
    meshes = [dragon(0.3)] * a.bodies
    v = meshes[0][0]
    for name, kw in (("polar FAST", dict(solver="polar", precision="fast")), ("Neo-Hookean FAST", dict(solver="neohookean", precision="fast"))):
        free = SoftBodyHIP.batch(meshes, dict(PP), **kw)
        off = median_ms(free)
        free.close()
        for k in PINS:
            held = SoftBodyHIP.batch(meshes, dict(PP), **kw)
            ids = np.linspace(0, len(v) - 1, k).astype(np.int32)   # spread over the body, each held 15 cm below where it starts
            held.setBodyPins(np.tile(ids, (a.bodies, 1)), np.tile(v[ids] - np.float32([0.0, 0.15, 0.0]), (a.bodies, 1, 1)))
            on = median_ms(held)
            lines.append("%-17s %d Dragons, path %d, %d substeps per call, median of %d calls: none held %.4f ms, %3d pins per body %.4f ms, ratio %.4f"
                         % (name, a.bodies, held.info.fused_particle_pass, SUB, CALLS, off, k, on, on / off))
            held.close()
    # a body of the persistent 256-tet frame kernel: with pins on it takes the fused kernels (one graph replay per call)
    from tetsim_amd import make_lattice
    lv, lt = make_lattice(28, y0=0.3)
    kw = dict(solver="polar", precision="fast")
    free = SoftBodyHIP(lv, lt, None, dict(PP), **kw)
    off, path = median_ms(free), free.info.fused_particle_pass
    free.close()
    for k in PINS:
        held = SoftBodyHIP(lv, lt, None, dict(PP), **kw)
        ids = np.linspace(0, len(lv) - 1, k).astype(np.int32)
        held.setBodyPins(ids[None], (lv[ids] - np.float32([0.0, 0.15, 0.0]))[None])
        on = median_ms(held)
        lines.append("polar FAST        28-cell lattice, path %d (frame kernel; fused kernels while pins are on), %d substeps per call: none held %.4f ms, %3d pins %.4f ms, ratio %.4f"
                     % (path, SUB, off, k, on, on / off))
        held.close()
    text = "\n".join(lines)
    print(text)
    if a.out:
        with open(a.out, "w") as f:
            f.write(text + "\n")


if __name__ == "__main__":
    main()
