"""What body colliders cost when they are ON: 64 Dragons in one batch, one call of 20 substeps (timeSubsteps), every body with its own four
colliders (scene() of tests/test_gpu_colliders.py, f32 values) against the same four colliders as the handle's list and against no
colliders -- median of 20 calls after 5 warm-up calls: polar FAST with and without the lean record (the batch takes the fused tile
kernels), Neo-Hookean FAST (which leaves its single-workgroup launch for the level kernels while the table is on), ONE Dragon and a
batch of 64 small lattices, whose quad tiles leave their persistent frame kernel for two launches per substep while the table is on.
Then the set kernel: tetsim_set_body_colliders_device for 64 and
for 4,096 bodies of eight rows, between two events on the caller's stream, median of 50 calls.

    python tools/body_colliders_cost.py [--bodies 64] [--out profiles/body_colliders_cost.txt]
"""
import argparse
import os
import statistics
import sys

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tests"))

import body_collider_ref as ref  # noqa: E402
from tetsim_amd import SoftBodyHIP, body_collider_rows, make_lattice  # noqa: E402

PP = dict(gravity=-9.81, friction=1000.0, density=1000.0, devCompliance=1e-5, volCompliance=0.0,
          worldBounds=[-2.5, -1.0, -2.5, 2.5, 10.0, 2.5])
DT = (1.0 / 60.0) / 20
SUB, WARM, CALLS = 20, 5, 20


def dragon(y0):
    gold = os.path.join(ROOT, "tests", "golden")
    v = np.fromfile(os.path.join(gold, "dragon_verts.f32"), dtype="<f4").reshape(-1, 3).copy()
    t = np.fromfile(os.path.join(gold, "dragon_tets.i32"), dtype="<i4").reshape(-1, 4)
    v[:, 1] += np.float32(y0) - v[:, 1].min()
    return v, t


def scene(v):
    """scene() of tests/test_gpu_colliders.py (frame 0) in f32 values, lifted 6 cm into the body so that it is met at once"""
    return ref.f32_scene(v + np.float32([0.0, 0.06, 0.0]), 0)


def median_ms(body):
    for _ in range(WARM):
        body.timeSubsteps(SUB, DT, PP)
    return statistics.median(body.timeSubsteps(SUB, DT, PP) for _ in range(CALLS))


def set_kernel_us(bodies):
    import torch
    tet = (np.array([[0, 0.5, 0], [0.5, 0.5, 0], [0, 1.0, 0], [0, 0.5, 0.5]], np.float32), np.array([[0, 1, 2, 3]], np.int32))
    batch = SoftBodyHIP.batch([tet] * bodies, dict(PP), solver="polar", precision="fast")
    rows = torch.from_numpy(body_collider_rows([scene(tet[0]) * 2] * bodies, 8)).cuda()
    batch.setBodyCollidersDevice(rows)   # (the first call allocates)
    torch.cuda.synchronize()
    times = []
    for _ in range(50):
        e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        e0.record()
        batch.setBodyCollidersDevice(rows)
        e1.record()
        e1.synchronize()
        times.append(e0.elapsed_time(e1) * 1e3)
    batch.close()
    return statistics.median(times)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--bodies", type=int, default=64)
    ap.add_argument("--out", default=None)
    a = ap.parse_args()
    import torch
    torch.cuda.init()   # (before the library opens the device: torch finds no GPU behind it otherwise)
    meshes = [dragon(0.3)] * a.bodies
    cols = scene(meshes[0][0])
    lines = []
    small = [make_lattice(4, y0=0.3)] * a.bodies   # 384 tets each: a batch of quad tiles
    for name, kw, count in (("polar FAST", dict(solver="polar", precision="fast"), a.bodies), ("polar FAST lean", dict(solver="polar", precision="fast", lean_state=True), a.bodies),
                            ("Neo-Hookean FAST", dict(solver="neohookean", precision="fast"), a.bodies),
                            ("polar FAST quad", dict(solver="polar", precision="fast"), 1), ("polar FAST quad batch", dict(solver="polar", precision="fast"), -a.bodies)):
        if count < 0:
            meshes, count = small, -count
            cols = scene(meshes[0][0])
        free, shared, own = (SoftBodyHIP.batch(meshes[:count], dict(PP), **kw) for _ in range(3))
        shared.setColliders(cols)
        own.setBodyColliders([cols] * count)
        none, one, per = median_ms(free), median_ms(shared), median_ms(own)
        lines.append("%-21s %d bodies, path %d, %d substeps per call, median of %d calls: no colliders %.4f ms, the handle's list of four %.4f ms, four per body %.4f ms; "
                     "per body / handle's list %.4f, per body / none %.4f" % (name, count, own.info.fused_particle_pass, SUB, CALLS, none, one, per, per / one, per / none))
        print(lines[-1], flush=True)
        for b in (free, shared, own):
            b.close()
    for bodies in (64, 4096):
        lines.append("set kernel (tetsim_set_body_colliders_device, eight rows per body, events on the caller's stream), %d bodies: median of 50 calls %.1f us" % (bodies, set_kernel_us(bodies)))
        print(lines[-1], flush=True)
    text = "\n".join(lines)
    if a.out:
        with open(a.out, "w") as f:
            f.write(text + "\n")


if __name__ == "__main__":
    main()
