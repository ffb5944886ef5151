"""What a placement costs: 64 Dragons in one batch, placeBodiesDevice with every body chosen and with one body chosen, next to
restore() of the same bodies from a snapshot and to the chip's streaming copy of the same bytes (a device-to-device copy of as many
bytes as the complete state holds; for one body a 64th of them).  Each figure: device time between two events on torch's stream
around 20 calls enqueued back to back, per call, median of 9 such measurements after 3 warm-up rounds.  Polar FAST and Neo-Hookean FAST.

    python tools/place_cost.py [--bodies 64] [--out profiles/place_cost.txt]
"""
import argparse
import ctypes as C
import os
import statistics
import sys

import numpy as np
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

from tetsim_amd import SoftBodyHIP, place_rows  # noqa: E402

PP = dict(gravity=-9.81, friction=1000.0, density=1000.0, devCompliance=1e-5, volCompliance=0.0,
          worldBounds=[-2.5, -1.0, -2.5, 2.5, 10.0, 2.5])
DT = (1.0 / 60.0) / 20
CALLS, WARM, ROUNDS = 20, 3, 9


def dragon(y0):
    gold = os.path.join(ROOT, "tests", "golden")
    v = np.fromfile(os.path.join(gold, "dragon_verts.f32"), dtype="<f4").reshape(-1, 3).copy()
    t = np.fromfile(os.path.join(gold, "dragon_tets.i32"), dtype="<i4").reshape(-1, 4)
    v[:, 1] += np.float32(y0) - v[:, 1].min()
    return v, t


def per_call_us(fn):
    """Device microseconds per call of fn, CALLS calls between two events, median of ROUNDS."""
    got = []
    for r in range(WARM + ROUNDS):
        e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        e0.record()
        for _ in range(CALLS):
            fn()
        e1.record()
        e1.synchronize()
        if r >= WARM:
            got.append(1000.0 * e0.elapsed_time(e1) / CALLS)
    return statistics.median(got)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--bodies", type=int, default=64)
    ap.add_argument("--out", default=None)
    a = ap.parse_args()
    nb = a.bodies
    meshes = [dragon(0.3)] * nb
    lines = []
    for name, kw in (("polar FAST", dict(solver="polar", precision="fast")), ("Neo-Hookean FAST", dict(solver="neohookean", precision="fast", order="clustered"))):
        body = SoftBodyHIP.batch(meshes, dict(PP), **kw)
        body.simulateSubsteps(20, DT, PP)
        size = C.c_uint64()
        body._L.tetsim_state_size(body._h, C.byref(size))
        state_bytes = int(size.value) - 64   # (less the checkpoint's header)
        # a quarter turn about y around the pivot, no offset: four calls bring a body back, so the timed state stays where it is
        rows = torch.from_numpy(place_rows([0.0, np.sqrt(0.5), 0.0, np.sqrt(0.5)], pivot=(0.0, 1.0, 0.0))).repeat(nb, 1).to("cuda")
        every = torch.ones(nb, dtype=torch.bool, device="cuda")
        one = torch.zeros(nb, dtype=torch.bool, device="cuda")
        one[nb // 2] = True
        snap = body.snapshot()
        src, dst = (torch.empty(state_bytes, dtype=torch.uint8, device="cuda") for _ in range(2))
        part = max(1, state_bytes // nb)
        body.placeBodiesDevice(rows, every, keep_velocity=True)   # (the first call uploads the body tables)
        body.restore(snap, every)
        torch.cuda.synchronize()
        t = {"place all": per_call_us(lambda: body.placeBodiesDevice(rows, every, keep_velocity=True)),
             "place one": per_call_us(lambda: body.placeBodiesDevice(rows, one, keep_velocity=True)),
             "restore all": per_call_us(lambda: body.restore(snap, every)),
             "restore one": per_call_us(lambda: body.restore(snap, one)),
             "copy all": per_call_us(lambda: dst.copy_(src)),
             "copy one": per_call_us(lambda: dst[:part].copy_(src[:part]))}
        lines.append("%-17s %d Dragons, path %d, state %d bytes, device us per call (%d calls between two events, median of %d):"
                     % (name, nb, body.info.fused_particle_pass, state_bytes, CALLS, ROUNDS))
        lines.append("    every body: place %.2f, snapshot restore %.2f, streaming copy of %d bytes %.2f" % (t["place all"], t["restore all"], state_bytes, t["copy all"]))
        lines.append("    one body:   place %.2f, snapshot restore %.2f, streaming copy of %d bytes %.2f" % (t["place one"], t["restore one"], part, t["copy one"]))
        snap.close()
        body.close()
    text = "\n".join(lines)
    print(text)
    if a.out:
        with open(a.out, "w") as f:
            f.write(text + "\n")


if __name__ == "__main__":
    main()
