"""Which kernels the stepping entry points launch, in which order: every stepping path at its smallest mesh (CASES of
tests/test_gpu_collider_pass.py), the same calls in a fixed order.  A recording tool: it asserts nothing and compares nothing itself.

    rocprofv3 --kernel-trace --output-format csv -d OUT -- python tools/step_kernel_sequence.py        # the trace
    python tools/step_kernel_sequence.py --sequence OUT > sequence.txt                                   # its kernels, one line each

Run both at two commits and diff the two sequence files: a host-side refactor must leave them equal line for line
(profiles/step_host_refactor.txt).  Per path: tetsim_step twice, tetsim_step_n of 4 twice, tetsim_profile of 2; body colliders on, step and
step_n, off, step_n; the same with body pins.  A switch a path refuses is printed and skipped."""
import csv
import glob
import os
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tests"))


def sequence(out_dir):
    """kernel name, grid and workgroup of every dispatch of the trace under out_dir, in the order they were dispatched"""
    rows = []
    for path in glob.glob(os.path.join(out_dir, "**", "*kernel_trace.csv"), recursive=True):
        with open(path, newline="") as f:
            rows += list(csv.DictReader(f))
    rows.sort(key=lambda r: int(r["Dispatch_Id"]))
    for r in rows:
        print("%s grid %s %s %s block %s %s %s" % (r["Kernel_Name"], r["Grid_Size_X"], r["Grid_Size_Y"], r["Grid_Size_Z"],
                                                   r["Workgroup_Size_X"], r["Workgroup_Size_Y"], r["Workgroup_Size_Z"]))


def walk():
    import numpy as np
    from test_gpu_collider_pass import CASES, DT, mesh
    from tetsim_amd import SoftBodyHIP, TetSimError

    def switched(body, what, on, off):
        try:
            on()
        except TetSimError as e:
            print("  %s refused: %s" % (what, e))
            return
        body.simulate(DT, pp)
        body.simulateSubsteps(4, DT, pp)
        off()
        body.simulateSubsteps(4, DT, pp)
        body.sync()

    for case, (name, kw, _, pp) in CASES.items():
        v, t = mesh(name)
        body = SoftBodyHIP(v, t, None, dict(pp), **kw)
        print("%s: path %d" % (case, body.info.fused_particle_pass))
        for _ in range(2):
            body.simulate(DT, pp)
        for _ in range(2):
            body.simulateSubsteps(4, DT, pp)
        body.profile(2, DT, pp)
        body.sync()
        sphere = dict(kind="sphere", a=[0.0, 0.1, 0.0], radius=0.2, friction=50.0)
        switched(body, "body colliders", lambda: body.setBodyColliders([[sphere]]), lambda: body.setBodyColliders(None))
        switched(body, "body pins", lambda: body.setBodyPins(np.int32([[int(t[0, 0])]]), np.float32([[v[t[0, 0]]]])), lambda: body.setBodyPins(None, None))
        body.close()


if __name__ == "__main__":
    if len(sys.argv) == 3 and sys.argv[1] == "--sequence":
        sequence(sys.argv[2])
    else:
        walk()
