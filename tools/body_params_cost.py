"""What body parameters (tetsim_set_body_params) cost.

Registers (no GPU needed): registers, scalar spills, private segment and waves per SIMD of the kernels that take the table, read from the
.note metadata of the code objects in a build's object directory -- one directory alone, or a parent's build against this one:

    python tools/body_params_cost.py --registers tetsim_amd/csrc/obj [--parent PARENT/tetsim_amd/csrc/obj] [--units body_colliders,body_params]

(--units: every kernel of the named units instead -- the set kernels themselves, profiles/body_rows_refactor.txt.)

Time (MI355X): 64 Dragons in one batch, one call of 20 substeps (timeSubsteps: between HIP events), polar FAST and Neo-Hookean FAST, with
the table ON (every row equal to the call's parameters) against OFF, median of 20 calls after 5 warm-up calls; then the set kernel,
tetsim_set_body_params_device for 64 and for 4,096 bodies, between two events on the caller's stream, median of 20 calls.

    python tools/body_params_cost.py [--bodies 64] [--out FILE]      (--out appends)
"""
import argparse
import glob
import os
import re
import statistics
import subprocess
import sys
import tempfile

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

PP = dict(gravity=-9.81, friction=1000.0, density=1000.0, devCompliance=1e-5, volCompliance=0.0,
          worldBounds=[-2.5, -1.0, -2.5, 2.5, 10.0, 2.5])
DT = (1.0 / 60.0) / 20
SUB, WARM, CALLS = 20, 5, 20
KERNELS = ("pjb_call_kernel", "pjb_frame_kernel", "pjq_frame_kernel", "pjb_vertex_kernel", "pjq_vertex_kernel", "pj_vertex_kernel", "nh_call_kernel", "nh_sweep1_kernel",
           "nh_frame_kernel", "nh_cluster4_kernel", "nh_cluster_kernel", "nh_level4_kernel", "nh_level_kernel", "nh_post_", "nh_predict_")
UNITS = ("pj_blocked", "pj_quad", "pj_fast", "pj_precise", "nh_fast", "nh_precise")


def llvm(tool):
    for d in (os.environ.get("ROCM_PATH", "/opt/rocm") + "/llvm/bin", os.environ.get("ROCM_PATH", "/opt/rocm") + "/lib/llvm/bin"):
        if os.path.exists(os.path.join(d, tool)):
            return os.path.join(d, tool)
    return tool


def kernel_notes(objdir, units=None):
    """{unit: kernel: (vgprs, sgprs, vgpr spills, sgpr spills, private segment)} of the gfx950 code objects of a build"""
    out = {}
    with tempfile.TemporaryDirectory() as tmp:
        for unit in units or UNITS:
            obj = os.path.join(objdir, unit + ".o")
            if not os.path.exists(obj):
                continue
            fb, co = os.path.join(tmp, unit + ".fatbin"), os.path.join(tmp, unit + ".co")
            subprocess.run([llvm("llvm-objcopy"), "-O", "binary", "--only-section=.hip_fatbin", obj, fb], check=True)
            subprocess.run([llvm("clang-offload-bundler"), "--unbundle", "--type=o", "--targets=hipv4-amdgcn-amd-amdhsa--gfx950", "--input=" + fb, "--output=" + co], check=True)
            notes = subprocess.run([llvm("llvm-readelf"), "--notes", co], capture_output=True, text=True, check=True).stdout
            for blk in notes.split("- .agpr_count:")[1:]:
                def field(k):
                    return re.search(r"\." + k + r":\s+(\S+)", blk).group(1)
                name = field("name")
                if not units and not any(k in name for k in KERNELS):
                    continue
                nice = subprocess.run(["c++filt", name], capture_output=True, text=True).stdout.strip()
                nice = re.sub(r"\(.*", "", nice.replace("(anonymous namespace)::", "").replace("void ", "").replace("tetsim::", ""))
                out[unit + ": " + nice] = tuple(int(field(k)) for k in ("vgpr_count", "sgpr_count", "vgpr_spill_count", "sgpr_spill_count", "private_segment_fixed_size"))
    return out


def waves(vgprs):
    return min(8, 512 // (max(vgprs, 1) + 7 & ~7))   # gfx950: 512 registers per lane and SIMD, granted in blocks of 8


def register_table(objdir, parent, units=None):
    mine, theirs = kernel_notes(objdir, units), kernel_notes(parent, units) if parent else {}
    lines = ["kernel: vgprs / sgprs / vgpr spills / sgpr spills / private segment bytes / waves per SIMD by vgprs" + (", parent -> this change" if parent else "")]
    for k in sorted(mine):
        def show(r):
            return "%3d / %3d / %d / %2d / %2d / %d" % (r + (waves(r[0]),))
        lines.append("%-62s %s" % (k, (show(theirs[k]) + "  ->  " if k in theirs else "") + show(mine[k]) + ("" if theirs.get(k, mine[k]) == mine[k] else "   *")))
    return lines


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


def set_kernel_us(bodies):
    import torch
    from tetsim_amd import SoftBodyHIP, body_param_rows
    tet = (np.array([[0, 0.5, 0], [0.5, 0.5, 0], [0, 1.0, 0], [0, 0.5, 0.5]], np.float32), np.array([[0, 1, 2, 3]], np.int32))
    batch = SoftBodyHIP.batch([tet] * bodies, dict(PP), solver="polar", precision="fast")
    rows = torch.from_numpy(body_param_rows([None] * bodies, PP)).cuda()
    batch.setBodyParamsDevice(rows)   # (the first call allocates)
    torch.cuda.synchronize()
    times = []
    for _ in range(CALLS):
        e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        e0.record()
        batch.setBodyParamsDevice(rows)
        e1.record()
        e1.synchronize()
        times.append(e0.elapsed_time(e1) * 1e3)
    batch.close()
    return statistics.median(times)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--bodies", type=int, default=64)
    ap.add_argument("--out", default=None)
    ap.add_argument("--registers", default=None, metavar="OBJDIR")
    ap.add_argument("--parent", default=None, metavar="OBJDIR")
    ap.add_argument("--units", default=None, help="with --registers: comma-separated units, every kernel of each")
    a = ap.parse_args()
    if a.registers:
        lines = register_table(a.registers, a.parent, a.units.split(",") if a.units else None)
    else:
        import torch
        torch.cuda.init()   # (before the library opens the device: torch finds no GPU behind it otherwise)
        from tetsim_amd import SoftBodyHIP
        meshes = [dragon(0.3)] * a.bodies
        lines = []
        for name, kw in (("polar FAST", dict(solver="polar", precision="fast")), ("Neo-Hookean FAST", dict(solver="neohookean", precision="fast"))):
            off, on = (SoftBodyHIP.batch(meshes, dict(PP), **kw) for _ in range(2))
            on.setBodyParams([None] * a.bodies)
            t_off, t_on = median_ms(off), median_ms(on)
            lines.append("%-17s %d Dragons, path %d, one call of %d substeps, median of %d calls: table OFF %.4f ms, ON (every row = the call's parameters) %.4f ms, ON / OFF %.4f"
                         % (name, a.bodies, on.info.fused_particle_pass, SUB, CALLS, t_off, t_on, t_on / t_off))
            print(lines[-1], flush=True)
            off.close()
            on.close()
        for bodies in (64, 4096):
            lines.append("set kernel (tetsim_set_body_params_device, events on the caller's stream), %d bodies: median of %d calls %.1f us" % (bodies, CALLS, set_kernel_us(bodies)))
            print(lines[-1], flush=True)
    text = "\n".join(lines)
    if a.registers:
        print(text)
    if a.out:
        with open(a.out, "a") as f:
            f.write(text + "\n")


if __name__ == "__main__":
    main()
