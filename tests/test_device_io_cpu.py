"""Device-side export / import (include/tetsim.h: tetsim_export_device, tetsim_import_device), CPU side: the library exports the two
entry points without a new ABI version, the descriptor's C layout and its ctypes mirror agree, a NULL handle is refused before
anything touches a device, and the Python layer stays importable without torch (only the two tensor methods import it)."""
import ctypes as C
import os
import subprocess
import sys

from tetsim_amd import _capi as capi

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))

LAYOUT_C = r"""
#include <stddef.h>
#include <stdio.h>
#include "tetsim.h"
int main(void) {
    printf("%zu %zu %zu %zu %zu %d %d %d %d %d %d %d %d\n", sizeof(TetSimDeviceField), offsetof(TetSimDeviceField, field),
           offsetof(TetSimDeviceField, reserved), offsetof(TetSimDeviceField, dst), offsetof(TetSimDeviceField, row_stride),
           TETSIM_FIELD_POSITIONS, TETSIM_FIELD_VELOCITIES, TETSIM_FIELD_PREV_POSITIONS, TETSIM_FIELD_QUATS, TETSIM_FIELD_VISUAL_POSITIONS,
           TETSIM_FIELD_VISUAL_NORMALS, TETSIM_FIELD_VISUAL_VERTEX_NORMALS, TETSIM_MAX_EXPORT_FIELDS);
    return 0;
}
"""


def test_both_entry_points_are_exported_and_the_abi_version_stays():
    L = capi.lib()
    for name in ("tetsim_export_device", "tetsim_import_device"):
        assert hasattr(L, name), name
        assert name in capi.SYMBOLS
    assert L.tetsim_abi_version() == 5


def test_device_field_is_24_bytes_and_matches_the_ctypes_mirror(tmp_path):
    src, exe = tmp_path / "layout.c", tmp_path / "layout"
    src.write_text(LAYOUT_C)
    r = subprocess.run(["gcc", "-std=c99", "-Wall", "-Werror", "-I" + os.path.join(ROOT, "include"), str(src), "-o", str(exe)], capture_output=True, text=True)
    assert r.returncode == 0, r.stderr
    got = [int(x) for x in subprocess.run([str(exe)], capture_output=True, text=True, check=True).stdout.split()]
    T = capi.TetSimDeviceField
    want = [C.sizeof(T)] + [getattr(T, f).offset for f in ("field", "reserved", "dst", "row_stride")] + \
        [capi.FIELD_POSITIONS, capi.FIELD_VELOCITIES, capi.FIELD_PREV_POSITIONS, capi.FIELD_QUATS, capi.FIELD_VISUAL_POSITIONS,
         capi.FIELD_VISUAL_NORMALS, capi.FIELD_VISUAL_VERTEX_NORMALS, capi.MAX_EXPORT_FIELDS]
    assert got == want
    assert got[0] == 24 and got[5:] == [0, 1, 2, 3, 4, 5, 6, 8]


def test_a_null_handle_is_einval():
    L = capi.lib()
    f = capi.TetSimDeviceField(capi.FIELD_POSITIONS, 0, 16, 0)
    assert L.tetsim_export_device(None, C.byref(f), 1, None) == capi.EINVAL
    assert L.tetsim_export_device(None, None, 0, None) == capi.EINVAL
    assert L.tetsim_import_device(None, 16, 0, 16, 0, None) == capi.EINVAL
    assert L.tetsim_import_device(None, None, 0, None, 0, None) == capi.EINVAL


def test_softbody_imports_without_torch():
    """torch is imported inside exportTensors / importTensors only: with the import blocked the module still loads and offers both."""
    code = ("import sys; sys.modules['torch'] = None\n"
            "import tetsim_amd.softbody as s\n"
            "assert 'torch' not in [k for k, v in sys.modules.items() if v is not None]\n"
            "assert callable(s.SoftBodyHIP.exportTensors) and callable(s.SoftBodyHIP.importTensors)\n"
            "print('ok')")
    r = subprocess.run([sys.executable, "-c", code], cwd=ROOT, capture_output=True, text=True)
    assert r.returncode == 0 and r.stdout.strip() == "ok", r.stderr
