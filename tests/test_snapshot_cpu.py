"""Device snapshots (include/tetsim.h: tetsim_snapshot_create / _capture / _restore / _destroy), CPU side: the library exports the entry
points without a new ABI version, a NULL handle is refused before anything touches a device, destroying NULL is harmless, and the
Python layer stays importable without torch (only capture / restore import it)."""
import ctypes as C
import os
import subprocess
import sys

from tetsim_amd import _capi as capi

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
NAMES = ("tetsim_snapshot_create", "tetsim_snapshot_capture", "tetsim_snapshot_restore", "tetsim_snapshot_destroy")


def test_the_entry_points_are_exported_and_the_abi_version_stays():
    L = capi.lib()
    for name in NAMES:
        assert hasattr(L, name), name
        assert name in capi.SYMBOLS
    header = open(os.path.join(ROOT, "include", "tetsim.h")).read()
    assert "typedef struct tetsim_snapshot_s *tetsim_snapshot;" in header
    assert L.tetsim_abi_version() == 5


def test_a_null_handle_is_einval_and_destroying_null_is_harmless():
    L = capi.lib()
    out = C.c_void_p()
    assert L.tetsim_snapshot_create(None, C.byref(out)) == capi.EINVAL and not out.value
    assert L.tetsim_snapshot_create(None, None) == capi.EINVAL
    for fn in (L.tetsim_snapshot_capture, L.tetsim_snapshot_restore):
        assert fn(None, None, None, None) == capi.EINVAL
        assert fn(None, 16, 16, None) == capi.EINVAL
    assert L.tetsim_snapshot_destroy(None) is None


def test_softbody_imports_without_torch():
    """torch is imported inside capture / restore only: with the import blocked the module still loads and offers the three methods."""
    code = ("import sys; sys.modules['torch'] = None\n"
            "import tetsim_amd.softbody as s\n"
            "assert 'torch' not in [k for k, v in sys.modules.items() if v is not None]\n"
            "assert callable(s.SoftBodyHIP.snapshot) and callable(s.SoftBodyHIP.capture) and callable(s.SoftBodyHIP.restore)\n"
            "assert callable(s.Snapshot.close)\n"
            "print('ok')")
    r = subprocess.run([sys.executable, "-c", code], cwd=ROOT, capture_output=True, text=True)
    assert r.returncode == 0 and r.stdout.strip() == "ok", r.stderr
