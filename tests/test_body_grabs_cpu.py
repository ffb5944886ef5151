"""Body grabs and the per-body nearest query (include/tetsim.h: tetsim_set_body_grabs / _device, tetsim_nearest_particles_device), as far as a
machine without a GPU can see them: declared, exported, prototyped in the ctypes binding, wrapped by SoftBodyHIP."""
import ctypes as C
import inspect
import os
import re

from conftest import ROOT
from tetsim_amd import SoftBodyHIP
from tetsim_amd import _capi as capi

NEW = ("tetsim_set_body_grabs", "tetsim_set_body_grabs_device", "tetsim_nearest_particles_device")


def test_the_three_symbols_are_declared_and_exported():
    header = open(os.path.join(ROOT, "include", "tetsim.h")).read()
    L = capi.lib()
    for s in NEW:
        assert re.search(r"\bint %s\s*\(tetsim_handle h," % s, header), s
        assert s in capi.SYMBOLS and s in capi.OPTIONAL_SYMBOLS and hasattr(L, s), s
    assert L.tetsim_abi_version() == 5   # additive: the ABI version stays


def test_the_ctypes_prototypes_match_the_header():
    L = capi.lib()
    vp, u64 = C.c_void_p, C.c_uint64
    assert L.tetsim_set_body_grabs.argtypes == [vp, C.POINTER(C.c_int32), C.POINTER(C.c_float)]
    assert L.tetsim_set_body_grabs_device.argtypes == [vp, vp, vp, u64, vp, vp]
    assert L.tetsim_nearest_particles_device.argtypes == [vp, vp, u64, vp, vp, vp]
    for s in NEW:
        assert getattr(L, s).restype == C.c_int, s


def test_a_null_handle_is_refused_without_a_device():
    L = capi.lib()
    assert L.tetsim_set_body_grabs(None, None, None) == capi.EINVAL
    assert L.tetsim_set_body_grabs_device(None, None, None, 0, None, None) == capi.EINVAL
    assert L.tetsim_nearest_particles_device(None, None, 0, None, None, None) == capi.EINVAL


def test_the_python_methods_exist():
    want = {"setBodyGrabs": ["self", "particles", "targets"],
            "setBodyGrabsDevice": ["self", "particles", "targets", "bodies", "stream"],
            "nearestParticlesDevice": ["self", "points", "out_ids", "out_dist2", "stream"]}
    for name, args in want.items():
        assert list(inspect.signature(getattr(SoftBodyHIP, name)).parameters) == args, name


def test_the_out_of_scope_lists_no_longer_name_what_exists():
    header = open(os.path.join(ROOT, "include", "tetsim.h")).read()
    assert "device-resident grab targets" not in header and "per-body grabs" not in header
