"""Body parameters (include/tetsim.h: tetsim_set_body_params / _device): what can be checked without a GPU -- the symbols, the row layout,
the Python row builder and the NULL-handle refusal."""
import ctypes as C
import os
import re

import numpy as np

import tetsim_amd
from tetsim_amd import _capi as capi

HEADER = os.path.join(os.path.dirname(os.path.dirname(os.path.abspath(__file__))), "include", "tetsim.h")
DEFAULTS = dict(gravity=-9.81, friction=1000.0, devCompliance=1e-5, volCompliance=0.0, worldBounds=[-2.5, -1.0, -2.5, 2.5, 10.0, 2.5])


def test_the_two_symbols_are_exported():
    L = capi.lib()
    for s in ("tetsim_set_body_params", "tetsim_set_body_params_device"):
        assert s in capi.SYMBOLS and s in capi.OPTIONAL_SYMBOLS and hasattr(L, s), s


def test_a_row_is_a_tetsim_params():
    assert C.sizeof(capi.TetSimParams) == 80 == 8 * capi.BODY_PARAMS_WIDTH
    fields = [f[0] for f in capi.TetSimParams._fields_]
    assert fields == ["gravity", "friction", "devCompliance", "volCompliance", "worldBounds"]
    for name, at in (("gravity", capi.BP_GRAVITY), ("friction", capi.BP_FRICTION), ("devCompliance", capi.BP_DEV_COMPLIANCE),
                     ("volCompliance", capi.BP_VOL_COMPLIANCE), ("worldBounds", capi.BP_BOUNDS_LO)):
        assert getattr(capi.TetSimParams, name).offset == 8 * at, name
    assert capi.BP_BOUNDS_HI == capi.BP_BOUNDS_LO + 3


def test_the_constants_match_the_header():
    text = open(HEADER).read()
    assert int(re.search(r"#define TETSIM_BODY_PARAMS_WIDTH (\d+)", text).group(1)) == capi.BODY_PARAMS_WIDTH == 10
    for name, value in (("GRAVITY", 0), ("FRICTION", 1), ("DEV_COMPLIANCE", 2), ("VOL_COMPLIANCE", 3), ("BOUNDS_LO", 4), ("BOUNDS_HI", 7)):
        assert int(re.search(r"TETSIM_BP_%s = (\d+)" % name, text).group(1)) == value == getattr(capi, "BP_" + name)
    assert "TETSIM_ABI_VERSION 5" in text


def test_body_param_rows_lays_out_the_fields_in_order_and_fills_from_the_defaults():
    own = dict(gravity=-3.0, friction=0.5, devCompliance=1e-4, volCompliance=1e-6, worldBounds=[-1.0, 0.25, -2.0, 1.0, 3.0, 2.0])
    rows = tetsim_amd.body_param_rows([None, own, dict(gravity=2.0)], DEFAULTS)
    assert rows.dtype == np.float64 and rows.shape == (3, 10)
    assert rows[0].tolist() == [-9.81, 1000.0, 1e-5, 0.0, -2.5, -1.0, -2.5, 2.5, 10.0, 2.5]
    assert rows[1].tolist() == [-3.0, 0.5, 1e-4, 1e-6, -1.0, 0.25, -2.0, 1.0, 3.0, 2.0]
    assert rows[2].tolist() == [2.0] + rows[0].tolist()[1:]
    # a row is what make_params makes of the same dict
    p = tetsim_amd.softbody.make_params(own)
    assert np.frombuffer(bytes(p), dtype=np.float64).tolist() == rows[1].tolist()


def test_a_null_handle_is_refused():
    L = capi.lib()
    rows = np.zeros((1, 10))
    assert L.tetsim_set_body_params(None, rows.ctypes.data_as(C.POINTER(C.c_double))) == capi.EINVAL
    assert L.tetsim_set_body_params(None, None) == capi.EINVAL
    assert L.tetsim_set_body_params_device(None, None, 0, None, None) == capi.EINVAL
