"""The one collider routine behind tetsim_set_colliders and tetsim_set_body_colliders (body_rows.h: collider_view / collider_f32), reached
without a GPU through tetsim_prep_collider_views, against its numpy restatement (body_collider_ref.views): the refusal code and every
byte of both views, for the host's doubles and for the same colliders held as a row's f32."""
import ctypes as C

import numpy as np
import pytest

import body_collider_ref as ref
from tetsim_amd import _capi as capi

D_BYTES, F_BYTES = 168, 88
EYE = (1.0, 0.0, 0.0, 0.0, 1.0, 0.0, 0.0, 0.0, 1.0)


def _w(kind, a=(0.0, 0.0, 0.0), b=(0.0, 0.0, 0.0), axes=EYE, radius=0.0, friction=0.0, velocity=(0.0, 0.0, 0.0)):
    """21 doubles in a row's order"""
    return np.concatenate([[kind], a, b, axes, [radius, friction], velocity]).astype(np.float64)


def _library(ws, as_rows):
    """[(code, f64 bytes, f32 bytes)] of the library for colliders given as 21 doubles each"""
    arr = (capi.TetSimCollider * len(ws))()
    for c, w in zip(arr, ws):
        c.kind, c.reserved = int(w[0]), 0
        c.a[:], c.b[:], c.axes[:], c.velocity[:] = w[1:4].tolist(), w[4:7].tolist(), w[7:16].tolist(), w[18:21].tolist()
        c.radius, c.friction = float(w[16]), float(w[17])
    codes = np.full(len(ws), -1, np.int32)
    d, f = np.full(len(ws) * D_BYTES, 0xAA, np.uint8), np.full(len(ws) * F_BYTES, 0xAA, np.uint8)
    assert capi.lib().tetsim_prep_collider_views(arr, len(ws), int(as_rows), codes.ctypes.data_as(C.POINTER(C.c_int32)), d.ctypes.data, f.ctypes.data) == 0
    return [(int(codes[k]), d[k * D_BYTES:(k + 1) * D_BYTES].tobytes(), f[k * F_BYTES:(k + 1) * F_BYTES].tobytes()) for k in range(len(ws))]


def _expected(w, as_rows):
    with np.errstate(over="ignore", invalid="ignore"):
        w = w.astype(np.float32).astype(np.float64) if as_rows else w
    code, d, f = ref.views(w)
    return (code, d, f) if code == 0 else (code, bytes(D_BYTES), bytes(F_BYTES))


def _check(ws, as_rows):
    for k, (got, w) in enumerate(zip(_library(ws, as_rows), ws)):
        assert got == _expected(w, as_rows), (k, as_rows, w.tolist())


def _skewed(eps):
    """a box whose axes are not unit vectors, the second leaning on the first by eps after normalisation"""
    return _w(2, a=(0.1, 0.2, 0.3), b=(0.5, 0.25, 1.0), axes=(2.0, 0.0, 0.0, 3.0 * eps, 3.0, 0.0, 0.0, 0.0, 0.5), friction=3.0)


VALID = [_w(0, a=(0.1, -0.2, 0.3), radius=0.25, friction=12.5, velocity=(0.1, 0.0, -0.3)),
         _w(1, a=(0.0, 0.1, 0.0), b=(0.3, 0.1, 0.7), radius=0.05, friction=1.0),
         _w(2, a=(1.0, 2.0, 3.0), b=(0.3, 0.2, 0.1), axes=(0.0, 0.3, 0.0, 0.0, 0.0, 7.0, 1e-3, 0.0, 0.0), radius=-1.0, friction=100.0),
         _w(3, a=(0.0, -1.0, 0.0), b=(0.1, 3.0, -0.2), radius=-5.0, friction=0.5, velocity=(0.0, 0.2, 0.0))]
# one per refusal, in the order of the codes: each passes every earlier check
REFUSED = [_w(7, radius=0.1),
           _w(0, axes=(1.0, 0.0, 0.0, 0.0, np.inf, 0.0, 0.0, 0.0, 1.0), radius=0.1),      # in a field a sphere does not use
           _w(1, radius=-0.1),
           _w(3, b=(0.0, 0.0, 0.0), radius=-1.0),
           _w(2, b=(0.1, -0.1, 0.1)),
           _w(2, b=(0.1, 0.1, 0.1), axes=(1.0, 0.0, 0.0, 0.0, 1.0, 0.0, 0.0, 0.0, 0.0)),
           _w(2, b=(0.1, 0.1, 0.1), axes=(1.0, 0.0, 0.0, 0.01, 1.0, 0.0, 0.0, 0.0, 1.0))]


@pytest.mark.parametrize("as_rows", [0, 1])
def test_one_valid_collider_of_each_kind(as_rows):
    assert [ref.views(w)[0] for w in VALID] == [0, 0, 0, 0]
    _check(VALID, as_rows)


@pytest.mark.parametrize("as_rows", [0, 1])
def test_nearly_orthogonal_axes_on_either_side_of_the_bound(as_rows):
    inside, outside = _skewed(0.99e-5), _skewed(1.01e-5)
    got = _library([inside, outside], as_rows)
    assert [g[0] for g in got] == [0, 7]
    _check([inside, outside], as_rows)


@pytest.mark.parametrize("as_rows", [0, 1])
def test_one_collider_per_refusal_code(as_rows):
    got = _library(REFUSED, as_rows)
    assert [g[0] for g in got] == [1, 2, 3, 4, 5, 6, 7]
    for g, w in zip(got, REFUSED):   # ... which are the codes the rows' reference has for the same numbers as a 24-float row
        row = np.zeros(ref.FLOATS, np.float32)
        row[:21] = w
        assert g[0] == ref.refusal(row) and g[1] == bytes(D_BYTES) and g[2] == bytes(F_BYTES)
    assert len(ref.REFUSALS) == 8


def _random_valid(rng):
    def mag(n=None):   # 1e-6 .. 1e6, either sign
        return rng.choice([-1.0, 1.0], n) * 10.0 ** rng.uniform(-6.0, 6.0, n)
    kind = int(rng.integers(0, 4))
    q, _ = np.linalg.qr(rng.normal(size=(3, 3)))
    axes = (q * np.abs(mag(3))[:, None]).reshape(9) if kind == 2 else mag(9)
    b = np.abs(mag(3)) if kind == 2 else mag(3)
    return _w(kind, a=mag(3), b=b, axes=axes, radius=abs(mag()) if kind < 2 else mag(), friction=abs(mag()), velocity=mag(3))


@pytest.mark.parametrize("as_rows", [0, 1])
def test_random_valid_colliders(as_rows):
    rng = np.random.default_rng(20)
    ws = [_random_valid(rng) for _ in range(300)]
    got = _library(ws, as_rows)
    assert [g[0] for g in got] == [0] * len(ws)
    assert sorted({int(w[0]) for w in ws}) == [0, 1, 2, 3]
    _check(ws, as_rows)
    # the f32 rounding is exercised: the f32 view is not the f64 view's values for nearly every collider -- of a row's f32 fields, for
    # nearly every box and plane, whose normalised vectors are new f64 values
    rounded = [np.frombuffer(g[2][:80], "<f4").astype(np.float64).tobytes() != g[1][:160] for g in got]
    normalised = [w[0] >= 2.0 for w in ws]
    assert sum(r for r, n in zip(rounded, normalised) if n or not as_rows) > 0.9 * (sum(normalised) if as_rows else len(ws))
