"""The one-launch polar call (pj_blocked.hip: pjb_call_kernel) in the order of a host-built dispatch table (host_prep.cpp:
build_call_schedule; TETSIM_PJ_CALL_LAG, read when a body is created): whatever the table's lag, a call equals the tet kernel + particle
kernel pair (TETSIM_PJ_ONE_LAUNCH=0) bit for bit.

Small bodies are forced into the one-launch call by a particle no tet references (fused_particle_pass == 5 at any size), where every
substep's workgroups are resident at once.  Lags 0 (the plain order), 1 and 3 (tables with wrapped particle blocks and held-back tiles on
bodies this small) and one beyond the tile count (falls back to the plain order); calls of 1, 2 and 7 substeps; a checkpoint loaded into a
fresh body.  (No case with a forced small chunk: the call's chunk length has no knob, it follows from the dispatch limit alone --
tests/test_gpu_call_kernel_irregular.py makes the one call long enough to be chunked.)"""
import os

import numpy as np
import pytest

from test_call_schedule import PARTICLES, Tiles
from test_gpu_call_kernel_irregular import DT, LOOSE, PP, _loose, _polar, _same, _tiles
from tetsim_amd import make_lattice

pytestmark = pytest.mark.gpu
CALLS = (1, 2, 7)


def _mesh(name):
    if name == "lattice12":
        v, t = make_lattice(12, y0=0.0001)                     # 10,368 tets, 0.1 mm above the floor: contact inside these calls
        return np.concatenate([v, [LOOSE]]).astype(np.float32), t
    v, t = _loose(31, 2302)
    v = v.copy()
    v[:-1, 1] -= v[:-1, 1].min() - np.float32(0.0001)
    return v, t


def _with_lag(v, t, lag):
    os.environ["TETSIM_PJ_CALL_LAG"] = str(lag)
    try:
        return _polar(v, t)
    finally:
        del os.environ["TETSIM_PJ_CALL_LAG"]


def test_the_lags_of_these_cases_give_other_tables_on_these_meshes():
    """What the bit-equality below is worth: on the very meshes it runs (loose particle included) lags 1 and 3 are laid out -- no fallback --
    and differ from the plain order, with wrapped particle blocks inside the tail (the path of a block whose substep is one period back); host only."""
    for name in ("lattice12", "loose31"):
        v, t = _mesh(name)
        T = Tiles(v, t)
        assert T.nb == _tiles(v, t)
        for lag in (1, 3):
            entry, period, tail, fell, why = T.schedule(lag)
            kind, wrapped = entry >> 30, (entry >> 29) & 1
            assert not fell, (name, lag, why)
            assert not np.array_equal(entry, T.plain()) and tail > 0 and wrapped[kind == PARTICLES].any(), (name, lag)
            assert (kind[:tail] == PARTICLES).any(), (name, lag)
        entry, period, tail, fell, why = T.schedule(T.nb + 1)
        assert fell and np.array_equal(entry, T.plain())


_twins = {}


def _twin(name):
    """The two-kernel twin's state after every call of CALLS, and after the restore case's calls: computed once per body."""
    if name not in _twins:
        v, t = _mesh(name)
        b = _polar(v, t, one_launch=False)
        assert b.info.fused_particle_pass == 0
        after = []
        for n in CALLS:
            b.simulateSubsteps(n, DT, PP)
            after.append((b.pos[:-1].copy(), b.vel[:-1].copy(), b.quats.copy()))
        b.simulateSubsteps(5, DT, PP)
        after.append((b.pos[:-1].copy(), b.vel[:-1].copy(), b.quats.copy()))
        _twins[name] = after
    return _twins[name]


@pytest.mark.parametrize("lag", [0, 1, 3, "more than the tiles"])
@pytest.mark.parametrize("name", ["lattice12", "loose31"])
def test_a_call_in_table_order_equals_the_kernel_pair(name, lag):
    """(The loose particle's row is left out: 0 / 0 on both paths, no parity evidence.)"""
    v, t = _mesh(name)
    L = _tiles(v, t) + 1 if lag == "more than the tiles" else lag
    a = _with_lag(v, t, L)
    assert a.info.fused_particle_pass == 5
    want = _twin(name)
    for k, n in enumerate(CALLS):
        a.simulateSubsteps(n, DT, PP)
        assert _same(a.pos[:-1], want[k][0]) and _same(a.vel[:-1], want[k][1]) and _same(a.quats, want[k][2]), (name, L, n)
    # restore: the blob into a fresh body built with the same lag, one more call
    blob = a.saveState()
    fresh = _with_lag(v, t, L)
    fresh.loadState(blob)
    for x in (a, fresh):
        x.simulateSubsteps(5, DT, PP)
        assert _same(x.pos[:-1], want[3][0]) and _same(x.vel[:-1], want[3][1]) and _same(x.quats, want[3][2]), (name, L, "restore")
    assert np.isfinite(a.pos[:-1]).all() and a.pos[:-1, 1].min() == 0.0   # contact was part of it
