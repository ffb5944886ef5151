"""TETSIM_ORDER_CLUSTERED schedule (host_prep.cpp prep_clusters), checked on the CPU: the plan is a permutation, and any two
tets that share a vertex are solved in their sequential order -- by different launches, or by ONE lane in step order."""
import ctypes as C

import numpy as np
import pytest

from conftest import load_mesh
from tetsim_amd import _capi as capi, make_lattice


def plan(t, nv):
    L = capi.lib()
    t = np.ascontiguousarray(t, np.int32)
    nt = len(t)
    out = [np.full(nt, -1, np.int32) for _ in range(4)]
    nl, nc = C.c_uint32(), C.c_uint32()
    ip = lambda a: a.ctypes.data_as(C.POINTER(C.c_int32))
    assert L.tetsim_prep_clusters(ip(t.ravel()), nt, nv, *[ip(a) for a in out], C.byref(nl), C.byref(nc)) == 0
    return (*out, nl.value, nc.value)


def check(t, order, launch, lane, step):
    assert np.array_equal(np.sort(order), np.arange(len(t)))
    seq = t[order]
    # every two consecutive touches of a vertex in sequential order: a later launch, or the same lane at a later step
    pos = np.repeat(np.arange(len(seq)), 4)
    by_vertex = np.lexsort((pos, seq.ravel()))
    vx, px = seq.ravel()[by_vertex], pos[by_vertex]
    same = vx[1:] == vx[:-1]
    a, b = px[:-1][same], px[1:][same]
    ok = (launch[a] < launch[b]) | ((launch[a] == launch[b]) & (lane[a] == lane[b]) & (step[a] < step[b]))
    assert ok.all(), (a[~ok][:5], b[~ok][:5])
    # a lane's cluster: at most 8 tets over at most 8 vertices; steps are 0..n-1 without holes
    key = launch.astype(np.int64) * (1 << 32) + lane
    _, inv, count = np.unique(key, return_inverse=True, return_counts=True)
    assert count.max(initial=0) <= 8
    pairs = np.unique(np.stack([np.repeat(inv, 4), seq.ravel()], axis=1), axis=0)
    assert np.bincount(pairs[:, 0], minlength=len(count)).max(initial=0) <= 8
    by_key = np.lexsort((step, inv))
    first = np.concatenate([[0], np.cumsum(count)[:-1]])
    assert np.array_equal(step[by_key], np.arange(len(t)) - np.repeat(first, count))


def test_lattice_cells_become_clusters():
    v, t = make_lattice(7)
    order, launch, lane, step, nl, nc = plan(t, len(v))
    check(t, order, launch, lane, step)
    assert nl == 8 and nc == 7 ** 3 and step.max() == 5   # one cluster per cell, 2x2x2 cell parities as colours


def test_dragon_and_random_meshes():
    v, t = load_mesh("dragon")
    order, launch, lane, step, nl, nc = plan(t, len(v))
    check(t, order, launch, lane, step)
    assert nl < 32 and nc < len(t) / 3
    rng = np.random.default_rng(7)
    for nv, nt in ((5, 1), (9, 40), (200, 900)):
        t = np.array([rng.choice(nv, 4, replace=False) for _ in range(nt)], np.int32)
        order, launch, lane, step, nl, nc = plan(t, nv)
        check(t, order, launch, lane, step)


def test_empty_mesh():
    order, launch, lane, step, nl, nc = plan(np.zeros((0, 4), np.int32), 0)
    assert nl == 0 and nc == 0


def fan(m, y0=0.05, r=0.3, h=0.2):
    """m tets around one edge (the axis from (0, y0, 0) to (0, y0 + h, 0)) over a closed ring of m points, every tet of positive volume.
    The planner's cluster is five consecutive tets (two axis points and six ring points): ceil(m / 5) clusters, one colour each."""
    a = np.arange(m) * (2.0 * np.pi / m)
    ring = np.stack([r * np.cos(a), np.full(m, y0 + 0.5 * h), r * np.sin(a)], axis=1)
    v = np.concatenate([[[0.0, y0, 0.0], [0.0, y0 + h, 0.0]], ring]).astype(np.float32)
    i = np.arange(m)
    t = np.stack([np.zeros(m), np.ones(m), 2 + i, 2 + (i + 1) % m], axis=1).astype(np.int32)
    d = v[t[:, 1:]].astype(np.float64) - v[t[:, :1]].astype(np.float64)
    flip = np.linalg.det(d) < 0
    t[flip] = t[flip][:, [0, 1, 3, 2]]
    return v, t


# the clustered FAST Neo-Hookean paths change at these colour counts (tetsim_create.hip): the call as one launch up to 127 colours
# (its 8-bit hand-over distances reach back up to 2 x colours - 1), the sweep as one launch up to 255, one launch per colour beyond
FANS = [(635, 127), (636, 128), (1275, 255), (1276, 256)]


@pytest.mark.parametrize("m,colours", FANS)
def test_fans_reach_the_colour_thresholds(m, colours):
    v, t = fan(m)
    d = v[t[:, 1:]].astype(np.float64) - v[t[:, :1]].astype(np.float64)
    assert (np.linalg.det(d) > 0).all()
    order, launch, lane, step, nl, nc = plan(t, len(v))
    check(t, order, launch, lane, step)
    assert nl == colours and nc == colours


def test_large_delaunay_mesh():
    """The 604,715-tet Delaunay body of the one-launch tests: 35 colours, from one cluster to ~6 k."""
    from test_gpu_call_kernel_irregular import _delaunay
    v, t = _delaunay()
    assert len(t) == 604715
    order, launch, lane, step, nl, nc = plan(t, len(v))
    check(t, order, launch, lane, step)
    per_colour = np.array([len(np.unique(lane[launch == l])) for l in range(nl)])
    assert nl == 35 and per_colour.min() == 1 and per_colour.max() > 6000 and per_colour.sum() == nc
