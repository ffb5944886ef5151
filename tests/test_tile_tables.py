"""The tables behind a tile's fixed reduction order (host_prep.cpp: build_blocks, through tetsim_prep_tile_tables; host only).

The 256-tet polar kernels add up a tile particle's corner goals along a LIST of the tile's (corner, tet) pairs sorted by slot: a tet leaves
each corner's goal at the corner's list position (tet_pos: the inverse permutation of the list, 10 bits a corner), a slot adds its run
[run_first[slot], run_first[slot + 1]) front to back, and a list position's run is also where a tet finds its corner's slot.  The four-lane
kernels of small bodies read the same order as entries + ranges (the form the 256-tet kernels read before): the two must say the same.

THE ORDERING RULE.  Inside a slot's run: first the pairs that count (the reference's 36-slot scatter table drops contributions past a
particle's 36th, and one more through its `<= 0.0` quirk), by ascending tet position in the tile, then by corner -- the order of `entries`;
behind them the pairs that do not count, in the same order (the kernels add +0 for them: no sum changes a bit).  Slots are the tile's
particles in ascending id.  The expectation is built from the mesh's tet array alone."""
import ctypes as C
import importlib.util
import os

import numpy as np
import pytest

from tetsim_amd import _capi as capi, make_lattice

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
_spec = importlib.util.spec_from_file_location("record_polar_bits", os.path.join(ROOT, "tools", "record_polar_bits.py"))
rec = importlib.util.module_from_spec(_spec)
_spec.loader.exec_module(rec)

REF_SLOTS = 36


def _ptr(a, t):
    return a.ctypes.data_as(C.POINTER(t))


class Tables:
    def __init__(self, v, t, ref_table):
        L = capi.lib()
        self.v, self.t = np.ascontiguousarray(v, np.float32), np.ascontiguousarray(t, np.int32)
        nt, sizes = len(t), (C.c_uint32 * 2)()
        head = (_ptr(self.v.ravel(), C.c_float), len(v), _ptr(self.t.ravel(), C.c_int32), nt, int(ref_table), sizes)
        assert L.tetsim_prep_tile_tables(*head, *([None] * 9)) == 0
        self.nb, self.ns = sizes[0], sizes[1]
        self.tile_tets, self.tile_off, self.slot_off = np.empty(nt, np.int32), np.empty(self.nb + 1, np.uint32), np.empty(self.nb + 1, np.uint32)
        self.slot_particle, self.corner_slot = np.empty(self.ns, np.int32), np.empty(4 * nt, np.uint8)
        self.entries, self.ranges = np.empty(4 * nt, np.uint16), np.empty(self.ns, np.uint32)
        self.tet_pos, self.run_first = np.empty(2 * nt, np.uint32), np.empty(self.ns + self.nb, np.uint16)
        assert L.tetsim_prep_tile_tables(*head, _ptr(self.tile_tets, C.c_int32), _ptr(self.tile_off, C.c_uint32), _ptr(self.slot_off, C.c_uint32),
                                         _ptr(self.slot_particle, C.c_int32), _ptr(self.corner_slot, C.c_uint8), _ptr(self.entries, C.c_uint16),
                                         _ptr(self.ranges, C.c_uint32), _ptr(self.tet_pos, C.c_uint32), _ptr(self.run_first, C.c_uint16)) == 0
        self.corner_slot = self.corner_slot.reshape(nt, 4)
        w = self.tet_pos.reshape(nt, 2).astype(np.uint64)
        w = w[:, 0] | (w[:, 1] << np.uint64(32))
        self.pos = np.stack([(w >> np.uint64(10 * k)) & np.uint64(1023) for k in range(4)], axis=1).astype(np.int64)      # [tet position][corner]
        self.dropped = np.stack([(w >> np.uint64(40 + k)) & np.uint64(1) for k in range(4)], axis=1).astype(bool)
        assert (w >> np.uint64(44)).max() == 0                                                                            # nothing else in the row


def counted_pairs(t, ref_table):
    """live[tet, corner] from the tet array alone: SoftbodyGPU.js:563-577 fills a particle's 36 slots in tet order, corner order; the slot
    that holds the encoded value 0 (tet 0, corner 0) passes for empty, so the particle's next contribution takes its place"""
    live = np.ones(t.shape, bool)
    if not ref_table:
        return live
    filled = np.zeros(int(t.max()) + 1, np.int64)
    quirk = int(t[0, 0]) if np.count_nonzero(t == t[0, 0]) >= 2 else -1
    for e in range(len(t)):
        for k in range(4):
            p = int(t[e, k])
            if e == 0 and k == 0 and p == quirk:
                live[e, k] = False
                continue
            live[e, k] = filled[p] < REF_SLOTS
            filled[p] += 1
    return live


def irregular():
    return rec.mesh("irregular")


CASES = {"irregular-ref-table": (irregular, 1), "irregular-all": (irregular, 0), "lattice12": (lambda: make_lattice(12), 0),
         "lattice7-ref-table": (lambda: make_lattice(7), 1)}


@pytest.fixture(scope="module", params=list(CASES))
def case(request):
    mesh, ref_table = CASES[request.param]
    v, t = mesh()
    return Tables(v, t, ref_table), counted_pairs(np.asarray(t), ref_table)


def _tiles(T):
    for b in range(T.nb):
        t0, t1, v0, v1 = int(T.tile_off[b]), int(T.tile_off[b + 1]), int(T.slot_off[b]), int(T.slot_off[b + 1])
        yield b, t0, t1 - t0, v0, v1 - v0


def test_the_irregular_case_drops_pairs_and_has_ragged_tiles():
    """what makes the recorded bodies (tools/record_polar_bits.py) and these cases worth their names"""
    v, t = irregular()
    T, live = Tables(v, t, 1), counted_pairs(t, 1)
    assert np.bincount(t.ravel()).max() > REF_SLOTS and 0 < (~live).sum() == T.dropped.sum()
    ntb, nu = np.diff(T.tile_off.astype(np.int64)), np.diff(T.slot_off.astype(np.int64))
    assert ntb[-1] < 256 and nu.min() < 64
    runs = np.concatenate([np.diff(T.run_first[v0 + b:v0 + b + n + 1].astype(np.int64) & 0x7ff) for b, _, _, v0, n in _tiles(T)])
    assert set(runs % 4) == {0, 1, 2, 3} and runs.max() > 16 and runs.min() >= 1
    v, t = rec.mesh("lattice")
    L = Tables(v, t, 0)
    tile_of = np.repeat(np.arange(L.nb), np.diff(L.tile_off.astype(np.int64)))
    pairs = np.unique(np.stack([t[L.tile_tets].ravel(), np.repeat(tile_of, 4)], axis=1), axis=0)
    assert L.nb >= 2048 and np.diff(L.tile_off.astype(np.int64))[-1] < 256 and np.bincount(pairs[:, 0]).max() >= 9


def test_positions_are_a_permutation_and_the_sentinels_close_the_lists(case):
    T, _ = case
    assert T.tile_off[0] == 0 and T.tile_off[T.nb] == len(T.t) and T.slot_off[T.nb] == T.ns
    for b, t0, ntb, v0, nu in _tiles(T):
        assert 1 <= ntb <= 256 and 1 <= nu <= 256
        assert np.array_equal(np.sort(T.pos[t0:t0 + ntb].ravel()), np.arange(4 * ntb)), b
        first = T.run_first[v0 + b:v0 + b + nu + 1].astype(np.int64)
        assert first[0] & 0x7ff == 0 and first[nu] == 4 * ntb, b                 # (the sentinel carries no owner bit)
        assert np.all(np.diff(first & 0x7ff) >= 1), b                            # every slot has a corner: no empty run
        assert np.all(first[:nu] & 0x7800 == 0), b


def test_every_run_lists_its_particles_corners_in_the_order_of_the_entries(case):
    T, live = case
    for b, t0, ntb, v0, nu in _tiles(T):
        tt = T.t[T.tile_tets[t0:t0 + ntb]]                                       # [tet position][corner] -> particle
        lv = live[T.tile_tets[t0:t0 + ntb]]
        particles = T.slot_particle[v0:v0 + nu]
        assert np.array_equal(particles, np.unique(tt)), b                       # slots: the tile's particles, ascending
        first = T.run_first[v0 + b:v0 + b + nu + 1].astype(np.int64) & 0x7ff
        at = np.empty(4 * ntb, np.int64)                                         # list position -> 4 * tet position + corner
        at[T.pos[t0:t0 + ntb].ravel()] = np.arange(4 * ntb)
        assert np.array_equal(T.dropped[t0:t0 + ntb], ~lv), b
        for u in range(nu):
            j, k = np.nonzero(tt == particles[u])                                # ascending tet position, then corner
            want = np.concatenate([4 * j[lv[j, k]] + k[lv[j, k]], 4 * j[~lv[j, k]] + k[~lv[j, k]]])
            got = at[first[u]:first[u + 1]]
            assert np.array_equal(got, want), (b, u)
            assert np.all(T.corner_slot[t0 + got // 4, got % 4] == u), (b, u)    # what a tet reads back from its list positions
            # the counted front of the run is the run of `entries` (corner * 256 + tet position), entry for entry
            r = int(T.ranges[v0 + u])
            ent = T.entries[4 * t0 + (r & 0x7ff):4 * t0 + (r >> 16)].astype(np.int64)
            n_live = int(lv[j, k].sum())
            assert len(ent) == n_live and np.array_equal(4 * (ent % 256) + ent // 256, got[:n_live]), (b, u)


def test_owner_bits_are_the_entries_owner_bits_and_name_the_first_tile_that_counts(case):
    T, live = case
    seen = set()
    for b, t0, ntb, v0, nu in _tiles(T):
        tt, lv = T.t[T.tile_tets[t0:t0 + ntb]], live[T.tile_tets[t0:t0 + ntb]]
        counted = set(np.unique(tt[lv]).tolist())
        own_new = (T.run_first[v0 + b:v0 + b + nu].astype(np.int64) >> 15) & 1
        own_old = (T.ranges[v0:v0 + nu].astype(np.int64) >> 15) & 1
        assert np.array_equal(own_new, own_old), b
        want = np.array([int(p) in counted and int(p) not in seen for p in T.slot_particle[v0:v0 + nu]], np.int64)
        assert np.array_equal(own_new, want), b
        seen |= counted
